// scan_export.hip -- ScanNet scan export on the device: a raw scan's mesh, labels, segments and aggregation to the per-scan arrays
// of the reference's data/scannet/prepare_scannet.py (export :138-178, process_one_scan :180-197, helpers :29-135) and the instance
// GT codes of prepare_scannet_inst_gt.py:38-65, driven by d3net_amd/scan_export.py.
//
// Two stages:
//   * d3_scan_mesh: the (N, 9) mesh (xyz, rgb, vertex normals, scannet_utils.py:117-136 / compute_normal :29-48) and its axis-aligned
//     copy (prepare_scannet.py:36-52).  Face normals are float32 in np.cross / normalize_v3 order.  The per-vertex accumulation
//     `normals[faces[:, c]] += n` is numpy's buffered fancy-index update: per corner c only the LAST face that names a vertex at
//     that corner contributes.  That face is found with an integer atomicMax on the face index, so the result does not depend on
//     scheduling.  The alignment is fp64 in the fixed order ((x m0 + y m1) + z m2) + m3, rounded to float32.
//   * d3_scan_labels: instance ids, remapped semantic labels, instance boxes of both meshes and instance GT codes
//     (prepare_scannet.py:23-25, :107-135, :183-191).  A segment claimed by several objects goes to the last one in dict order
//     (atomicMax on the order index), an object's label is the raw label of the first vertex (atomicMin) of its last listed
//     segment, box extents are integer atomics on order-preserving float keys, reduced per workgroup in LDS first.
// Only integer atomics, no float atomics: every output is bitwise reproducible.  The library builds with -ffp-contract=off, so
// tests/scan_export_restate.py restates every float operation in numpy.
#include "common.h"

#define SX_MAX_VERTICES (1 << 24)
#define SX_MAX_FACES (1 << 25)
#define SX_MAX_SEGMENTS (1 << 24)  // segment ids 0 .. S-1
#define SX_MAX_OBJECTS 1024        // objects kept from the aggregation (the LDS box table of sx_vertex_kernel)
#define SX_MAX_ROWS 65536          // box rows = max objectId + 1
#define SX_MAX_PAIRS (1 << 24)     // (segment, object) pairs listed by the aggregation
#define SX_BLOCK 256
#define SX_VREC 16                 // vertex record: float x, y, z; uchar red, green, blue, alpha
#define SX_FREC 13                 // face record: uchar count (3); int32 vertex_indices[3], unaligned
#define SX_NLABEL 150              // remapper size (prepare_scannet.py:23)
#define SX_SENT 0x7f7f7f7f         // "no vertex" of the atomicMin tables (memset byte 0x7f)

// flag bits of flags[0] (d3net_amd/scan_export.py names them)
#define SX_BAD_FACE_COUNT 1
#define SX_BAD_FACE_INDEX 2
#define SX_BAD_LABEL 4
#define SX_BAD_SEGMENT 8
#define SX_MISSING_SEGMENT 16
#define SX_BAD_TABLE 32            // pair_obj outside [0, K), obj_id outside [0, R) or repeated: the entry is skipped

int d3_scan_limits(int *max_vertices, int *max_faces, int *max_segments, int *max_objects, int *max_rows) {
    if (max_vertices) *max_vertices = SX_MAX_VERTICES;
    if (max_faces) *max_faces = SX_MAX_FACES;
    if (max_segments) *max_segments = SX_MAX_SEGMENTS;
    if (max_objects) *max_objects = SX_MAX_OBJECTS;
    if (max_rows) *max_rows = SX_MAX_ROWS;
    return 0;
}

static inline int sx_blocks(long long n, int per) {
    long long g = (n + per - 1) / per;
    return (int)(g < 1 ? 1 : g);
}

// the reference's remapper: nyu40 ids of the 20 benchmark classes -> 0..19, everything else -> -1
__device__ __forceinline__ int sx_remap(int raw) {
    switch (raw) {
    case 1: return 0;   case 2: return 1;   case 3: return 2;   case 4: return 3;   case 5: return 4;
    case 6: return 5;   case 7: return 6;   case 8: return 7;   case 9: return 8;   case 10: return 9;
    case 11: return 10; case 12: return 11; case 14: return 12; case 16: return 13; case 24: return 14;
    case 28: return 15; case 33: return 16; case 34: return 17; case 36: return 18; case 39: return 19;
    default: return -1;
    }
}

// semantic_label_idxs of prepare_scannet_inst_gt.py:15 (inverse of sx_remap)
__device__ __forceinline__ int sx_nyu40(int sem) {
    const int idx[20] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 16, 24, 28, 33, 34, 36, 39};
    return sem < 0 ? 0 : idx[sem];
}

// order-preserving float32 <-> uint32 keys (unsigned comparison == float comparison, -0.0 below +0.0)
__device__ __forceinline__ unsigned sx_key(float f) {
    unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float sx_unkey(unsigned k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// ---- stage 1: mesh ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void sx_vertex_xyz(const unsigned char *__restrict__ vrec, int v, float *p) {
    const float *r = (const float *)(vrec + (size_t)v * SX_VREC);
    p[0] = r[0]; p[1] = r[1]; p[2] = r[2];
}

__device__ __forceinline__ int sx_face_index(const unsigned char *r) {
    return (int)((unsigned)r[0] | ((unsigned)r[1] << 8) | ((unsigned)r[2] << 16) | ((unsigned)r[3] << 24));
}

// np.cross(v1 - v0, v2 - v0) then normalize_v3 (scannet_utils.py:21-27, :35-38): products rounded one by one, len computed once,
// every component divided by len + 1e-8f.  Also records, per corner c, the last face naming each vertex (atomicMax).
__global__ __launch_bounds__(SX_BLOCK) void sx_face_kernel(const unsigned char *__restrict__ vrec, int N,
                                                           const unsigned char *__restrict__ frec, int F, float *__restrict__ fn,
                                                           int *__restrict__ last, int *__restrict__ flags) {
    int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F) return;
    const unsigned char *r = frec + (size_t)f * SX_FREC;
    int idx[3] = {sx_face_index(r + 1), sx_face_index(r + 5), sx_face_index(r + 9)};
    int bad = 0;
    if (r[0] != 3) bad |= SX_BAD_FACE_COUNT;
    for (int c = 0; c < 3; c++)
        if (idx[c] < 0 || idx[c] >= N) bad |= SX_BAD_FACE_INDEX;
    if (bad) {
        atomicOr(flags, bad);
        fn[3 * (size_t)f] = 0.0f; fn[3 * (size_t)f + 1] = 0.0f; fn[3 * (size_t)f + 2] = 0.0f;
        return;
    }
    float p0[3], p1[3], p2[3];
    sx_vertex_xyz(vrec, idx[0], p0);
    sx_vertex_xyz(vrec, idx[1], p1);
    sx_vertex_xyz(vrec, idx[2], p2);
    float a[3] = {p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]};
    float b[3] = {p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2]};
    float n0 = a[1] * b[2] - a[2] * b[1];
    float n1 = a[2] * b[0] - a[0] * b[2];
    float n2 = a[0] * b[1] - a[1] * b[0];
    float len = sqrtf((n0 * n0 + n1 * n1) + n2 * n2);
    float d = len + 1e-8f;
    fn[3 * (size_t)f] = n0 / d;
    fn[3 * (size_t)f + 1] = n1 / d;
    fn[3 * (size_t)f + 2] = n2 / d;
    for (int c = 0; c < 3; c++) atomicMax(&last[(size_t)c * N + idx[c]], f);
}

struct SxAlign {
    double m[16];
    int on;
};

// mesh row v: xyz, rgb (0-255 as float), normals; aligned row: aligned xyz (or a copy), rgb, normals.  The normal is
// ((0 + n[last0]) + n[last1]) + n[last2] over the corners that name v, normalised like a face normal.
__global__ __launch_bounds__(SX_BLOCK) void sx_vertex_mesh_kernel(const unsigned char *__restrict__ vrec, int N,
                                                                  const float *__restrict__ fn, const int *__restrict__ last, SxAlign al,
                                                                  float *__restrict__ mesh, float *__restrict__ aligned) {
    int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= N) return;
    const unsigned char *r = vrec + (size_t)v * SX_VREC;
    const float *rf = (const float *)r;
    float x = rf[0], y = rf[1], z = rf[2];
    float cr = (float)r[12], cg = (float)r[13], cb = (float)r[14];
    float acc[3] = {0.0f, 0.0f, 0.0f};
    for (int c = 0; c < 3; c++) {
        int f = last[(size_t)c * N + v];
        if (f >= 0) {
            acc[0] = acc[0] + fn[3 * (size_t)f];
            acc[1] = acc[1] + fn[3 * (size_t)f + 1];
            acc[2] = acc[2] + fn[3 * (size_t)f + 2];
        }
    }
    float len = sqrtf((acc[0] * acc[0] + acc[1] * acc[1]) + acc[2] * acc[2]);
    float d = len + 1e-8f;
    float nx = acc[0] / d, ny = acc[1] / d, nz = acc[2] / d;
    float ax = x, ay = y, az = z;
    if (al.on) {
        double dx = (double)x, dy = (double)y, dz = (double)z;
        ax = (float)(((dx * al.m[0] + dy * al.m[1]) + dz * al.m[2]) + al.m[3]);
        ay = (float)(((dx * al.m[4] + dy * al.m[5]) + dz * al.m[6]) + al.m[7]);
        az = (float)(((dx * al.m[8] + dy * al.m[9]) + dz * al.m[10]) + al.m[11]);
    }
    float *m = mesh + 9 * (size_t)v, *a = aligned + 9 * (size_t)v;
    m[0] = x;  m[1] = y;  m[2] = z;  m[3] = cr; m[4] = cg; m[5] = cb; m[6] = nx; m[7] = ny; m[8] = nz;
    a[0] = ax; a[1] = ay; a[2] = az; a[3] = cr; a[4] = cg; a[5] = cb; a[6] = nx; a[7] = ny; a[8] = nz;
}

struct SxMeshWs { int *last; float *fn; };
static void sx_mesh_layout(D3Carver &c, int N, int F, SxMeshWs &w) {
    w.last = c.take<int>((size_t)3 * N);
    w.fn = c.take<float>((size_t)3 * (F > 0 ? F : 1));
}

size_t d3_scan_mesh_ws_bytes(int N, int F) {
    if (N < 1 || N > SX_MAX_VERTICES || F < 0 || F > SX_MAX_FACES) return 0;
    D3Carver c(nullptr, 0);
    SxMeshWs w;
    sx_mesh_layout(c, N, F, w);
    return c.off;
}

int d3_scan_mesh(const void *vertex_rec, int N, const void *face_rec, int F, const double *align_host, float *mesh, float *aligned_mesh,
                 int *flags, void *ws, size_t ws_bytes, void *stream) {
    if (N < 1 || N > SX_MAX_VERTICES || F < 0 || F > SX_MAX_FACES) return D3_ERR_RANGE;
    if (!vertex_rec || (F > 0 && !face_rec) || !mesh || !aligned_mesh || !flags || !ws) return D3_ERR_ARG;
    if (((uintptr_t)vertex_rec & 3) != 0) return D3_ERR_ARG;
    D3Carver cv(ws, ws_bytes);
    SxMeshWs w;
    sx_mesh_layout(cv, N, F, w);
    if (!cv.ok()) return D3_ERR_WORKSPACE;
    int *last = w.last;
    float *fn = w.fn;
    SxAlign al;
    al.on = align_host != nullptr;
    for (int i = 0; i < 16; i++) al.m[i] = align_host ? align_host[i] : 0.0;
    hipStream_t st = d3_stream(stream);
    D3_CLEAR();
    D3_CHECK(hipMemsetAsync(last, 0xff, (size_t)3 * N * 4, st));
    if (F > 0)
        hipLaunchKernelGGL(sx_face_kernel, dim3(sx_blocks(F, SX_BLOCK)), dim3(SX_BLOCK), 0, st, (const unsigned char *)vertex_rec, N,
                           (const unsigned char *)face_rec, F, fn, last, flags);
    hipLaunchKernelGGL(sx_vertex_mesh_kernel, dim3(sx_blocks(N, SX_BLOCK)), dim3(SX_BLOCK), 0, st, (const unsigned char *)vertex_rec,
                       N, fn, last, al, mesh, aligned_mesh);
    D3_LAUNCH_CHECK();
    return 0;
}

// ---- stage 2: labels, instances, boxes ------------------------------------------------------------------------------------------
// seg_first[s] = min vertex carrying segment s; flags raw labels outside the remapper and segment ids outside [0, S)
__global__ __launch_bounds__(SX_BLOCK) void sx_seg_first_kernel(const unsigned short *__restrict__ raw, const int *__restrict__ seg,
                                                                int N, int S, int *__restrict__ seg_first, int *__restrict__ flags) {
    int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= N) return;
    int s = seg[v], bad = 0;
    if (raw[v] >= SX_NLABEL) bad |= SX_BAD_LABEL;
    if (s < 0 || s >= S) bad |= SX_BAD_SEGMENT;
    else atomicMin(&seg_first[s], v);
    if (bad) atomicOr(flags, bad);
}

// seg_owner[s] = the last object (dict order index) that lists s; a listed segment that no vertex carries is the reference's KeyError
__global__ __launch_bounds__(SX_BLOCK) void sx_pair_kernel(const int *__restrict__ pair_seg, const int *__restrict__ pair_obj, int P,
                                                           int S, int K, const int *__restrict__ seg_first, int *__restrict__ seg_owner,
                                                           int *__restrict__ flags) {
    int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    int s = pair_seg[p], k = pair_obj[p];
    if (k < 0 || k >= K) {         // seg_owner feeds the LDS tables and obj_id: only [0, K) may enter it
        atomicOr(flags, SX_BAD_TABLE);
        return;
    }
    if (s < 0 || s >= S || seg_first[s] == SX_SENT) {
        atomicOr(flags, SX_MISSING_SEGMENT);
        return;
    }
    atomicMax(&seg_owner[s], k);
}

__device__ __forceinline__ int sx_owner(const int *__restrict__ seg, const int *__restrict__ seg_owner, int S, int v) {
    int s = seg[v];
    return (s >= 0 && s < S) ? seg_owner[s] : -1;
}

// per vertex: instance id and remapped label (float64, as the reference saves them); per object: first vertex and the min / max
// keys of xyz in both meshes, reduced in LDS per workgroup (one global atomic per touched entry and workgroup)
__global__ __launch_bounds__(SX_BLOCK) void sx_vertex_kernel(const unsigned short *__restrict__ raw, const int *__restrict__ seg, int N,
                                                             int S, const int *__restrict__ seg_owner, const int *__restrict__ obj_id,
                                                             int K, const float *__restrict__ mesh, const float *__restrict__ aligned,
                                                             double *__restrict__ ids, double *__restrict__ sem, int *__restrict__ kfirst,
                                                             unsigned *__restrict__ kmin, unsigned *__restrict__ kmax) {
    extern __shared__ unsigned sx_lds[];
    unsigned *lfirst = sx_lds, *lmin = sx_lds + K, *lmax = sx_lds + 7 * K;
    for (int i = threadIdx.x; i < K; i += blockDim.x) lfirst[i] = SX_SENT;
    for (int i = threadIdx.x; i < 6 * K; i += blockDim.x) {
        lmin[i] = 0xffffffffu;
        lmax[i] = 0u;
    }
    __syncthreads();
    for (long long v0 = (long long)blockIdx.x * blockDim.x; v0 < N; v0 += (long long)gridDim.x * blockDim.x) {
        int v = (int)v0 + threadIdx.x;
        if (v >= N) break;
        int o = sx_owner(seg, seg_owner, S, v);
        int r = raw[v];
        ids[v] = o >= 0 ? (double)obj_id[o] : -1.0;
        sem[v] = (double)(r < SX_NLABEL ? sx_remap(r) : -1);
        if (o >= 0) {
            atomicMin(&lfirst[o], (unsigned)v);
            const float *m = mesh + 9 * (size_t)v, *a = aligned + 9 * (size_t)v;
            for (int j = 0; j < 3; j++) {
                unsigned km = sx_key(m[j]), ka = sx_key(a[j]);
                atomicMin(&lmin[6 * o + j], km);
                atomicMax(&lmax[6 * o + j], km);
                atomicMin(&lmin[6 * o + 3 + j], ka);
                atomicMax(&lmax[6 * o + 3 + j], ka);
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < K; i += blockDim.x)
        if (lfirst[i] != SX_SENT) atomicMin(&kfirst[i], (int)lfirst[i]);
    for (int i = threadIdx.x; i < 6 * K; i += blockDim.x) {
        if (lmin[i] != 0xffffffffu) atomicMin(&kmin[i], lmin[i]);
        if (lmax[i] != 0u) atomicMax(&kmax[i], lmax[i]);
    }
}

// one workgroup: box rows of both meshes (get_instance_bboxes, prepare_scannet.py:120-135) indexed by objectId, the instance GT
// code of every object (prepare_scannet_inst_gt.py:53-62), then the ordered compaction that drops rows labelled 1, 2 or 22 when
// there is more than one row (process_one_scan :185-191); flags[1] = rows kept
#define SX_ROWS_BLOCK 1024
__global__ __launch_bounds__(SX_ROWS_BLOCK) void sx_rows_kernel(const unsigned short *__restrict__ raw, const int *__restrict__ seg_first,
                                                                int S, const int *__restrict__ obj_id,
                                                                const int *__restrict__ obj_label_seg, int K, int R,
                                                                const int *__restrict__ kfirst, const unsigned *__restrict__ kmin,
                                                                const unsigned *__restrict__ kmax, double *__restrict__ rows,
                                                                int *__restrict__ row_claim, int *__restrict__ code, double *__restrict__ boxes,
                                                                double *__restrict__ aligned_boxes, int *__restrict__ flags) {
    __shared__ int cnt[SX_ROWS_BLOCK];
    const int t = threadIdx.x;
    double *rows_a = rows + (size_t)R * 8;
    for (int i = t; i < R * 8; i += SX_ROWS_BLOCK) {
        rows[i] = 0.0;
        rows_a[i] = 0.0;
    }
    __syncthreads();
    for (int k = t; k < K; k += SX_ROWS_BLOCK) {
        int first = kfirst[k], o = obj_id[k];
        code[k] = 0;
        // a row is written by the one object that claims it; an id outside [0, R) or claimed twice is a broken table
        if (o < 0 || o >= R || atomicCAS(&row_claim[o], -1, k) != -1) {
            atomicOr(flags, SX_BAD_TABLE);
            continue;
        }
        if (first == SX_SENT) continue;
        int ls = obj_label_seg[k];
        int lv = (ls >= 0 && ls < S) ? seg_first[ls] : SX_SENT;
        int label = lv == SX_SENT ? 0 : (int)raw[lv];
        int fr = raw[first];
        code[k] = sx_nyu40(fr < SX_NLABEL ? sx_remap(fr) : -1) * 1000 + o + 1;
        for (int mset = 0; mset < 2; mset++) {
            double *row = (mset ? rows_a : rows) + (size_t)o * 8;
            for (int j = 0; j < 3; j++) {
                float mn = sx_unkey(kmin[6 * k + 3 * mset + j]), mx = sx_unkey(kmax[6 * k + 3 * mset + j]);
                row[j] = (double)((mn + mx) / 2.0f);
                row[3 + j] = (double)(mx - mn);
            }
            row[6] = (double)label;
            row[7] = (double)o;
        }
    }
    __syncthreads();
    const int per = (R + SX_ROWS_BLOCK - 1) / SX_ROWS_BLOCK;
    const int r0 = t * per, r1 = min(R, r0 + per);
    auto keep = [&](int r) {
        if (R <= 1) return true;
        double l = rows[(size_t)r * 8 + 6];
        return !(l == 1.0 || l == 2.0 || l == 22.0);
    };
    int n = 0;
    for (int r = r0; r < r1; r++) n += keep(r) ? 1 : 0;
    cnt[t] = n;
    __syncthreads();
    for (int off = 1; off < SX_ROWS_BLOCK; off <<= 1) {  // inclusive Hillis-Steele scan
        int add = t >= off ? cnt[t - off] : 0;
        __syncthreads();
        cnt[t] += add;
        __syncthreads();
    }
    int pos = cnt[t] - n;
    for (int r = r0; r < r1; r++) {
        if (!keep(r)) continue;
        for (int j = 0; j < 8; j++) {
            boxes[(size_t)pos * 8 + j] = rows[(size_t)r * 8 + j];
            aligned_boxes[(size_t)pos * 8 + j] = rows_a[(size_t)r * 8 + j];
        }
        pos++;
    }
    if (t == SX_ROWS_BLOCK - 1) flags[1] = cnt[t];
}

// instance GT: (sem + 1) * 1000 outside instances, the object's code inside (prepare_scannet_inst_gt.py:48-62)
__global__ __launch_bounds__(SX_BLOCK) void sx_inst_gt_kernel(const unsigned short *__restrict__ raw, const int *__restrict__ seg, int N,
                                                              int S, const int *__restrict__ seg_owner, const int *__restrict__ code,
                                                              int *__restrict__ inst_gt) {
    int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= N) return;
    int o = sx_owner(seg, seg_owner, S, v);
    int r = raw[v];
    inst_gt[v] = o >= 0 ? code[o] : ((r < SX_NLABEL ? sx_remap(r) : -1) + 1) * 1000;
}

static bool sx_label_sizes_ok(int N, int S, int P, int K, int R) {
    return N >= 1 && N <= SX_MAX_VERTICES && S >= 1 && S <= SX_MAX_SEGMENTS && P >= 0 && P <= SX_MAX_PAIRS && K >= 1 &&
           K <= SX_MAX_OBJECTS && R >= 1 && R <= SX_MAX_ROWS;
}

struct SxLabelWs { int *seg_first, *seg_owner, *kfirst, *code, *row_claim; unsigned *kmin, *kmax; double *rows; };
static void sx_label_layout(D3Carver &c, int S, int K, int R, SxLabelWs &w) {
    w.seg_first = c.take<int>(S); w.seg_owner = c.take<int>(S);
    w.kfirst = c.take<int>(K); w.code = c.take<int>(K);
    w.kmin = c.take<unsigned>((size_t)6 * K); w.kmax = c.take<unsigned>((size_t)6 * K);
    w.rows = c.take<double>((size_t)16 * R);
    w.row_claim = c.take<int>(R);
}

size_t d3_scan_labels_ws_bytes(int N, int S, int P, int K, int R) {
    if (!sx_label_sizes_ok(N, S, P, K, R)) return 0;
    D3Carver c(nullptr, 0);
    SxLabelWs w;
    sx_label_layout(c, S, K, R, w);
    return c.off;
}

int d3_scan_labels(const unsigned short *raw, const int *seg, int N, int S, const int *pair_seg, const int *pair_obj, int P,
                   const int *obj_id, const int *obj_label_seg, int K, int R, const float *mesh, const float *aligned_mesh,
                   double *instance_ids, double *sem_labels, int *inst_gt, double *boxes, double *aligned_boxes, int *flags, void *ws,
                   size_t ws_bytes, void *stream) {
    if (!sx_label_sizes_ok(N, S, P, K, R)) return D3_ERR_RANGE;
    if (!raw || !seg || (P > 0 && (!pair_seg || !pair_obj)) || !obj_id || !obj_label_seg || !mesh || !aligned_mesh ||
        !instance_ids || !sem_labels || !inst_gt || !boxes || !aligned_boxes || !flags || !ws)
        return D3_ERR_ARG;
    D3Carver cv(ws, ws_bytes);
    SxLabelWs w;
    sx_label_layout(cv, S, K, R, w);
    if (!cv.ok()) return D3_ERR_WORKSPACE;
    int *seg_first = w.seg_first, *seg_owner = w.seg_owner, *kfirst = w.kfirst, *code = w.code, *row_claim = w.row_claim;
    unsigned *kmin = w.kmin, *kmax = w.kmax;
    double *rows = w.rows;
    hipStream_t st = d3_stream(stream);
    D3_CLEAR();
    D3_CHECK(hipMemsetAsync(seg_first, 0x7f, (size_t)S * 4, st));
    D3_CHECK(hipMemsetAsync(seg_owner, 0xff, (size_t)S * 4, st));
    D3_CHECK(hipMemsetAsync(kfirst, 0x7f, (size_t)K * 4, st));
    D3_CHECK(hipMemsetAsync(kmin, 0xff, (size_t)6 * K * 4, st));
    D3_CHECK(hipMemsetAsync(kmax, 0x00, (size_t)6 * K * 4, st));
    D3_CHECK(hipMemsetAsync(row_claim, 0xff, (size_t)R * 4, st));
    const int gv = sx_blocks(N, SX_BLOCK);
    hipLaunchKernelGGL(sx_seg_first_kernel, dim3(gv), dim3(SX_BLOCK), 0, st, raw, seg, N, S, seg_first, flags);
    if (P > 0)
        hipLaunchKernelGGL(sx_pair_kernel, dim3(sx_blocks(P, SX_BLOCK)), dim3(SX_BLOCK), 0, st, pair_seg, pair_obj, P, S, K, seg_first,
                           seg_owner, flags);
    // 4 vertices per thread: the LDS table's set-up and flush are paid once per 1024 vertices
    const int gb = sx_blocks(N, 4 * SX_BLOCK);
    hipLaunchKernelGGL(sx_vertex_kernel, dim3(gb), dim3(SX_BLOCK), (size_t)13 * K * 4, st, raw, seg, N, S, seg_owner, obj_id, K, mesh,
                       aligned_mesh, instance_ids, sem_labels, kfirst, kmin, kmax);
    hipLaunchKernelGGL(sx_rows_kernel, dim3(1), dim3(SX_ROWS_BLOCK), 0, st, raw, seg_first, S, obj_id, obj_label_seg, K, R, kfirst,
                       kmin, kmax, rows, row_claim, code, boxes, aligned_boxes, flags);
    hipLaunchKernelGGL(sx_inst_gt_kernel, dim3(gv), dim3(SX_BLOCK), 0, st, raw, seg, N, S, seg_owner, code, inst_gt);
    D3_LAUNCH_CHECK();
    return 0;
}
