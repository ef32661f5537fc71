// multiview.hip -- projection of per-frame 2D feature maps onto a scene's mesh vertices (reference: lib/utils/projection.py:180-256
// ProjectionHelper.compute_projection / project, data/scannet/project_multiview_features.py:88-205), driven by d3net_amd/multiview.py.
//
// Per frame f and point p the mapping is the reference's chain: frustum test (six planes, `round(dot * 100) / 100 < 0`), projection
// through world_to_camera (computed by the caller on the host, torch.inverse), rint to a pixel inside the image, depth test against
// the frame's depth map.  Every step is explicit float32 in a fixed operation order (the library builds with -ffp-contract=off), so
// tests/multiview_restate.py restates it bit for bit.
//
// Two consumers of the mapping:
//   * d3_multiview_project: the reference's per-frame (indices_3d, indices_2d) lists for F frames at once, a stable compaction in
//     ascending point order through one rocPRIM scan over the F x N flags;
//   * d3_multiview_fuse: the fused path -- per-frame valid counts, a CHW -> HWC transpose of the features so that a mapped point
//     gathers one contiguous 512-B row, then a point-stationary pass that walks the frames in order with the running rows in
//     registers.  Gathers and max are exact and nothing is accumulated in floating point, so the output is bit-determined by the
//     mapping (no float atomics; the only atomics are integer counts).
#include "common.h"

#define MV_C 128                 // the reference's emptiness test hard-codes 128 channels
#define MV_MAX_POINTS (1 << 24)
#define MV_MAX_FRAMES 16384
#define MV_MAX_PIXELS 65536
#define MV_NPAR 36               // per frame: world_to_camera rows 0-2 (12), six normals (18), corners 2 and 4 (6)
#define MV_BLOCK 256
#define MV_TILE_P 64             // fuse: points per workgroup
#define MV_TILE_F 4              // fuse: frames mapped per LDS phase (one wave per frame)

int d3_multiview_limits(int *max_points, int *max_frames, int *max_pixels) {
    if (max_points) *max_points = MV_MAX_POINTS;
    if (max_frames) *max_frames = MV_MAX_FRAMES;
    if (max_pixels) *max_pixels = MV_MAX_PIXELS;
    return 0;
}

// camera constants of a ProjectionHelper: float32 intrinsics / limits and the 8 unprojected image corners (camera space)
struct MvCam {
    float fx, fy, cx, cy, dmin, dmax, acc;
    int W, H;
    float cp[8][3];
};

static int mv_cam(const double *intr_host, int W, int H, MvCam *cam) {
    if (!intr_host) return D3_ERR_ARG;
    double fx = intr_host[0], fy = intr_host[1], cx = intr_host[2], cy = intr_host[3];
    double dmin = intr_host[4], dmax = intr_host[5];
    cam->fx = (float)fx; cam->fy = (float)fy; cam->cx = (float)cx; cam->cy = (float)cy;
    cam->dmin = (float)dmin; cam->dmax = (float)dmax; cam->acc = (float)intr_host[6];
    cam->W = W; cam->H = H;
    // depth_to_skeleton (projection.py:18-22) in double, stored as float32 like its torch.Tensor([...]); corner order of :28-45
    const double ux[4] = {0.0, (double)(W - 1), (double)(W - 1), 0.0}, uy[4] = {0.0, 0.0, (double)(H - 1), (double)(H - 1)};
    for (int k = 0; k < 8; k++) {
        double d = k < 4 ? dmin : dmax;
        double x = (ux[k & 3] - cx) / fx, y = (uy[k & 3] - cy) / fy;
        cam->cp[k][0] = (float)(d * x); cam->cp[k][1] = (float)(d * y); cam->cp[k][2] = (float)d;
    }
    return 0;
}

static inline int mv_blocks(long long n, int per) {
    long long g = (n + per - 1) / per;
    return (int)(g < 1 ? 1 : g);
}

// ---- per-frame parameters (projection.py:50-130: frustum corners, inward normals) ------------------------------------------------
__device__ __forceinline__ void mv_cross(const float *a, const float *b, float *o) {
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}

__global__ void mv_params_kernel(const float *__restrict__ c2w, const float *__restrict__ w2c, int F, MvCam cam,
                                 float *__restrict__ par) {
    int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F) return;
    const float *M = c2w + 16 * (size_t)f;
    float cc[8][3];
    for (int k = 0; k < 8; k++)
        for (int r = 0; r < 3; r++) {
            float v = M[4 * r] * cam.cp[k][0] + M[4 * r + 1] * cam.cp[k][1];
            v = v + M[4 * r + 2] * cam.cp[k][2];
            cc[k][r] = v + M[4 * r + 3];
        }
    // plane k: cross(corner[A] - corner[B], corner[C] - corner[B])
    const int A[6] = {3, 2, 3, 0, 1, 6}, B[6] = {0, 1, 2, 3, 0, 5}, Cc[6] = {1, 5, 6, 7, 4, 4};
    float *P = par + MV_NPAR * (size_t)f;
    for (int i = 0; i < 12; i++) P[i] = w2c[16 * (size_t)f + i];
    for (int k = 0; k < 6; k++) {
        float a[3], b[3], n[3];
        for (int r = 0; r < 3; r++) {
            a[r] = cc[A[k]][r] - cc[B[k]][r];
            b[r] = cc[Cc[k]][r] - cc[B[k]][r];
        }
        mv_cross(a, b, n);
        for (int r = 0; r < 3; r++) P[12 + 3 * k + r] = n[r];
    }
    for (int r = 0; r < 3; r++) {
        P[30 + r] = cc[2][r];
        P[33 + r] = cc[4][r];
    }
}

// ---- the mapping of one (frame, point): pixel index v * W + u, or -1 (projection.py:133-160 points_in_frustum, :195-238) -------
// P: the frame's MV_NPAR parameters, depth: its H x W map.  NaN parameters (a -inf pose) fail every comparison.
__device__ __forceinline__ int mv_pixel(const float *__restrict__ P, const float *__restrict__ depth, const MvCam &cam, float x, float y,
                                        float z) {
    float a0 = x - P[30], a1 = y - P[31], a2 = z - P[32];
    float b0 = x - P[33], b1 = y - P[34], b2 = z - P[35];
#pragma unroll
    for (int k = 0; k < 6; k++) {
        float d0 = k < 3 ? a0 : b0, d1 = k < 3 ? a1 : b1, d2 = k < 3 ? a2 : b2;
        float dot = d0 * P[12 + 3 * k] + d1 * P[13 + 3 * k];
        dot = dot + d2 * P[14 + 3 * k];
        // round(dot * 100) / 100 < 0 with round half to even  <=>  dot * 100 < -0.5
        if (!(dot * 100.0f < -0.5f)) return -1;
    }
    float c[3];
#pragma unroll
    for (int r = 0; r < 3; r++) {
        float v = P[4 * r] * x + P[4 * r + 1] * y;
        v = v + P[4 * r + 2] * z;
        c[r] = v + P[4 * r + 3];
    }
    float u = rintf((c[0] * cam.fx) / c[2] + cam.cx);
    float v = rintf((c[1] * cam.fy) / c[2] + cam.cy);
    if (!(u >= 0.0f && u < (float)cam.W && v >= 0.0f && v < (float)cam.H)) return -1;
    int pix = (int)v * cam.W + (int)u;
    float d = depth[pix];
    if (!(d >= cam.dmin && d <= cam.dmax && fabsf(d - c[2]) <= cam.acc)) return -1;
    return pix;
}

// ---- per-frame mapped-point counts: grid (x: point chunks, y: frame), one integer atomic per workgroup ----------------------------
__global__ __launch_bounds__(MV_BLOCK) void mv_count_kernel(const float *__restrict__ pts, int N, const float *__restrict__ depths,
                                                             const float *__restrict__ par, MvCam cam, int *__restrict__ counts) {
    __shared__ int part[MV_BLOCK / D3_WAVE];
    int f = blockIdx.y;
    const float *P = par + MV_NPAR * (size_t)f;
    const float *dep = depths + (size_t)f * cam.W * cam.H;
    int c = 0;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < N; i += gridDim.x * blockDim.x)
        c += mv_pixel(P, dep, cam, pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]) >= 0;
    for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off);
    if (d3_lane() == 0) part[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        int s = 0;
        for (int w = 0; w < MV_BLOCK / D3_WAVE; w++) s += part[w];
        if (s) atomicAdd(&counts[f], s);
    }
}

static inline int mv_count_grid(int N) {
    int g = mv_blocks(N, MV_BLOCK * 16);
    return g > 256 ? 256 : g;
}

// ---- d3_multiview_project: (F, N+1) index lists --------------------------------------------------------------------------------
__global__ __launch_bounds__(MV_BLOCK) void mv_map_kernel(const float *__restrict__ pts, int N, const float *__restrict__ depths,
                                                           const float *__restrict__ par, MvCam cam, int *__restrict__ pix,
                                                           int *__restrict__ flag) {
    int f = blockIdx.y;
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    int q = mv_pixel(par + MV_NPAR * (size_t)f, depths + (size_t)f * cam.W * cam.H, cam, pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]);
    size_t o = (size_t)f * N + i;
    pix[o] = q;
    flag[o] = q >= 0;
}

__global__ __launch_bounds__(MV_BLOCK) void mv_scatter_kernel(int N, const int *__restrict__ pix, const int *__restrict__ pos,
                                                               long long *__restrict__ i3d, long long *__restrict__ i2d) {
    int f = blockIdx.y;
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    size_t o = (size_t)f * N + i;
    int q = pix[o];
    int base = pos[(size_t)f * N];
    long long *r3 = i3d + (size_t)f * (N + 1), *r2 = i2d + (size_t)f * (N + 1);
    if (q >= 0) {
        int j = pos[o] - base;
        r3[1 + j] = i;
        r2[1 + j] = q;
    }
    if (i == N - 1) {
        long long cnt = (long long)(pos[o] - base) + (q >= 0);
        r3[0] = cnt;
        r2[0] = cnt;
    }
}

struct MvProjWs { float *par; int *pix, *flag, *pos; void *temp; size_t temp_bytes; };
static void mv_project_layout(D3Carver &c, int N, int F, MvProjWs &w) {
    const size_t nf = (size_t)N * F;
    w.par = c.take<float>((size_t)F * MV_NPAR);
    w.pix = c.take<int>(nf); w.flag = c.take<int>(nf); w.pos = c.take<int>(nf);
    w.temp_bytes = d3_scan_temp_bytes((int)nf);
    w.temp = c.take<char>(w.temp_bytes);
}

size_t d3_multiview_project_ws_bytes(int N, int F) {
    if (N < 1 || N > MV_MAX_POINTS || F < 1 || F > MV_MAX_FRAMES || (long long)N * F > 0x7fffffffll) return 0;
    D3Carver c(nullptr, 0);
    MvProjWs w;
    mv_project_layout(c, N, F, w);
    return c.off;
}

static int mv_check_sizes(int N, int F, int W, int H) {
    if (N < 0 || N > MV_MAX_POINTS || F < 0 || F > MV_MAX_FRAMES) return D3_ERR_RANGE;
    if (W < 1 || H < 1 || (long long)W * H > MV_MAX_PIXELS) return D3_ERR_RANGE;
    return 0;
}

int d3_multiview_project(const float *points, int N, const float *depths, const float *c2w, const float *w2c, int F,
                         const double *intr_host, int W, int H, long long *idx3d, long long *idx2d, void *ws, size_t ws_bytes,
                         void *stream) {
    D3_CLEAR();
    int rc = mv_check_sizes(N, F, W, H);
    if (rc) return rc;
    if ((long long)N * F > 0x7fffffffll) return D3_ERR_RANGE;
    MvCam cam;
    rc = mv_cam(intr_host, W, H, &cam);
    if (rc) return rc;
    if (N == 0 || F == 0) return 0;
    D3Carver cv(ws, ws_bytes);
    MvProjWs w;
    mv_project_layout(cv, N, F, w);
    if (!cv.ok()) return D3_ERR_WORKSPACE;
    const size_t nf = (size_t)N * F;
    float *par = w.par;
    int *pix = w.pix, *flag = w.flag, *pos = w.pos;
    hipStream_t st = d3_stream(stream);
    D3_CHECK(hipMemsetAsync(idx3d, 0, (size_t)F * (N + 1) * sizeof(long long), st));
    D3_CHECK(hipMemsetAsync(idx2d, 0, (size_t)F * (N + 1) * sizeof(long long), st));
    hipLaunchKernelGGL(mv_params_kernel, dim3(mv_blocks(F, 64)), dim3(64), 0, st, c2w, w2c, F, cam, par);
    D3_LAUNCH_CHECK();
    dim3 g(mv_blocks(N, MV_BLOCK), F);
    hipLaunchKernelGGL(mv_map_kernel, g, dim3(MV_BLOCK), 0, st, points, N, depths, par, cam, pix, flag);
    D3_LAUNCH_CHECK();
    rc = d3_exclusive_scan_i32(flag, pos, (int)nf, w.temp, w.temp_bytes, st);
    if (rc) return rc;
    hipLaunchKernelGGL(mv_scatter_kernel, g, dim3(MV_BLOCK), 0, st, N, pix, pos, idx3d, idx2d);
    D3_LAUNCH_CHECK();
    return 0;
}

// ---- ProjectionHelper.project (projection.py:240-256) for one frame: out (C, N) = 0, out[:, i3d[1+j]] = label[:, i2d[1+j]] -----
// The count is read from i3d[0] on the device (no host sync); entries outside [0, N) / [0, HW) are skipped.
__global__ __launch_bounds__(MV_BLOCK) void mv_project_frame_kernel(const float *__restrict__ label, int C, int HW,
                                                                     const long long *__restrict__ i3d, const long long *__restrict__ i2d,
                                                                     int N, float *__restrict__ out) {
    long long cnt = i3d[0];
    int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= N || (long long)j >= cnt) return;
    long long p = i3d[1 + j], q = i2d[1 + j];
    if (p < 0 || p >= N || q < 0 || q >= HW) return;
    for (int c = blockIdx.y; c < C; c += gridDim.y) out[(size_t)c * N + p] = label[(size_t)c * HW + q];
}

int d3_multiview_project_frame(const float *label, int C, int HW, const long long *idx3d, const long long *idx2d, int N, float *out,
                               void *stream) {
    D3_CLEAR();
    if (C < 1 || C > 65535 || HW < 1 || HW > MV_MAX_PIXELS || N < 0 || N > MV_MAX_POINTS) return D3_ERR_RANGE;
    if (N == 0) return 0;
    hipStream_t st = d3_stream(stream);
    D3_CHECK(hipMemsetAsync(out, 0, (size_t)C * N * sizeof(float), st));
    int gy = C < 128 ? C : 128;
    hipLaunchKernelGGL(mv_project_frame_kernel, dim3(mv_blocks(N, MV_BLOCK), gy), dim3(MV_BLOCK), 0, st, label, C, HW, idx3d, idx2d, N,
                       out);
    D3_LAUNCH_CHECK();
    return 0;
}

// ---- d3_multiview_fuse ---------------------------------------------------------------------------------------------------------
// CHW -> HWC per frame: a workgroup moves 32 pixels x 128 channels through a padded LDS tile
__global__ __launch_bounds__(MV_BLOCK) void mv_transpose_kernel(const float *__restrict__ in, int HW, float *__restrict__ out) {
    __shared__ float tile[MV_C][33];
    int f = blockIdx.y, px0 = blockIdx.x * 32, t = threadIdx.x;
    const float *src = in + (size_t)f * MV_C * HW;
    float *dst = out + (size_t)f * HW * MV_C;
    for (int i = 0; i < MV_C / 8; i++) {
        int c = (t >> 5) + 8 * i, px = px0 + (t & 31);
        tile[c][t & 31] = px < HW ? src[(size_t)c * HW + px] : 0.0f;
    }
    __syncthreads();
    for (int i = 0; i < MV_C / 8; i++) {
        int idx = t + MV_BLOCK * i, px = idx >> 7, c = idx & (MV_C - 1);
        if (px0 + px < HW) dst[(size_t)(px0 + px) * MV_C + c] = tile[c][px];
    }
}

__device__ __forceinline__ bool mv_nz(float4 a) { return a.x != 0.0f || a.y != 0.0f || a.z != 0.0f || a.w != 0.0f; }
// torch.max(a, b) element-wise: NaN propagates
__device__ __forceinline__ float mv_max(float a, float b) { return (a > b || a != a) ? a : b; }
// this half-wave's 32 bits of a ballot (a point's row is spread over 32 lanes x float4)
__device__ __forceinline__ unsigned mv_half(unsigned long long m) { return (unsigned)(m >> (threadIdx.x & 32)); }

// Workgroup = 64 points.  Phase 1: wave w maps the workgroup's points for frame f0 + w (one lane per point) into LDS.  Phase 2:
// half-wave h owns points h, h + 8, ..., h + 56, 32 lanes x float4 of each row, and applies the frames in order
// (project_multiview_features.py:170-200):
//   maxpool: proj non-empty -> row = proj if the row is empty, else max(row, proj);
//   else   : row empty -> row = proj (zero for an unmapped point).
// Frames with no mapped point anywhere (counts[f] == 0) are skipped, as the reference drops them.
__global__ __launch_bounds__(MV_BLOCK) void mv_fuse_kernel(const float *__restrict__ pts, int N, const float *__restrict__ depths,
                                                            const float *__restrict__ par, const int *__restrict__ counts, int F,
                                                            MvCam cam, const float *__restrict__ feat, int maxpool,
                                                            float *__restrict__ out) {
    __shared__ int spix[MV_TILE_F][MV_TILE_P];
    const int t = threadIdx.x, base = blockIdx.x * MV_TILE_P;
    const int HW = cam.W * cam.H;
    const int mp = base + (t & (MV_TILE_P - 1));
    float x = 0.0f, y = 0.0f, z = 0.0f;
    if (mp < N) { x = pts[3 * mp]; y = pts[3 * mp + 1]; z = pts[3 * mp + 2]; }
    const int h = t >> 5, l4 = t & 31;
    float4 r[8];
    bool empty[8];
#pragma unroll
    for (int k = 0; k < 8; k++) { r[k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f); empty[k] = true; }

    for (int f0 = 0; f0 < F; f0 += MV_TILE_F) {
        {
            int f = __builtin_amdgcn_readfirstlane(f0 + (t >> 6));
            int q = -1;
            if (f < F && counts[f] > 0 && mp < N) q = mv_pixel(par + MV_NPAR * (size_t)f, depths + (size_t)f * HW, cam, x, y, z);
            spix[t >> 6][t & (MV_TILE_P - 1)] = q;
        }
        __syncthreads();
        const int nf = F - f0 < MV_TILE_F ? F - f0 : MV_TILE_F;
        for (int j = 0; j < nf; j++) {
            const int f = f0 + j;
            if (counts[f] == 0) continue;
            const float4 *fr = (const float4 *)(feat + (size_t)f * HW * MV_C) + l4;
            int q[8];
            float4 p[8];
#pragma unroll
            for (int k = 0; k < 8; k++) {
                q[k] = spix[j][h + 8 * k];
                p[k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (q[k] >= 0 && (maxpool || empty[k])) p[k] = fr[(size_t)q[k] * (MV_C / 4)];
            }
#pragma unroll
            for (int k = 0; k < 8; k++) {
                if (q[k] >= 0) {
                    if (maxpool) {
                        if (mv_half(__ballot(mv_nz(p[k])))) {
                            if (empty[k]) {
                                r[k] = p[k];
                                empty[k] = false;
                            } else {
                                r[k].x = mv_max(r[k].x, p[k].x); r[k].y = mv_max(r[k].y, p[k].y);
                                r[k].z = mv_max(r[k].z, p[k].z); r[k].w = mv_max(r[k].w, p[k].w);
                                empty[k] = mv_half(__ballot(mv_nz(r[k]))) == 0;
                            }
                        }
                    } else if (empty[k]) {
                        r[k] = p[k];
                        empty[k] = mv_half(__ballot(mv_nz(p[k]))) == 0;
                    }
                } else if (!maxpool && empty[k]) {
                    r[k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                }
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < 8; k++) {
        int pt = base + h + 8 * k;
        if (pt < N) ((float4 *)(out + (size_t)pt * MV_C))[l4] = r[k];
    }
}

struct MvFuseWs { float *par; int *counts; float *hwc; };
static void mv_fuse_layout(D3Carver &c, int F, int W, int H, MvFuseWs &w) {
    w.par = c.take<float>((size_t)F * MV_NPAR);
    w.counts = c.take<int>(F);
    w.hwc = c.take<float>((size_t)F * W * H * MV_C);
}

size_t d3_multiview_fuse_ws_bytes(int F, int W, int H) {
    if (F < 1 || F > MV_MAX_FRAMES || W < 1 || H < 1 || (long long)W * H > MV_MAX_PIXELS) return 0;
    D3Carver c(nullptr, 0);
    MvFuseWs w;
    mv_fuse_layout(c, F, W, H, w);
    return c.off;
}

int d3_multiview_fuse(const float *points, int N, const float *depths, const float *c2w, const float *w2c, int F,
                      const double *intr_host, int W, int H, const float *feats, int C, int maxpool, float *out, int *frame_counts,
                      void *ws, size_t ws_bytes, void *stream) {
    D3_CLEAR();
    if (C != MV_C) return D3_ERR_ARG;
    int rc = mv_check_sizes(N, F, W, H);
    if (rc) return rc;
    MvCam cam;
    rc = mv_cam(intr_host, W, H, &cam);
    if (rc) return rc;
    if (N == 0) return 0;
    hipStream_t st = d3_stream(stream);
    if (F == 0) {
        D3_CHECK(hipMemsetAsync(out, 0, (size_t)N * MV_C * sizeof(float), st));
        return 0;
    }
    D3Carver cv(ws, ws_bytes);
    MvFuseWs w;
    mv_fuse_layout(cv, F, W, H, w);
    if (!cv.ok()) return D3_ERR_WORKSPACE;
    float *par = w.par;
    int *counts = w.counts;
    float *hwc = w.hwc;
    const int HW = W * H;
    D3_CHECK(hipMemsetAsync(counts, 0, (size_t)F * sizeof(int), st));
    hipLaunchKernelGGL(mv_params_kernel, dim3(mv_blocks(F, 64)), dim3(64), 0, st, c2w, w2c, F, cam, par);
    D3_LAUNCH_CHECK();
    hipLaunchKernelGGL(mv_count_kernel, dim3(mv_count_grid(N), F), dim3(MV_BLOCK), 0, st, points, N, depths, par, cam, counts);
    D3_LAUNCH_CHECK();
    hipLaunchKernelGGL(mv_transpose_kernel, dim3(mv_blocks(HW, 32), F), dim3(MV_BLOCK), 0, st, feats, HW, hwc);
    D3_LAUNCH_CHECK();
    hipLaunchKernelGGL(mv_fuse_kernel, dim3(mv_blocks(N, MV_TILE_P)), dim3(MV_BLOCK), 0, st, points, N, depths, par, counts, F, cam, hwc,
                       maxpool ? 1 : 0, out);
    D3_LAUNCH_CHECK();
    if (frame_counts) D3_CHECK(hipMemcpyAsync(frame_counts, counts, (size_t)F * sizeof(int), hipMemcpyDeviceToDevice, st));
    return 0;
}
