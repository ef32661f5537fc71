// batch_prep.hip -- a whole training batch straight from the resident scene store (d3net_amd/dataset.py:SceneStore), on the paths
// that run neither elastic distortion nor crop: what scene_prep.hip computes scene by scene (transform, offset, emit, instance
// statistics, box labels, GT proposal lists) and collate.hip then stacks, written ONCE into the batch tensors, bit for bit.
// Driven by d3net_amd/scene_prep.py:prepare_batch_store.
//
// Without a crop a scene keeps all its points, so everything that depends only on its instance_ids / sem_labels -- the id range,
// the hist / rank / start tables, the stably sorted per-instance point lists, K, Lp -- is static and comes from the store's
// instance index (SceneStore.instance_index).  Only the coordinates change from batch to batch.  So there is no read-back, no scan
// and no sort here: one table copy and three launches whatever the batch size.  Each launch is a flat grid over all slots; a block
// finds its (slot, tile) by binary search of a tile-prefix table it first loads into LDS, as collate.hip does.
//
// y = xyz @ M and s = y * scale are recomputed from the store's float32 xyz wherever they are used (the same expressions in the
// same order as sp_transform_kernel; -ffp-contract=off), never stored: 12 bytes read per use instead of 48 written and read.
// Every reduction is deterministic: the per-slot minimum by integer atomics on the order-preserving encoding, the per-instance
// sums sequential over ascending point index.  Every output element has exactly one writer.
//
// The second half of the file is the label-free batch of the test split (d3_store_extents, d3_points_batch; driven by
// scene_prep.py:prepare_points_store), which shares bp_find and bp_transform (scene_prep.h, with the box-label rows).  pb_points_kernel REPEATS stage 1's feature-row
// copy line for line instead of sharing a helper: moving the copy into a function changed stage 1's generated code, and that
// kernel's measured time is on record.  Keep the two copies in step.
#include "scene_prep.h"

#define BP_BLOCK 256
#define BP_PTILE 1024                 // points (or proposal entries) per block: 4 per thread
#define BP_WTILE 4096                 // feature words per block: four 16-byte accesses per thread
#define BP_MAX_B 512                  // slots per batch: a prefix table of 2 * B + 1 ints in LDS
#define BP_NOUT 20

struct BpSlot {
    long long row0;                   // first store row
    int n, voff, V, K, Lp, has_unl;   // points, index-table offset, id values, instances, labelled points, any unlabelled point
    int P, I, Q, vbase;               // points / instances / proposal entries / id values of the slots before
    double m[9];
};

struct BpArgs {
    const float *xyz, *feats;
    const int *sem, *ids, *hist, *rank, *start, *sorted;
    const double *mean_size;
    const BpSlot *slots;
    u64 *smin;                        // (B,3) encoded minima of s, preset to ~0 by the table copy
    const int *prefix;                // this stage's tile prefix: 2 jobs per slot, 2 * B + 1 entries
    double *istats;                   // 9 per (slot, id value): mean, min, max
    int B, C, R, fp32, has_gt;
    double scale; float scale_f;
    BpOut o;
};

// ---- stage 1: the per-slot minimum of s (job 2 * slot) and the feature rows, store -> batch (job 2 * slot + 1) ---------------------
__global__ void __launch_bounds__(BP_BLOCK) bp_stage1_kernel(BpArgs a) {
    extern __shared__ int s_prefix[];
    __shared__ u64 s_min[BP_BLOCK / 64][3];
    const int t = (int)threadIdx.x;
    const int j = bp_find(s_prefix, a.prefix, 2 * a.B);
    const int slot = j >> 1, tile = (int)blockIdx.x - s_prefix[j];
    const BpSlot *__restrict__ sl = a.slots + slot;
    const int n = sl->n;
    const long long row0 = sl->row0;

    if (j & 1) {
        const long long count = (long long)n * a.C, base = (long long)tile * BP_WTILE;
        const unsigned *__restrict__ src = (const unsigned *)a.feats + row0 * a.C;
        unsigned *__restrict__ dst = (unsigned *)a.o.feats + (long long)sl->P * a.C;
        if ((((size_t)src | (size_t)dst) & 15) == 0) {            // 16-byte accesses, the four loads in flight together
            const uint4 *__restrict__ s4 = (const uint4 *)(src + base) + t;
            uint4 *__restrict__ d4 = (uint4 *)(dst + base) + t;
            if (base + BP_WTILE <= count) {
                uint4 v0 = s4[0], v1 = s4[BP_BLOCK], v2 = s4[2 * BP_BLOCK], v3 = s4[3 * BP_BLOCK];
                d4[0] = v0; d4[BP_BLOCK] = v1; d4[2 * BP_BLOCK] = v2; d4[3 * BP_BLOCK] = v3;
            } else {                                              // the slot's last tile
                for (int k = 0; k < BP_WTILE / (4 * BP_BLOCK); ++k) {
                    const long long w = base + 4ll * (k * BP_BLOCK + t);
                    if (w + 4 <= count) d4[k * BP_BLOCK] = s4[k * BP_BLOCK];
                    else
                        for (long long u = w; u < count; ++u) dst[u] = src[u];   // at most 3 words, in one thread
                }
            }
        } else {                                                  // lane-consecutive words
            for (int k = 0; k < BP_WTILE / BP_BLOCK; ++k) {
                long long w = base + t + k * BP_BLOCK;
                if (w < count) dst[w] = src[w];
            }
        }
        return;
    }

    double m[9];
    for (int k = 0; k < 9; k++) m[k] = a.fp32 ? 0.0 : sl->m[k];
    const float *__restrict__ x = a.xyz + 3 * row0;
    u64 mn[3] = {~0ull, ~0ull, ~0ull};
    for (int k = 0; k < BP_PTILE / BP_BLOCK; ++k) {
        int i = tile * BP_PTILE + t + k * BP_BLOCK;
        if (i < n) {
            double y[3], s[3];
            bp_transform(x[3 * (size_t)i], x[3 * (size_t)i + 1], x[3 * (size_t)i + 2], m, a.fp32, a.scale, a.scale_f, y, s);
            for (int d = 0; d < 3; d++) {
                u64 e = sp_enc(s[d]);
                mn[d] = e < mn[d] ? e : mn[d];
            }
        }
    }
    for (int off = 32; off > 0; off >>= 1)
        for (int d = 0; d < 3; d++) {
            u64 b = __shfl_xor(mn[d], off);
            mn[d] = b < mn[d] ? b : mn[d];
        }
    if (d3_lane() == 0)
        for (int d = 0; d < 3; d++) s_min[t >> 6][d] = mn[d];
    __syncthreads();
    if (t < 3) {
        u64 v = s_min[0][t];
        for (int w = 1; w < BP_BLOCK / 64; w++) v = s_min[w][t] < v ? s_min[w][t] : v;
        atomicMin(&a.smin[3 * slot + t], v);
    }
}

// ---- stage 2: one wave per (slot, id value) (job 2 * slot); the rows of the box labels no instance owns and the offset tables
// (job 2 * slot + 1, 64 rows per block).  sp_instance_kernel's arithmetic, order of summation and box-slot rule. ---------------------
template <typename T>
__global__ void __launch_bounds__(64) bp_stage2_kernel(BpArgs a) {
    extern __shared__ int s_prefix[];
    __shared__ T buf[64][3];
    const int lane = (int)threadIdx.x;
    const int j = bp_find(s_prefix, a.prefix, 2 * a.B);
    const int slot = j >> 1, idx = (int)blockIdx.x - s_prefix[j];
    const BpSlot *__restrict__ sl = a.slots + slot;
    const int K = sl->K, R = a.R, sh = sl->has_unl ? 0 : 1;
    const int kmax = K - 1 - sh;

    if (j & 1) {
        bp_unowned_rows(a.o, slot, R, K, sh, idx * 64 + lane);
        if (idx == 0 && lane == 0) {
            a.o.boff[slot] = sl->P;
            a.o.ioff[slot] = sl->I;
            if (slot == a.B - 1) { a.o.boff[a.B] = sl->P + sl->n; a.o.ioff[a.B] = sl->I + K; }
            if (slot == 0 && a.has_gt) a.o.gt_off[0] = 0;
        }
        return;
    }

    const int v = idx, voff = sl->voff;
    const int cnt = a.hist[voff + v + 1];
    if (cnt == 0) return;
    const int st = a.start[voff + v], r = a.rank[voff + v];
    const long long row0 = sl->row0;
    const int *__restrict__ sorted = a.sorted + row0;
    const float *__restrict__ x = a.xyz + 3 * row0;
    double m[9];
    for (int k = 0; k < 9; k++) m[k] = a.fp32 ? 0.0 : sl->m[k];
    T mn[3], mx[3], sum[3];
    for (int d = 0; d < 3; d++) { mn[d] = (T)INFINITY; mx[d] = (T)-INFINITY; sum[d] = (T)0; }
    for (int base = 0; base < cnt; base += 64) {
        int mm = cnt - base < 64 ? cnt - base : 64;
        if (lane < mm) {
            int p = sorted[st + base + lane];
            double y[3], s[3];
            bp_transform(x[3 * (size_t)p], x[3 * (size_t)p + 1], x[3 * (size_t)p + 2], m, a.fp32, a.scale, a.scale_f, y, s);
            for (int d = 0; d < 3; d++) {
                T val = (T)y[d];
                buf[lane][d] = val;
                mn[d] = val < mn[d] ? val : mn[d];
                mx[d] = val > mx[d] ? val : mx[d];
            }
        }
        __syncthreads();
        if (lane < 3)
            for (int q = 0; q < mm; q++) sum[lane] = sum[lane] + buf[q][lane];
        __syncthreads();
    }
    for (int off = 32; off > 0; off >>= 1)
        for (int d = 0; d < 3; d++) {
            T p = __shfl_xor(mn[d], off), q = __shfl_xor(mx[d], off);
            mn[d] = p < mn[d] ? p : mn[d];
            mx[d] = q > mx[d] ? q : mx[d];
        }
    double *__restrict__ is = a.istats + 9 * ((long long)sl->vbase + v);
    if (lane < 3) {
        is[lane] = (double)(sum[lane] / (T)cnt);
        is[3 + lane] = (double)mn[lane];
        is[6 + lane] = (double)mx[lane];
    }
    if (lane != 0) return;
    a.o.num_point[sl->I + r] = cnt;
    if (a.has_gt) a.o.gt_off[sl->I + r + 1] = sl->Q + st + cnt;   // each instance writes its END: the next one's start
    // enumerate(np.unique(ids), -1), as sp_instance_kernel: without unlabelled points the first instance gets k = -1 (the last row)
    // unless a later instance takes k = R - 1; k >= 128 and k >= R are skipped
    const int k = r - sh;
    if (k >= 128 || k >= R) return;
    if (k < 0 && R - 1 < 128 && kmax >= R - 1) return;
    const long long row = (long long)slot * R + (k < 0 ? R - 1 : k);
    bp_box_row<T>(a.o, row, a.sem[row0 + sorted[st]], v, mn, mx, a.mean_size);
}

// ---- stage 3: the point rows (job 2 * slot) and the GT proposal list (job 2 * slot + 1) ------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(BP_BLOCK) bp_stage3_kernel(BpArgs a) {
    extern __shared__ int s_prefix[];
    const int t = (int)threadIdx.x;
    const int j = bp_find(s_prefix, a.prefix, 2 * a.B);
    const int slot = j >> 1, tile = (int)blockIdx.x - s_prefix[j];
    const BpSlot *__restrict__ sl = a.slots + slot;
    const long long row0 = sl->row0;
    const int P = sl->P, I = sl->I;
    const int *__restrict__ ids = a.ids + row0;

    if (j & 1) {                                      // sp_gtidx_kernel's rows, column 0 + the instances, column 1 + the points before
        const int Lp = sl->Lp, shift = sl->has_unl ? 0 : 1;
        const int *__restrict__ sorted = a.sorted + row0;
        const int *__restrict__ rank = a.rank + sl->voff;
        int2 *__restrict__ out = (int2 *)a.o.gt_idx + sl->Q;
        for (int k = 0; k < BP_PTILE / BP_BLOCK; ++k) {
            int p = tile * BP_PTILE + t + k * BP_BLOCK;
            if (p < Lp) {
                int i = sorted[p];
                out[p] = make_int2(rank[ids[i]] - shift + I, i + P);
            }
        }
        return;
    }

    const int n = sl->n;
    double m[9], mnd[3];
    for (int k = 0; k < 9; k++) m[k] = a.fp32 ? 0.0 : sl->m[k];
    for (int d = 0; d < 3; d++) mnd[d] = sp_dec(a.smin[3 * slot + d]);
    const float *__restrict__ x = a.xyz + 3 * row0;
    const int *__restrict__ sem = a.sem + row0;
    const double *__restrict__ istats = a.istats + 9 * (long long)sl->vbase;
    for (int k = 0; k < BP_PTILE / BP_BLOCK; ++k) {
        int i = tile * BP_PTILE + t + k * BP_BLOCK;
        if (i >= n) continue;
        const long long g = (long long)P + i;
        double y[3], s[3];
        bp_transform(x[3 * (size_t)i], x[3 * (size_t)i + 1], x[3 * (size_t)i + 2], m, a.fp32, a.scale, a.scale_f, y, s);
        float ls[3];
        for (int d = 0; d < 3; d++) {
            a.o.locs[3 * g + d] = (float)y[d];
            // sp_offset_kernel, then sp_emit_kernel's cast (its crop offset is 0 here)
            if (a.fp32) ls[d] = (float)(double)((float)s[d] - (float)mnd[d]);
            else ls[d] = (float)((s[d] - mnd[d]) + 0.0);
        }
        longlong2 *lo = (longlong2 *)(a.o.locs_scaled + 4 * g);       // 32-byte rows from a 16-byte aligned base
        lo[0] = make_longlong2((long long)slot, (long long)ls[0]);
        lo[1] = make_longlong2((long long)ls[1], (long long)ls[2]);
        a.o.sem[g] = (long long)sem[i];
        const int v = ids[i];
        a.o.ids[g] = (long long)(v != -1 ? v + I : v);
        float o[12];
        if (v < 0) {
            for (int c = 0; c < 12; c++) o[c] = 0.0f;
        } else {                                      // sp_info_kernel: mean, (min + max) / 2, min, max
            const double *q = istats + 9 * (long long)v;
            for (int d = 0; d < 3; d++) {
                T mn = (T)q[3 + d], mx = (T)q[6 + d];
                o[d] = (float)q[d];
                o[3 + d] = (float)((mn + mx) / (T)2);
                o[6 + d] = (float)mn;
                o[9 + d] = (float)mx;
            }
        }
        float4 *io = (float4 *)(a.o.info + 12 * g);                   // 48-byte rows from a 16-byte aligned base
        io[0] = make_float4(o[0], o[1], o[2], o[3]);
        io[1] = make_float4(o[4], o[5], o[6], o[7]);
        io[2] = make_float4(o[8], o[9], o[10], o[11]);
    }
}

// ---- the table the call builds in host memory and copies to the device as it stands --------------------------------------------------
struct BpTable { BpSlot *slots; u64 *smin; int *prefix[3]; };
static void bp_table_layout(D3Carver &c, int B, BpTable &w) {
    w.slots = c.take<BpSlot>(B);
    w.smin = c.take<u64>(3 * (size_t)B);
    for (int k = 0; k < 3; k++) w.prefix[k] = c.take<int>(2 * (size_t)B + 1);
}
struct BpWs { char *table; double *istats; };
static void bp_ws_layout(D3Carver &c, size_t table_bytes, long long v_total, BpWs &w) {
    w.table = c.take<char>(table_bytes);
    w.istats = c.take<double>(9 * (size_t)(v_total < 1 ? 1 : v_total));
}

size_t d3_batch_prepare_table_bytes(int B) {
    if (B < 1 || B > BP_MAX_B) return 0;
    D3Carver c(nullptr, 0);
    BpTable w;
    bp_table_layout(c, B, w);
    return c.off;
}

size_t d3_batch_prepare_ws_bytes(int B, long long v_total) {
    const size_t tb = d3_batch_prepare_table_bytes(B);
    if (tb == 0 || v_total < 0 || v_total > (long long)BP_MAX_B * (SP_MAX_ID + 1)) return 0;
    D3Carver c(nullptr, 0);
    BpWs w;
    bp_ws_layout(c, tb, v_total, w);
    return c.off;
}

int d3_batch_prepare(const float *xyz, const float *feats, const int *sem, const int *ids, long long store_rows,
                     const int *ix_hist, const int *ix_rank, const int *ix_start, const int *ix_sorted, long long table_len,
                     const long long *row0_host, const int *slots_host, const double *mats_host, int B, int C, int R, int fp32,
                     int has_gt, double scale, const double *mean_size, void *const *out_host, void *table_host, void *ws,
                     size_t ws_bytes, void *stream) {
    if (B < 1 || B > BP_MAX_B || C < 0 || C > SP_MAX_FEAT || R < 1) return D3_ERR_RANGE;
    if (!xyz || !sem || !ids || !ix_hist || !ix_rank || !ix_start || !ix_sorted || !row0_host || !slots_host || !mean_size ||
        !out_host || !table_host || !ws || (C > 0 && !feats) || (!fp32 && !mats_host))
        return D3_ERR_ARG;
    // the int64 outputs; locs_scaled, instance_info and gt_bbox rows are stored 16 bytes at a time, gt_proposals_idx 8
    if (((size_t)out_host[3] | (size_t)out_host[4] | (size_t)out_host[12] | (size_t)out_host[13] | (size_t)out_host[15] |
         (size_t)out_host[17] | (size_t)out_host[18]) & 7)
        return D3_ERR_ARG;
    if (((size_t)out_host[1] | (size_t)out_host[5] | (size_t)out_host[19]) & 15) return D3_ERR_ARG;
    if (has_gt && ((size_t)out_host[7] & 7)) return D3_ERR_ARG;

    const size_t tb = d3_batch_prepare_table_bytes(B);
    D3Carver ch(table_host, tb);
    BpTable h;
    bp_table_layout(ch, B, h);
    const long long lim = 0x7fffffffll - BP_WTILE;
    long long P = 0, I = 0, Q = 0, Vt = 0, tiles[3] = {0, 0, 0};
    for (int i = 0; i < B; ++i) {
        const int *s = slots_host + 6 * i;
        const int n = s[0], voff = s[1], V = s[2], K = s[3], Lp = s[4];
        const long long row0 = row0_host[i];
        if (n < 0 || n > SP_MAX_POINTS || V < 1 || V > SP_MAX_ID + 1) return D3_ERR_RANGE;
        if ((long long)n * (C > 12 ? C : 12) > lim || (long long)R * 24 > lim) return D3_ERR_RANGE;
        if (row0 < 0 || row0 + n > store_rows || voff < 0 || (long long)voff + V + 1 > table_len || K < 0 || K > V || Lp < 0 || Lp > n)
            return D3_ERR_ARG;
        BpSlot &o = h.slots[i];
        o.row0 = row0; o.n = n; o.voff = voff; o.V = V; o.K = K; o.Lp = Lp; o.has_unl = s[5] != 0;
        o.P = (int)P; o.I = (int)I; o.Q = (int)Q; o.vbase = (int)Vt;
        for (int k = 0; k < 9; k++) o.m[k] = fp32 ? 0.0 : mats_host[9 * i + k];
        for (int d = 0; d < 3; d++) h.smin[3 * i + d] = ~0ull;
        h.prefix[0][2 * i] = (int)tiles[0];
        tiles[0] += (n + BP_PTILE - 1) / BP_PTILE;
        h.prefix[0][2 * i + 1] = (int)tiles[0];
        tiles[0] += ((long long)n * C + BP_WTILE - 1) / BP_WTILE;
        h.prefix[1][2 * i] = (int)tiles[1];
        tiles[1] += V;
        h.prefix[1][2 * i + 1] = (int)tiles[1];
        tiles[1] += (R + 63) / 64;
        h.prefix[2][2 * i] = (int)tiles[2];
        tiles[2] += (n + BP_PTILE - 1) / BP_PTILE;
        h.prefix[2][2 * i + 1] = (int)tiles[2];
        tiles[2] += has_gt ? (Lp + BP_PTILE - 1) / BP_PTILE : 0;
        P += n; I += K; Q += Lp; Vt += V;
        if (P > lim || I > lim || Q > lim || tiles[0] > lim || tiles[1] > lim || tiles[2] > lim) return D3_ERR_RANGE;
    }
    for (int k = 0; k < 3; k++) h.prefix[k][2 * B] = (int)tiles[k];
    for (int k = 0; k < BP_NOUT; ++k) {                   // an output without elements may be NULL
        const bool empty = k < 6 ? (P == 0 || (k == 2 && C == 0)) : k == 6 ? I == 0 : k == 7 ? (!has_gt || Q == 0) : k == 8 ? !has_gt : false;
        if (!out_host[k] && !empty) return D3_ERR_ARG;
    }

    D3Carver cw(ws, ws_bytes);
    BpWs w;
    bp_ws_layout(cw, tb, Vt, w);
    if (!cw.ok()) return D3_ERR_WORKSPACE;
    D3Carver cd(w.table, tb);
    BpTable d;
    bp_table_layout(cd, B, d);

    BpArgs a;
    a.xyz = xyz; a.feats = feats; a.sem = sem; a.ids = ids;
    a.hist = ix_hist; a.rank = ix_rank; a.start = ix_start; a.sorted = ix_sorted;
    a.mean_size = mean_size; a.slots = d.slots; a.smin = d.smin; a.istats = w.istats;
    a.B = B; a.C = C; a.R = R; a.fp32 = fp32 ? 1 : 0; a.has_gt = has_gt ? 1 : 0;
    a.scale = scale; a.scale_f = (float)scale;
    void *const *p = out_host;
    a.o = BpOut{(float *)p[0], (long long *)p[1], (float *)p[2], (long long *)p[3], (long long *)p[4], (float *)p[5], (int *)p[6],
                (int *)p[7], (int *)p[8], (int *)p[9], (int *)p[10], (float *)p[11], (long long *)p[12], (long long *)p[13],
                (float *)p[14], (long long *)p[15], (float *)p[16], (long long *)p[17], (long long *)p[18], (float *)p[19]};

    hipStream_t st = d3_stream(stream);
    const size_t lds = (2 * (size_t)B + 1) * sizeof(int);
    D3_CLEAR();
    // ONE copy: table_host is the caller's pinned buffer and must stay as it is until the copy has run
    D3_CHECK(hipMemcpyAsync(w.table, table_host, ch.off, hipMemcpyHostToDevice, st));
    if (tiles[0] > 0) {
        a.prefix = d.prefix[0];
        hipLaunchKernelGGL(bp_stage1_kernel, dim3((unsigned)tiles[0]), dim3(BP_BLOCK), lds, st, a);
        D3_LAUNCH_CHECK();
    }
    a.prefix = d.prefix[1];
    if (fp32) hipLaunchKernelGGL(bp_stage2_kernel<float>, dim3((unsigned)tiles[1]), dim3(64), lds, st, a);
    else hipLaunchKernelGGL(bp_stage2_kernel<double>, dim3((unsigned)tiles[1]), dim3(64), lds, st, a);
    D3_LAUNCH_CHECK();
    if (tiles[2] > 0) {
        a.prefix = d.prefix[2];
        if (fp32) hipLaunchKernelGGL(bp_stage3_kernel<float>, dim3((unsigned)tiles[2]), dim3(BP_BLOCK), lds, st, a);
        else hipLaunchKernelGGL(bp_stage3_kernel<double>, dim3((unsigned)tiles[2]), dim3(BP_BLOCK), lds, st, a);
        D3_LAUNCH_CHECK();
    }
    return 0;
}

// ==== the label-free scene half (lib/dataset/pipeline.py:352-380, :937-976): the test split's batch, which has no label key =========
// Nothing is drawn and no point is dropped there, so the per-scene minimum of fl32(x * scale) is a constant of the (store, scale)
// pair: d3_store_extents computes it ONCE for every scene of a store, and d3_points_batch is then a pure row-wise map from the
// store's rows to the batch's rows -- one launch, no reduction, no atomics, no read-back.  The expressions are stage 1's and
// stage 3's fp32 ones, so the keys equal the labelled path's bit for bit.
#define SE_MAX_S 8192                 // scenes per store: a prefix table of S + 1 ints in LDS (32 KiB)

struct SeScene { long long row0; int n, pad; };
struct SeArgs { const float *xyz; const SeScene *scenes; const int *prefix; u64 *ext; int S; float scale_f; };

// one launch over all scenes: job = scene, BP_PTILE points per block; the encoded minima are combined by the integer atomicMin
__global__ void __launch_bounds__(BP_BLOCK) se_extents_kernel(SeArgs a) {
    extern __shared__ int s_prefix[];
    __shared__ u64 s_min[BP_BLOCK / 64][3];
    const int t = (int)threadIdx.x;
    const int j = bp_find(s_prefix, a.prefix, a.S);
    const int tile = (int)blockIdx.x - s_prefix[j];
    const int n = a.scenes[j].n;
    const float *__restrict__ x = a.xyz + 3 * a.scenes[j].row0;
    u64 mn[3] = {~0ull, ~0ull, ~0ull};
    for (int k = 0; k < BP_PTILE / BP_BLOCK; ++k) {
        int i = tile * BP_PTILE + t + k * BP_BLOCK;
        if (i < n) {
            double y[3], s[3];
            bp_transform(x[3 * (size_t)i], x[3 * (size_t)i + 1], x[3 * (size_t)i + 2], nullptr, 1, 0.0, a.scale_f, y, s);
            for (int d = 0; d < 3; d++) {
                u64 e = sp_enc(s[d]);
                mn[d] = e < mn[d] ? e : mn[d];
            }
        }
    }
    for (int off = 32; off > 0; off >>= 1)
        for (int d = 0; d < 3; d++) {
            u64 b = __shfl_xor(mn[d], off);
            mn[d] = b < mn[d] ? b : mn[d];
        }
    if (d3_lane() == 0)
        for (int d = 0; d < 3; d++) s_min[t >> 6][d] = mn[d];
    __syncthreads();
    if (t < 3) {
        u64 v = s_min[0][t];
        for (int w = 1; w < BP_BLOCK / 64; w++) v = s_min[w][t] < v ? s_min[w][t] : v;
        atomicMin(&a.ext[3 * (size_t)j + t], v);
    }
}

struct SeTable { SeScene *scenes; int *prefix; };
static void se_table_layout(D3Carver &c, int S, SeTable &w) {
    w.scenes = c.take<SeScene>(S);
    w.prefix = c.take<int>((size_t)S + 1);
}
struct SeWs { char *table; };
static void se_ws_layout(D3Carver &c, size_t table_bytes, SeWs &w) { w.table = c.take<char>(table_bytes); }

size_t d3_store_extents_table_bytes(int S) {
    if (S < 1 || S > SE_MAX_S) return 0;
    D3Carver c(nullptr, 0);
    SeTable w;
    se_table_layout(c, S, w);
    return c.off;
}

size_t d3_store_extents_ws_bytes(int S) {
    const size_t tb = d3_store_extents_table_bytes(S);
    if (tb == 0) return 0;
    D3Carver c(nullptr, 0);
    SeWs w;
    se_ws_layout(c, tb, w);
    return c.off;
}

int d3_store_extents(const float *xyz, long long store_rows, const long long *offsets_host, int S, double scale,
                     unsigned long long *extents, void *table_host, void *ws, size_t ws_bytes, void *stream) {
    if (S < 1 || S > SE_MAX_S) return D3_ERR_RANGE;
    if (!xyz || !offsets_host || !extents || !table_host || !ws || ((size_t)extents & 7)) return D3_ERR_ARG;
    const size_t tb = d3_store_extents_table_bytes(S);
    D3Carver ch(table_host, tb);
    SeTable h;
    se_table_layout(ch, S, h);
    const long long lim = 0x7fffffffll - BP_WTILE;
    long long tiles = 0;
    for (int i = 0; i < S; ++i) {
        const long long row0 = offsets_host[i], n = offsets_host[i + 1] - row0;
        if (n < 1 || n > SP_MAX_POINTS) return D3_ERR_RANGE;            // points.min(0) of an empty scene raises in the reference
        if (row0 < 0 || row0 + n > store_rows) return D3_ERR_ARG;
        h.scenes[i].row0 = row0; h.scenes[i].n = (int)n; h.scenes[i].pad = 0;
        h.prefix[i] = (int)tiles;
        tiles += (n + BP_PTILE - 1) / BP_PTILE;
        if (tiles > lim) return D3_ERR_RANGE;
    }
    h.prefix[S] = (int)tiles;

    D3Carver cw(ws, ws_bytes);
    SeWs w;
    se_ws_layout(cw, tb, w);
    if (!cw.ok()) return D3_ERR_WORKSPACE;
    D3Carver cd(w.table, tb);
    SeTable d;
    se_table_layout(cd, S, d);

    SeArgs a;
    a.xyz = xyz; a.scenes = d.scenes; a.prefix = d.prefix; a.ext = (u64 *)extents; a.S = S; a.scale_f = (float)scale;
    hipStream_t st = d3_stream(stream);
    D3_CLEAR();
    D3_CHECK(hipMemcpyAsync(w.table, table_host, ch.off, hipMemcpyHostToDevice, st));
    D3_CHECK(hipMemsetAsync(extents, 0xff, 3 * (size_t)S * sizeof(u64), st));      // the start value of every minimum: ~0
    hipLaunchKernelGGL(se_extents_kernel, dim3((unsigned)tiles), dim3(BP_BLOCK), ((size_t)S + 1) * sizeof(int), st, a);
    D3_LAUNCH_CHECK();
    return 0;
}

struct PbSlot { long long row0; int n, srow, P, pad; };   // first store row, points, the scene's store row, points of the slots before
struct PbArgs {
    const float *xyz, *feats;
    const u64 *ext;                   // (S,3) d3_store_extents
    const PbSlot *slots;
    const int *prefix;                // 2 jobs per slot, 2 * B + 1 entries
    float *locs; long long *locs_scaled; float *ofeats; int *boff;
    int B, C; float scale_f;
};

// the point rows (job 2 * slot; its first thread also writes the slot's batch_offsets entry) and the feature words (job 2 * slot + 1)
__global__ void __launch_bounds__(BP_BLOCK) pb_points_kernel(PbArgs a) {
    extern __shared__ int s_prefix[];
    const int t = (int)threadIdx.x;
    const int j = bp_find(s_prefix, a.prefix, 2 * a.B);
    const int slot = j >> 1, tile = (int)blockIdx.x - s_prefix[j];
    const PbSlot *__restrict__ sl = a.slots + slot;
    const int n = sl->n, P = sl->P;
    const long long row0 = sl->row0;

    if (j & 1) {                                                  // bp_stage1_kernel's copy
        const long long count = (long long)n * a.C, base = (long long)tile * BP_WTILE;
        const unsigned *__restrict__ src = (const unsigned *)a.feats + row0 * a.C;
        unsigned *__restrict__ dst = (unsigned *)a.ofeats + (long long)P * a.C;
        if ((((size_t)src | (size_t)dst) & 15) == 0) {            // 16-byte accesses, the four loads in flight together
            const uint4 *__restrict__ s4 = (const uint4 *)(src + base) + t;
            uint4 *__restrict__ d4 = (uint4 *)(dst + base) + t;
            if (base + BP_WTILE <= count) {
                uint4 v0 = s4[0], v1 = s4[BP_BLOCK], v2 = s4[2 * BP_BLOCK], v3 = s4[3 * BP_BLOCK];
                d4[0] = v0; d4[BP_BLOCK] = v1; d4[2 * BP_BLOCK] = v2; d4[3 * BP_BLOCK] = v3;
            } else {                                              // the slot's last tile
                for (int k = 0; k < BP_WTILE / (4 * BP_BLOCK); ++k) {
                    const long long w = base + 4ll * (k * BP_BLOCK + t);
                    if (w + 4 <= count) d4[k * BP_BLOCK] = s4[k * BP_BLOCK];
                    else
                        for (long long u = w; u < count; ++u) dst[u] = src[u];   // at most 3 words, in one thread
                }
            }
        } else {                                                  // lane-consecutive words
            for (int k = 0; k < BP_WTILE / BP_BLOCK; ++k) {
                long long w = base + t + k * BP_BLOCK;
                if (w < count) dst[w] = src[w];
            }
        }
        return;
    }

    if (tile == 0 && t == 0) {                                    // every slot has points, so every slot has this block
        a.boff[slot] = P;
        if (slot == a.B - 1) a.boff[a.B] = P + n;
    }
    double mnd[3];
    for (int d = 0; d < 3; d++) mnd[d] = sp_dec(a.ext[3 * (size_t)sl->srow + d]);
    const float *__restrict__ x = a.xyz + 3 * row0;
    for (int k = 0; k < BP_PTILE / BP_BLOCK; ++k) {
        int i = tile * BP_PTILE + t + k * BP_BLOCK;
        if (i >= n) continue;
        const long long g = (long long)P + i;
        double y[3], s[3];
        bp_transform(x[3 * (size_t)i], x[3 * (size_t)i + 1], x[3 * (size_t)i + 2], nullptr, 1, 0.0, a.scale_f, y, s);
        float ls[3];
        for (int d = 0; d < 3; d++) {
            a.locs[3 * g + d] = (float)y[d];
            ls[d] = (float)(double)((float)s[d] - (float)mnd[d]);     // bp_stage3_kernel's fp32 expression
        }
        longlong2 *lo = (longlong2 *)(a.locs_scaled + 4 * g);         // 32-byte rows from a 16-byte aligned base
        lo[0] = make_longlong2((long long)slot, (long long)ls[0]);
        lo[1] = make_longlong2((long long)ls[1], (long long)ls[2]);
    }
}

struct PbTable { PbSlot *slots; int *prefix; };
static void pb_table_layout(D3Carver &c, int B, PbTable &w) {
    w.slots = c.take<PbSlot>(B);
    w.prefix = c.take<int>(2 * (size_t)B + 1);
}
struct PbWs { char *table; };
static void pb_ws_layout(D3Carver &c, size_t table_bytes, PbWs &w) { w.table = c.take<char>(table_bytes); }

size_t d3_points_batch_table_bytes(int B) {
    if (B < 1 || B > BP_MAX_B) return 0;
    D3Carver c(nullptr, 0);
    PbTable w;
    pb_table_layout(c, B, w);
    return c.off;
}

size_t d3_points_batch_ws_bytes(int B) {
    const size_t tb = d3_points_batch_table_bytes(B);
    if (tb == 0) return 0;
    D3Carver c(nullptr, 0);
    PbWs w;
    pb_ws_layout(c, tb, w);
    return c.off;
}

int d3_points_batch(const float *xyz, const float *feats, long long store_rows, const unsigned long long *extents, int S,
                    const long long *row0_host, const int *srow_host, const int *n_host, int B, int C, double scale,
                    float *locs, long long *locs_scaled, float *out_feats, int *batch_offsets, void *table_host, void *ws,
                    size_t ws_bytes, void *stream) {
    if (B < 1 || B > BP_MAX_B || C < 0 || C > SP_MAX_FEAT || S < 1) return D3_ERR_RANGE;
    if (!xyz || !extents || !row0_host || !srow_host || !n_host || !locs || !locs_scaled || !batch_offsets || !table_host || !ws ||
        (C > 0 && (!feats || !out_feats)))
        return D3_ERR_ARG;
    // locs_scaled rows are stored 16 bytes at a time
    if (((size_t)locs_scaled & 15) || (((size_t)locs | (size_t)out_feats | (size_t)batch_offsets | (size_t)extents) & 3) ||
        ((size_t)extents & 7))
        return D3_ERR_ARG;

    const size_t tb = d3_points_batch_table_bytes(B);
    D3Carver ch(table_host, tb);
    PbTable h;
    pb_table_layout(ch, B, h);
    const long long lim = 0x7fffffffll - BP_WTILE;
    long long P = 0, tiles = 0;
    for (int i = 0; i < B; ++i) {
        const int n = n_host[i], srow = srow_host[i];
        const long long row0 = row0_host[i];
        if (n < 1 || n > SP_MAX_POINTS) return D3_ERR_RANGE;             // n == 0: points.min(0) raises in the reference
        if ((long long)n * (C > 4 ? C : 4) > lim) return D3_ERR_RANGE;
        if (row0 < 0 || row0 + n > store_rows || srow < 0 || srow >= S) return D3_ERR_ARG;
        PbSlot &o = h.slots[i];
        o.row0 = row0; o.n = n; o.srow = srow; o.P = (int)P; o.pad = 0;
        h.prefix[2 * i] = (int)tiles;
        tiles += (n + BP_PTILE - 1) / BP_PTILE;
        h.prefix[2 * i + 1] = (int)tiles;
        tiles += ((long long)n * C + BP_WTILE - 1) / BP_WTILE;
        P += n;
        if (P > lim || tiles > lim) return D3_ERR_RANGE;
    }
    h.prefix[2 * B] = (int)tiles;

    D3Carver cw(ws, ws_bytes);
    PbWs w;
    pb_ws_layout(cw, tb, w);
    if (!cw.ok()) return D3_ERR_WORKSPACE;
    D3Carver cd(w.table, tb);
    PbTable d;
    pb_table_layout(cd, B, d);

    PbArgs a;
    a.xyz = xyz; a.feats = feats; a.ext = (const u64 *)extents; a.slots = d.slots; a.prefix = d.prefix;
    a.locs = locs; a.locs_scaled = locs_scaled; a.ofeats = out_feats; a.boff = batch_offsets;
    a.B = B; a.C = C; a.scale_f = (float)scale;
    hipStream_t st = d3_stream(stream);
    D3_CLEAR();
    // ONE copy: table_host is the caller's pinned buffer and must stay as it is until the copy has run
    D3_CHECK(hipMemcpyAsync(w.table, table_host, ch.off, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(pb_points_kernel, dim3((unsigned)tiles), dim3(BP_BLOCK), (2 * (size_t)B + 1) * sizeof(int), st, a);
    D3_LAUNCH_CHECK();
    return 0;
}
