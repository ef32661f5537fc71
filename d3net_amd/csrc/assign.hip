// assign.hip -- dense-caption evaluation: GIoU cost and Hungarian assignment on the device (gfx950).
//
// Replaces, per validation batch, lib/captioning/eval_helper.py:120-182 (box_assignment: the cost matrix, its copy to the host and
// scipy.optimize.linear_sum_assignment once per scene), with lib/utils/bbox.py generalized_box3d_iou (axis-aligned path) computed
// inside the kernel.  Two entry points share one solver body (ls_solve):
//   d3_lsap_batched           the cost matrix is given (B, R, C); entries are read from global memory where the solver needs them;
//   d3_dense_caption_assign   cost = -GIoU of (proposal, GT) box pairs, recomputed from twelve per-box floats wherever the solver
//                             needs an entry: the matrix never exists unless the caller asks for it (cost_out).
//
// Layout: one workgroup of 256 threads per scene.  All four waves run the prologue (per-box quantities into LDS, the non-finite
// scan over the valid entries, cost_out); after ONE barrier waves 1-3 retire and wave 0 alone runs the solver with no barrier
// and no LDS write at all: the chain of dependent argmin steps is cross-lane traffic inside one wave.
//   column j of the (nr <= nc <= 256) problem lives in lane j & 63, slot j >> 6 (four slots): v, shortest path cost sp, path,
//     row4col, its position in scipy's `remaining` array and (GIoU) its box; row i likewise: u, col4row, "in SR" and the minVal at
//     which the row was reached (== sp[col4row[i]], so the dual update needs no gather);
//   a step = one row broadcast (readlane), four entries per lane, a lexicographic (sp, tie key) butterfly over 64 lanes.
// The solver is scipy's (rectangular_lsap.cpp, Crouse's shortest augmenting path) in float64 with scipy's scan order restated
// as a comparison key -- smaller sp; then an unassigned column before an assigned one; among unassigned the LARGEST position in
// `remaining`, among assigned the SMALLEST -- so assignments, ties included, are scipy's.  Every loop is bounded by nr or nc.
#include "common.h"
#include <limits.h>

#define LS_MAX 256        // rows and columns per scene
#define LS_SLOTS 4        // LS_MAX / 64
#define LS_THREADS 256

// per-box quantities of the cost: AABB over the 8 corners, clamped edge volume, and the five corner coordinates the
// reference's footprint / height terms read (corner 0: x, z; corner 2: x, z; corner 4: z)
struct LsBox { float lox, loy, loz, hix, hiy, hiz, vol, c0x, c0z, c2x, c2z, c4z; };

// PROP: a NaN operand gives NaN, like torch.minimum / maximum / clamp (the prologue decides "non-finite" with these); !PROP: one
// instruction (the solver, which only runs once the prologue has seen every entry finite, where both forms agree)
template <bool PROP> __device__ __forceinline__ float ls_min(float a, float b) {
    if (PROP) return (a < b || a != a) ? a : b;
    return fminf(a, b);
}
template <bool PROP> __device__ __forceinline__ float ls_max(float a, float b) {
    if (PROP) return (a > b || a != a) ? a : b;
    return fmaxf(a, b);
}

__device__ __forceinline__ float ls_edge(const float *c, int i, int j) {
    const float dx = c[i * 3] - c[j * 3], dy = c[i * 3 + 1] - c[j * 3 + 1], dz = c[i * 3 + 2] - c[j * 3 + 2];
    return sqrtf(ls_max<true>((dx * dx + dy * dy) + dz * dz, 1e-6f));
}

__device__ __forceinline__ LsBox ls_boxq(const float *__restrict__ c) {
    LsBox q;
    q.lox = q.hix = c[0]; q.loy = q.hiy = c[1]; q.loz = q.hiz = c[2];
#pragma unroll
    for (int k = 1; k < 8; k++) {
        q.lox = ls_min<true>(q.lox, c[k * 3]);     q.hix = ls_max<true>(q.hix, c[k * 3]);
        q.loy = ls_min<true>(q.loy, c[k * 3 + 1]); q.hiy = ls_max<true>(q.hiy, c[k * 3 + 1]);
        q.loz = ls_min<true>(q.loz, c[k * 3 + 2]); q.hiz = ls_max<true>(q.hiz, c[k * 3 + 2]);
    }
    q.vol = ls_max<true>((ls_edge(c, 0, 1) * ls_edge(c, 1, 2)) * ls_edge(c, 0, 4), 1e-8f);
    q.c0x = c[0]; q.c0z = c[2]; q.c2x = c[6]; q.c2z = c[8]; q.c4z = c[14];
    return q;
}

// cost = -GIoU of proposal a and GT b, fp32 in the host path's operation order (caption_eval.generalized_box3d_iou)
template <bool PROP> __device__ __forceinline__ float ls_giou_cost(const LsBox &a, const LsBox &b) {
    const float top = ls_min<PROP>(a.c0z, b.c0z);
    const float height = ls_max<PROP>(top - ls_max<PROP>(a.c4z, b.c4z), 0.f);
    const float w0 = ls_max<PROP>(ls_min<PROP>(a.c0x, b.c0x) - ls_max<PROP>(a.c2x, b.c2x), 0.f);
    const float w1 = ls_max<PROP>(top - ls_max<PROP>(a.c2z, b.c2z), 0.f);
    const float inter = (w0 * w1) * height;
    const float ex = fabsf(ls_max<PROP>(a.hix, b.hix) - ls_min<PROP>(a.lox, b.lox));
    const float ey = fabsf(ls_max<PROP>(a.hiy, b.hiy) - ls_min<PROP>(a.loy, b.loy));
    const float ez = fabsf(ls_max<PROP>(a.hiz, b.hiz) - ls_min<PROP>(a.loz, b.loz));
    const float enclosing = (ex * ey) * ez;
    const float s = a.vol + b.vol;
    const float good = (enclosing > 2e-8f && s > 4e-8f) ? 1.f : 0.f;
    const float uni = ls_max<PROP>(s - inter, 1e-8f);
    return -((inter / uni - (1.f - uni / enclosing)) * good);
}

__device__ __forceinline__ bool ls_finite(float x) { return fabsf(x) <= 3.402823466e+38f; }

// ---- cost accessors: load_row(i) once per step (wave-uniform i), at(i, q, j) for the lane's column j of slot q
struct LsMatCost {
    const float *c; long long rs, cs;                 // entry (i, j) = c[i rs + j cs]: cs == 1 as given, rs == 1 transposed
    __device__ __forceinline__ void load_row(int) {}
    __device__ __forceinline__ float at(int i, int, int j) const { return c[i * rs + j * cs]; }
};

struct LsBoxCost {
    const LsBox *rows;                                // LDS: the solver's rows (GT boxes when transposed, else proposals)
    LsBox col[LS_SLOTS], row;
    bool rows_are_gt;
    __device__ __forceinline__ void load_row(int i) { row = rows[i]; }
    __device__ __forceinline__ float at(int, int q, int) const {
        return rows_are_gt ? ls_giou_cost<false>(col[q], row) : ls_giou_cost<false>(row, col[q]);
    }
};

// ---- slot helpers: q is wave-uniform, the arrays stay in registers
template <typename T> __device__ __forceinline__ T ls_pick(const T (&a)[LS_SLOTS], int q) {
    return q == 0 ? a[0] : (q == 1 ? a[1] : (q == 2 ? a[2] : a[3]));
}
template <typename T> __device__ __forceinline__ void ls_put(T (&a)[LS_SLOTS], int q, T x) {
#pragma unroll
    for (int s = 0; s < LS_SLOTS; s++)
        if (s == q) a[s] = x;
}
__device__ __forceinline__ int ls_read_i(int x, int lane) { return __builtin_amdgcn_readlane(x, lane); }
__device__ __forceinline__ double ls_read_d(double x, int lane) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(x), lane), hi = __builtin_amdgcn_readlane(__double2hiint(x), lane);
    return __hiloint2double(hi, lo);
}

// One wave.  nr <= nc <= LS_MAX.  -> 0, or 2 when the problem is infeasible; row4col[q] of column q * 64 + lane and col4row[q]
// of row q * 64 + lane (-1: none).
template <class Cost>
__device__ __forceinline__ int ls_solve(Cost &cost, const int nr, const int nc, int (&row4col)[LS_SLOTS], int (&col4row)[LS_SLOTS]) {
    const int lane = threadIdx.x & 63;
    const double INF = __longlong_as_double(0x7ff0000000000000LL);
    double u[LS_SLOTS], reached[LS_SLOTS], v[LS_SLOTS], sp[LS_SLOTS];
    int path[LS_SLOTS], pos[LS_SLOTS];
#pragma unroll
    for (int q = 0; q < LS_SLOTS; q++) { u[q] = 0.0; v[q] = 0.0; reached[q] = 0.0; row4col[q] = -1; col4row[q] = -1; }
    for (int cur = 0; cur < nr; cur++) {
#pragma unroll
        for (int q = 0; q < LS_SLOTS; q++) {
            const int j = q * 64 + lane;
            pos[q] = j < nc ? nc - 1 - j : -1;        // remaining[it] = nc - 1 - it; -1 = not in `remaining` (SC, or no such column)
            sp[q] = INF;
            path[q] = -1;
        }
        int in_sr = 0, num_remaining = nc, i = cur, sink = -1;
        double minVal = 0.0;
        for (int step = 0; step < nc && sink < 0; step++) {
            if (lane == (i & 63)) { in_sr |= 1 << (i >> 6); ls_put(reached, i >> 6, minVal); }
            const double ui = ls_read_d(ls_pick(u, i >> 6), i & 63);
            cost.load_row(i);
            double bs = INF;
            int bk = INT_MAX;
#pragma unroll
            for (int q = 0; q < LS_SLOTS; q++) {
                if (pos[q] >= 0) {
                    const int j = q * 64 + lane;
                    const double r = ((minVal + (double)cost.at(i, q, j)) - ui) - v[q];
                    if (r < sp[q]) { path[q] = i; sp[q] = r; }
                    const int key = (((row4col[q] < 0) ? 0xFFFF - pos[q] : 0x10000 + pos[q]) << 8) | j;
                    if (sp[q] < bs || (sp[q] == bs && key < bk)) { bs = sp[q]; bk = key; }
                }
            }
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) {
                const double os = __shfl_xor(bs, m, 64);
                const int ok = __shfl_xor(bk, m, 64);
                if (os < bs || (os == bs && ok < bk)) { bs = os; bk = ok; }
            }
            bk = __builtin_amdgcn_readfirstlane(bk);
            bs = ls_read_d(bs, 0);
            if (bk == INT_MAX || !(bs < INF)) return 2;
            minVal = bs;
            const int j = bk & 255, tie = bk >> 8;
            const bool assigned = tie >= 0x10000;
            const int index = assigned ? tie - 0x10000 : 0xFFFF - tie;
            const int last = --num_remaining;         // remaining[index] = remaining[--num_remaining]
#pragma unroll
            for (int q = 0; q < LS_SLOTS; q++)
                if (pos[q] == last) pos[q] = index;
            if (lane == (j & 63)) ls_put(pos, j >> 6, -1);
            if (!assigned) sink = j;
            else i = ls_read_i(ls_pick(row4col, j >> 6), j & 63);
        }
        if (sink < 0) return 2;
        // dual update: u[cur] += minVal; u[i] += minVal - sp[col4row[i]] for the other rows in SR; v[j] -= minVal - sp[j] for SC
#pragma unroll
        for (int q = 0; q < LS_SLOTS; q++) {
            if (q * 64 + lane == cur) u[q] += minVal;
            else if ((in_sr >> q) & 1) u[q] += minVal - reached[q];
            if (q * 64 + lane < nc && pos[q] < 0) v[q] -= minVal - sp[q];
        }
        // augment along the path from the sink back to cur
        int j = sink;
        for (int hop = 0; hop < nr; hop++) {
            const int r = ls_read_i(ls_pick(path, j >> 6), j & 63);
            if (lane == (j & 63)) ls_put(row4col, j >> 6, r);
            const int prev = ls_read_i(ls_pick(col4row, r >> 6), r & 63);
            if (lane == (r & 63)) ls_put(col4row, r >> 6, j);
            j = prev;
            if (r == cur) break;
        }
    }
    return 0;
}

// wave 0 writes every element of out (C) once: out[col] = row of the pair, 0 for an unassigned or invalid column or a failed scene
__device__ __forceinline__ void ls_write(int *out, int C, int n, bool transposed, int st, const int (&row4col)[LS_SLOTS],
                                         const int (&col4row)[LS_SLOTS]) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int q = 0; q < LS_SLOTS; q++) {
        const int c = q * 64 + lane;
        if (c < C) {
            const int r = transposed ? col4row[q] : row4col[q];      // transposed: the solver's row c is column c
            out[c] = (st == 0 && c < n && r > 0) ? r : 0;
        }
    }
}

__global__ __launch_bounds__(LS_THREADS) void ls_lsap_kernel(const float *__restrict__ cost, const int *__restrict__ ncols, int R, int C,
                                                             int *__restrict__ per_col, int *__restrict__ status) {
    const int b = blockIdx.x, t = threadIdx.x;
    const int n = min(max(ncols[b], 0), C);
    const float *cb = cost + (size_t)b * R * C;
    int bad = 0;
    for (int e = t; e < R * n; e += LS_THREADS) {
        const int r = e / n, c = e - r * n;
        if (!ls_finite(cb[r * C + c])) bad = 1;
    }
    bad = __syncthreads_or(bad);
    if (t >= 64) return;
    int row4col[LS_SLOTS] = {-1, -1, -1, -1}, col4row[LS_SLOTS] = {-1, -1, -1, -1};
    const bool transposed = n < R;
    int st = bad ? 1 : 0;
    if (!bad && n > 0) {
        LsMatCost mc = {cb, transposed ? 1 : (long long)C, transposed ? (long long)C : 1};
        st = ls_solve(mc, min(R, n), max(R, n), row4col, col4row);
    }
    ls_write(per_col + (size_t)b * C, C, n, transposed, st, row4col, col4row);
    if (t == 0) status[b] = st;
}

__global__ __launch_bounds__(LS_THREADS) void ls_giou_kernel(const float *__restrict__ pred, const float *__restrict__ gt,
                                                             const int *__restrict__ nactual, int K, int G, int *__restrict__ per_gt,
                                                             int *__restrict__ status, float *__restrict__ cost_out) {
    __shared__ LsBox pb[LS_MAX], gb[LS_MAX];
    const int b = blockIdx.x, t = threadIdx.x;
    const int n = min(max(nactual[b], 0), G);
    for (int e = t; e < K + n; e += LS_THREADS) {
        if (e < K) pb[e] = ls_boxq(pred + ((size_t)b * K + e) * 24);
        else gb[e - K] = ls_boxq(gt + ((size_t)b * G + (e - K)) * 24);
    }
    __syncthreads();
    int bad = 0;
    const int W = cost_out ? G : n;                   // the padded columns are only visited to write their zeros
    for (int e = t; e < K * W; e += LS_THREADS) {
        const int k = e / W, g = e - k * W;
        float c = 0.f;
        if (g < n) {
            c = ls_giou_cost<true>(pb[k], gb[g]);
            if (!ls_finite(c)) bad = 1;
        }
        if (cost_out) cost_out[((size_t)b * K + k) * G + g] = c;
    }
    bad = __syncthreads_or(bad);
    if (t >= 64) return;
    int row4col[LS_SLOTS] = {-1, -1, -1, -1}, col4row[LS_SLOTS] = {-1, -1, -1, -1};
    const bool transposed = n < K;
    int st = bad ? 1 : 0;
    if (!bad && n > 0) {
        const int nc = max(K, n);
        LsBoxCost bc;
        bc.rows = transposed ? gb : pb;
        bc.rows_are_gt = transposed;
        const LsBox *cols = transposed ? pb : gb;
#pragma unroll
        for (int q = 0; q < LS_SLOTS; q++) bc.col[q] = cols[min(q * 64 + t, nc - 1)];
        bc.row = bc.rows[0];
        st = ls_solve(bc, min(K, n), nc, row4col, col4row);
    }
    ls_write(per_gt + (size_t)b * G, G, n, transposed, st, row4col, col4row);
    if (t == 0) status[b] = st;
}

// ------------------------------------------------------------------------------------------------- host
static int ls_check(int B, int R, int C) {
    if (B < 1 || R < 1 || C < 1) return D3_ERR_ARG;
    if (R > LS_MAX || C > LS_MAX) return D3_ERR_RANGE;
    return 0;
}

extern "C" int d3_lsap_batched(const float *cost, const int *ncols, int B, int R, int C, int *per_col, int *status, void *stream) {
    D3_CLEAR();
    if (!cost || !ncols || !per_col || !status) return D3_ERR_ARG;
    const int rc = ls_check(B, R, C);
    if (rc) return rc;
    ls_lsap_kernel<<<B, LS_THREADS, 0, d3_stream(stream)>>>(cost, ncols, R, C, per_col, status);
    D3_LAUNCH_CHECK();
    return 0;
}

extern "C" int d3_dense_caption_assign(const float *pred_boxes, const float *gt_boxes, const int *nactual, int B, int K, int G, int *per_gt,
                                       int *status, float *cost_out, void *stream) {
    D3_CLEAR();
    if (!pred_boxes || !gt_boxes || !nactual || !per_gt || !status) return D3_ERR_ARG;
    const int rc = ls_check(B, K, G);
    if (rc) return rc;
    ls_giou_kernel<<<B, LS_THREADS, 0, d3_stream(stream)>>>(pred_boxes, gt_boxes, nactual, K, G, per_gt, status, cost_out);
    D3_LAUNCH_CHECK();
    return 0;
}
