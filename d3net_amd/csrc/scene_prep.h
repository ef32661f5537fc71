// scene_prep.h -- what scene_prep.hip (one scene at a time), batch_prep.hip (a batch from the scene store) and batch_elastic.hip
// (the augmented detector-only batch from the store) share: the limits, the order-preserving integer image of a double that
// carries the deterministic min / max reductions, and the per-point / per-cell arithmetic, so that each expression exists once.
#pragma once
#include "common.h"

#define SP_MAX_POINTS (1 << 24)
#define SP_MAX_GRID_DIM 2048
#define SP_MAX_GRID (1 << 25)
#define SP_MAX_ID 65535
#define SP_MAX_FEAT 256
#define SP_BLOCK 256

typedef unsigned long long u64;

// order-preserving u64 image of a double (a < b  <=>  enc(a) < enc(b)); the host decodes it (scene_prep.py)
__device__ __forceinline__ u64 sp_enc(double d) {
    u64 b = (u64)__double_as_longlong(d);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double sp_dec(u64 e) {
    u64 b = (e >> 63) ? (e & 0x7fffffffffffffffull) : ~e;
    return __longlong_as_double((long long)b);
}

// loads the prefix table into LDS and returns the job j with s_prefix[j] <= b < s_prefix[j + 1] (jobs without tiles are skipped)
__device__ __forceinline__ int bp_find(int *s_prefix, const int *__restrict__ prefix, int J) {
    for (int i = (int)threadIdx.x; i <= J; i += (int)blockDim.x) s_prefix[i] = prefix[i];
    __syncthreads();
    const int b = (int)blockIdx.x;
    int lo = 0, hi = J;
    while (hi - lo > 1) {
        int mid = (lo + hi) >> 1;
        if (s_prefix[mid] <= b) lo = mid; else hi = mid;
    }
    return lo;
}

// sp_transform_kernel's two paths for one point
__device__ __forceinline__ void bp_transform(float x0, float x1, float x2, const double *m, int fp32, double scale, float scale_f,
                                             double *y, double *s) {
    if (fp32) {                                       // points.copy() * scale: float32
        y[0] = x0; y[1] = x1; y[2] = x2;
        s[0] = (double)(x0 * scale_f); s[1] = (double)(x1 * scale_f); s[2] = (double)(x2 * scale_f);
    } else {                                          // np.matmul(xyz, m) in float64, then * scale
        for (int j = 0; j < 3; j++) {
            double v = (double)x0 * m[j] + (double)x1 * m[3 + j];
            v = v + (double)x2 * m[6 + j];
            y[j] = v;
            s[j] = v * scale;
        }
    }
}

// ---- device noise: Philox4x32-10 + Box-Muller, counter = element index / 4, key = seed --------------------------------------
__device__ __forceinline__ uint4 sp_philox(uint4 c, uint2 k) {
    for (int r = 0; r < 10; r++) {
        unsigned lo0 = 0xD2511F53u * c.x, hi0 = __umulhi(0xD2511F53u, c.x);
        unsigned lo1 = 0xCD9E8D57u * c.z, hi1 = __umulhi(0xCD9E8D57u, c.z);
        c = make_uint4(hi1 ^ c.y ^ k.x, lo1, hi0 ^ c.w ^ k.y, lo0);
        k.x += 0x9E3779B9u; k.y += 0xBB67AE85u;
    }
    return c;
}

// the four normals of counter t: elements 4 t .. 4 t + 3 of the noise stream `seed`
__device__ __forceinline__ void sp_noise_quad(long long t, u64 seed, float z[4]) {
    uint4 r = sp_philox(make_uint4((unsigned)t, (unsigned)(t >> 32), 0u, 0u), make_uint2((unsigned)seed, (unsigned)(seed >> 32)));
    const float inv = 2.3283064365386963e-10f;                 // 2^-32
    float u1 = ((float)r.x + 1.0f) * inv, u2 = (float)r.y * inv;  // u1 in (0, 1]
    float u3 = ((float)r.z + 1.0f) * inv, u4 = (float)r.w * inv;
    u1 = fminf(u1, 1.0f); u3 = fminf(u3, 1.0f);
    float ra = sqrtf(-2.0f * logf(u1)), rb = sqrtf(-2.0f * logf(u3));
    z[0] = ra * cospif(2.0f * u2); z[1] = ra * sinpif(2.0f * u2);
    z[2] = rb * cospif(2.0f * u4); z[3] = rb * sinpif(2.0f * u4);
}

// one output of a 3-tap box pass: scipy.ndimage.convolve accumulates input * float32(1/3) in double over offsets -1, 0, +1 and
// rounds the sum to float32 (a / d: the neighbours, 0 outside the grid)
__device__ __forceinline__ float sp_blur_tap(float a, float b, float d) {
    const double w = (double)(1.0f / 3.0f);
    double t = 0.0;
    t += (double)a * w;
    t += (double)b * w;
    t += (double)d * w;
    return (float)t;
}

// largest k in [0, L-2] with ax[k] <= x (scipy's find_interval_ascending, in-range x)
__device__ __forceinline__ int sp_interval(const double *ax, int L, double x) {
    int lo = 0, hi = L - 1;
    while (lo < hi - 1) {
        int mid = (lo + hi) >> 1;
        if (x < ax[mid]) hi = mid; else lo = mid;
    }
    return lo;
}

// RegularGridInterpolator(ax, noise, bounds_error=0, fill_value=0) at the point s3, then s3 += g * mag; g (3, X, Y, Z), axes the
// three coordinate axes one after the other
__device__ __forceinline__ void sp_interp_point(double *__restrict__ s3, const float *__restrict__ g, const double *__restrict__ axes,
                                                int X, int Y, int Z, double mag) {
    const double *ax[3] = {axes, axes + X, axes + X + Y};
    int L[3] = {X, Y, Z};
    long long per = (long long)X * Y * Z;
    double x[3] = {s3[0], s3[1], s3[2]};
    int idx[3];
    double y[3];
    bool oob = false;
    for (int d = 0; d < 3; d++) {
        oob = oob || x[d] < ax[d][0] || x[d] > ax[d][L[d] - 1];
        idx[d] = sp_interval(ax[d], L[d], x[d]);
        y[d] = (x[d] - ax[d][idx[d]]) / (ax[d][idx[d] + 1] - ax[d][idx[d]]);
    }
    double v[3] = {0.0, 0.0, 0.0};
    if (!oob) {
        for (int h = 0; h < 8; h++) {            // itertools.product order: the last axis varies fastest
            int b0 = (h >> 2) & 1, b1 = (h >> 1) & 1, b2 = h & 1;
            double wt = 1.0;
            wt = wt * (b0 ? y[0] : 1.0 - y[0]);
            wt = wt * (b1 ? y[1] : 1.0 - y[1]);
            wt = wt * (b2 ? y[2] : 1.0 - y[2]);
            long long e = ((long long)(idx[0] + b0) * Y + (idx[1] + b1)) * Z + (idx[2] + b2);
            for (int c = 0; c < 3; c++) v[c] = v[c] + (double)g[c * per + e] * wt;
        }
    }
    for (int c = 0; c < 3; c++) s3[c] = x[c] + v[c] * mag;
}

// pc.py:crop :40-42 for one point: all(s + off >= 0) and all(s + off < range)
__device__ __forceinline__ int sp_crop_keep(const double *__restrict__ s3, const double *off, const double *rng) {
    bool lo = true, hi = true;
    for (int d = 0; d < 3; d++) {
        double v = s3[d] + off[d];
        lo = lo && v >= 0.0;
        hi = hi && v < rng[d];
    }
    return (lo && hi) ? 1 : 0;
}

// `_croppedInstanceIds` on the id-presence table, by ONE thread: `while j < ids.max(): if j absent: ids[ids == ids.max()] = j; j += 1`
__device__ __forceinline__ void sp_relabel_walk(const int *__restrict__ pres, int V, int *__restrict__ val_of, int *__restrict__ orig_at) {
    int cur = -1;
    for (int v = 0; v < V; v++) {
        val_of[v] = v;
        orig_at[v] = pres[v] ? v : -1;
        if (pres[v]) cur = v;
    }
    for (int j = 0; j < cur; j++) {
        if (orig_at[j] != -1) continue;
        int o = orig_at[cur];
        orig_at[j] = o;
        val_of[o] = j;
        orig_at[cur] = -1;
        while (cur > j && orig_at[cur] == -1) cur--;
    }
}

// ---- the batch outputs (batch_prep.hip, batch_elastic.hip) and the box-label rows both write into them ---------------------------
struct BpOut {                        // scene_prep._POINT_KEYS, batch_offsets, instance_offsets, scene_prep._BOX_KEYS
    float *locs; long long *locs_scaled; float *feats; long long *sem, *ids; float *info; int *num_point, *gt_idx, *gt_off;
    int *boff, *ioff;
    float *center; long long *sem_cls, *head_cls; float *head_res; long long *size_cls; float *size_res;
    long long *obj_id, *label; float *bbox;
};

// row k of slot `slot`: the heading labels (always zero) and, where no instance owns the row, zeros in the other seven labels;
// K instances, sh = 1 without unlabelled points (then the first instance takes row R - 1)
__device__ __forceinline__ void bp_unowned_rows(const BpOut &o, int slot, int R, int K, int sh, int k) {
    const int kmax = K - 1 - sh;
    if (k < R) {
        const long long row = (long long)slot * R + k;
        const bool owned = (k < 128 && k <= kmax) || (sh == 1 && K >= 1 && k == R - 1);
        o.head_cls[row] = 0;
        o.head_res[row] = 0.0f;
        if (!owned) {
            for (int d = 0; d < 3; d++) { o.center[3 * row + d] = 0.0f; o.size_res[3 * row + d] = 0.0f; }
            o.sem_cls[row] = 0; o.size_cls[row] = 0; o.obj_id[row] = 0; o.label[row] = 0;
            float4 *bb = (float4 *)(o.bbox + 24 * row);       // 96-byte rows from a 16-byte aligned base
            for (int q = 0; q < 6; q++) bb[q] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        }
    }
}

// the box-label row of the instance with id value v, semantic label `sem` of its first point and exact extent mn / mx
template <typename T>
__device__ __forceinline__ void bp_box_row(const BpOut &o, long long row, int sem, int v, const T *mn, const T *mx,
                                           const double *__restrict__ mean_size) {
    int c = sem;
    c = c >= 2 ? c - 2 : 17;
    double ctr[3], size[3];
    for (int d = 0; d < 3; d++) {
        ctr[d] = (double)((mn[d] + mx[d]) / (T)2);
        size[d] = (double)(mx[d] - mn[d]);
        o.center[3 * row + d] = (float)ctr[d];
        o.size_res[3 * row + d] = (float)(size[d] - mean_size[3 * c + d]);
    }
    o.sem_cls[row] = c; o.size_cls[row] = c; o.obj_id[row] = v; o.label[row] = 1;
    // get_3d_box_batch with heading 0: corners = center + (+-l/2, +-w/2, +-h/2)
    const int sx[8] = {1, 1, -1, -1, 1, 1, -1, -1}, sy[8] = {1, -1, -1, 1, 1, -1, -1, 1}, sz[8] = {1, 1, 1, 1, -1, -1, -1, -1};
    float *bb = o.bbox + 24 * row;
    for (int q = 0; q < 8; q++) {
        bb[3 * q] = (float)(sx[q] * (size[0] / 2) + ctr[0]);
        bb[3 * q + 1] = (float)(sy[q] * (size[1] / 2) + ctr[1]);
        bb[3 * q + 2] = (float)(sz[q] * (size[2] / 2) + ctr[2]);
    }
}
