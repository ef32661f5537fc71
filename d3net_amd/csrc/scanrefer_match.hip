// scanrefer_match.hip -- the ScanRefer match module (model/match_module.py:11-141) of the listener, fused (gfx950).
//
// The reference repeats the proposal features and the language embedding to (N, K, m+L), concatenates, masks, and runs
//     fuse  = Conv1d(m+L -> 128), BatchNorm1d, PReLU(128), Conv1d(128 -> 128)
//     match = Conv1d, ReLU, BatchNorm1d, Conv1d, ReLU, BatchNorm1d, Conv1d(128 -> 1)
// as seven library calls with three training-mode BatchNorms between them.  Here, with R = N K positions (rows):
//
//   * the first convolution is split: W0 = [W_det | W_lang], P = feats W_det^T (B K rows), Q = lang W_lang^T (N rows) -- two
//     problems of one hgemm call through strided views of W0 -- and  h1[n,k,:] = mask[b,k] (P[b,k,:] + Q[n,:]) + b0,  b = n / div
//     (div = descriptions per scene, or sampled captions per scene in the RL branch where mask == 1).  h1 is one add per element and
//     is recomputed wherever it is needed: neither the concatenation nor the per-description copies of the proposal rows exist;
//   * the rest is cut only where a training-mode BatchNorm needs statistics over ALL rows (no grid-wide barrier):
//       sm_stats1_kernel   per-channel sum / sum of squares of h1
//       sm_fwd_kernel [A]  BN1 + PReLU -> fuse.3 -> match.0 -> ReLU, store, BN2 partial sums   (two 128 x 128 products back to back)
//       sm_fwd_kernel [B]  BN2 -> match.3 -> ReLU, store, BN3 partial sums
//       sm_fwd_kernel [C]  BN3 -> the 128 -> 1 product -> confidences
//     in eval() the running statistics are known up front and [A][B][C] run as ONE launch;
//   * every producer writes per-workgroup partial sums (double) and every consumer adds them in workgroup order in its
//     prologue: no floating-point atomics, two runs are bit-identical.  Workgroup 0 of the consumer also applies the
//     momentum update of the running statistics (unbiased variance), counts the batch and keeps mean / rstd for the backward;
//   * the backward mirrors the cuts (sm_bwd3_sums / sm_bwd3 / sm_bwd2 / sm_bwd1 kernels below); weight and bias gradients are hgemm /
//     colsum problems over the activations the forward saved.
// A workgroup (4 waves) owns 64 rows: the 64 x 128 activation tile and ONE 128 x 128 weight live in LDS (pitch 132 floats:
// 33 KB + 66 KB), every wave multiplies its 16 rows by the whole weight on v_mfma_f32_16x16x4_f32 (exact fp32, as hgemm.hip):
// 8 accumulator tiles = 32 VGPRs.  The second weight of stage [A] replaces the first in LDS between the two products.
// Roofline: at N = 32, K = 128 the whole module is 0.4 GFLOP and ~10 MB of traffic per pass: launch / latency bound.
#include "common.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

#define SM_H 128          // hidden width (the only one the kernels are written for)
#define SM_TR 64          // rows per workgroup
#define SM_LP 132         // LDS row pitch in floats: 16-byte aligned rows, the 16 lanes of a k quad on distinct banks

struct SmShared {
    float X[SM_TR * SM_LP];
    float W[SM_H * SM_LP];
    double red[3][SM_H];
    float sc[SM_H], sh[SM_H], c0[SM_H], c1[SM_H], c2[SM_H];
};

// h1 of (row, channel c): mask (P + Q) + b0; P row = scene b's proposal k, Q row = description n
__device__ __forceinline__ float sm_h1(const d3_srm_args &a, int row, int c) {
    const int n = row / a.K, k = row - n * a.K, b = n / a.div;
    const long long pr = (long long)b * a.K + k;
    const float mk = a.mask ? a.mask[pr] : 1.f;
    return mk * (a.PQ[pr * SM_H + c] + a.PQ[((long long)a.B * a.K + n) * SM_H + c]) + a.b0[c];
}

// W (128 out, 128 in) row-major -> S.W[n][k] = W[n][k], or (transpose) S.W[n][k] = W[k][n]
__device__ __forceinline__ void sm_load_w(SmShared &S, const float *__restrict__ W, bool transpose) {
    const int t = threadIdx.x;
    if (!transpose) {
        for (int e = t; e < SM_H * 32; e += 256) {
            const int r = e >> 5, c4 = (e & 31) * 4;
            *(f32x4 *)&S.W[r * SM_LP + c4] = *(const f32x4 *)(W + r * SM_H + c4);
        }
    } else {
        for (int e = t; e < SM_H * 32; e += 256) {
            const int n = e & 127, k4 = (e >> 7) * 4;
            f32x4 v;
#pragma unroll
            for (int s = 0; s < 4; s++) v[s] = W[(k4 + s) * SM_H + n];
            *(f32x4 *)&S.W[n * SM_LP + k4] = v;
        }
    }
}

// acc[ct][q] = sum_k X[wave*16 + g*4 + q][k] . S.W[ct*16 + i][k]
__device__ __forceinline__ void sm_gemm(const SmShared &S, f32x4 acc[8]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 15, g = lane >> 4;
#pragma unroll
    for (int ct = 0; ct < 8; ct++) acc[ct] = (f32x4){0.f, 0.f, 0.f, 0.f};
    for (int kb = 0; kb < 8; kb++) {
        const f32x4 av = *(const f32x4 *)&S.X[(wave * 16 + i) * SM_LP + kb * 16 + g * 4];
#pragma unroll
        for (int ct = 0; ct < 8; ct++) {
            const f32x4 bv = *(const f32x4 *)&S.W[(ct * 16 + i) * SM_LP + kb * 16 + g * 4];
#pragma unroll
            for (int q = 0; q < 4; q++) acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[q], bv[q], acc[ct], 0, 0, 0);
        }
    }
}

// the wave's finished 16 x 128 tile (+ bias, ReLU) back into its own rows of S.X and, when out != NULL, to global rows r0 + ...
__device__ __forceinline__ void sm_put(SmShared &S, const f32x4 acc[8], const float *bias, bool relu, float *out, int r0, int R) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 15, g = lane >> 4;
#pragma unroll
    for (int ct = 0; ct < 8; ct++) {
        const int c = ct * 16 + i;
        const float bv = bias ? bias[c] : 0.f;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int r = wave * 16 + g * 4 + q;
            float v = acc[ct][q] + bv;
            if (relu && v < 0.f) v = 0.f;
            S.X[r * SM_LP + c] = v;
            if (out && r0 + r < R) out[(long long)(r0 + r) * SM_H + c] = v;
        }
    }
}

// S.X <- rows r0 .. r0+63 of src (R, 128); rows beyond R are zero
__device__ __forceinline__ void sm_load_x(SmShared &S, const float *__restrict__ src, int r0, int R) {
    for (int e = threadIdx.x; e < SM_TR * 32; e += 256) {
        const int r = e >> 5, c4 = (e & 31) * 4;
        f32x4 v = (f32x4){0.f, 0.f, 0.f, 0.f};
        if (r0 + r < R) v = *(const f32x4 *)(src + (long long)(r0 + r) * SM_H + c4);
        *(f32x4 *)&S.X[r * SM_LP + c4] = v;
    }
}

// per-channel sum and sum of squares of the valid rows of S.X -> part (2, 128) of this workgroup.  Caller syncs before.
__device__ __forceinline__ void sm_tile_stats(SmShared &S, int nvalid, double *part) {
    const int c = threadIdx.x & 127, half = threadIdx.x >> 7;
    double s = 0.0, ss = 0.0;
    const int rend = min(nvalid, half * 32 + 32);
    for (int r = half * 32; r < rend; r++) { const double v = (double)S.X[r * SM_LP + c]; s += v; ss += v * v; }
    if (half) { S.red[0][c] = s; S.red[1][c] = ss; }
    __syncthreads();
    if (!half) { part[c] = s + S.red[0][c]; part[SM_H + c] = ss + S.red[1][c]; }
    __syncthreads();
}

// BatchNorm j: S.sc / S.sh such that bn(x) = sc x + sh.  train: batch statistics from the producers' partial sums (G workgroups,
// added in workgroup order); workgroup 0 applies the running update and keeps mean / rstd.  eval: running statistics.
__device__ __forceinline__ void sm_bn_coef(SmShared &S, const d3_srm_args &a, int j, int train, int G, int R) {
    const int t = threadIdx.x;
    __syncthreads();
    if (t < SM_H) {
        const float *gamma = j == 0 ? a.g1 : (j == 1 ? a.g2 : a.g3), *beta = j == 0 ? a.be1 : (j == 1 ? a.be2 : a.be3);
        float *rm = j == 0 ? a.rm1 : (j == 1 ? a.rm2 : a.rm3), *rv = j == 0 ? a.rv1 : (j == 1 ? a.rv2 : a.rv3);
        const bool writer = blockIdx.x == 0;
        float mean, rstd;
        if (train) {
            const double *part = a.part + (size_t)j * G * 2 * SM_H;
            double s = 0.0, ss = 0.0;
            for (int w = 0; w < G; w++) { s += part[(size_t)w * 2 * SM_H + t]; ss += part[(size_t)w * 2 * SM_H + SM_H + t]; }
            const double mu = s / (double)R;
            double var = ss / (double)R - mu * mu;
            if (var < 0.0) var = 0.0;
            mean = (float)mu;
            rstd = (float)(1.0 / sqrt(var + (double)a.eps[j]));
            if (writer) {
                const float mom = a.momentum[j];
                rm[t] = (1.f - mom) * rm[t] + mom * mean;
                rv[t] = (1.f - mom) * rv[t] + mom * (float)(var * (double)R / (double)(R - 1));
                if (t == 0 && a.nbt[j]) *a.nbt[j] += 1;
            }
        } else {
            mean = rm[t];
            rstd = (float)(1.0 / sqrt((double)rv[t] + (double)a.eps[j]));
        }
        if (writer && a.bnstat) { a.bnstat[j * 2 * SM_H + t] = mean; a.bnstat[j * 2 * SM_H + SM_H + t] = rstd; }
        const float sc = gamma[t] * rstd;
        S.sc[t] = sc;
        S.sh[t] = beta[t] - mean * sc;
    }
    __syncthreads();
}

// ------------------------------------------------------------------------------------------------ forward
__global__ __launch_bounds__(256) void sm_stats1_kernel(const d3_srm_args a) {
    __shared__ double red[2][SM_H];
    const int R = a.N * a.K, r0 = blockIdx.x * SM_TR, c = threadIdx.x & 127, half = threadIdx.x >> 7;
    double s = 0.0, ss = 0.0;
    const int rend = min(R, r0 + half * 32 + 32);
    for (int row = r0 + half * 32; row < rend; row++) { const double v = (double)sm_h1(a, row, c); s += v; ss += v * v; }
    if (half) { red[0][c] = s; red[1][c] = ss; }
    __syncthreads();
    if (!half) {
        double *part = a.part + (size_t)blockIdx.x * 2 * SM_H;
        part[c] = s + red[0][c];
        part[SM_H + c] = ss + red[1][c];
    }
}

// stages s0 .. s1 of {0: [A], 1: [B], 2: [C]} on this workgroup's 64 rows
__global__ __launch_bounds__(256) void sm_fwd_kernel(const d3_srm_args a, int s0, int s1, int train) {
    __shared__ __attribute__((aligned(16))) SmShared S;
    const int t = threadIdx.x, R = a.N * a.K, G = gridDim.x, r0 = blockIdx.x * SM_TR;
    const int nvalid = min(SM_TR, R - r0);
    f32x4 acc[8];
    if (s0 <= 0) {
        sm_bn_coef(S, a, 0, train, G, R);
        for (int e = t; e < SM_TR * 32; e += 256) {
            const int r = e >> 5, c4 = (e & 31) * 4, row = r0 + r;
            f32x4 v = (f32x4){0.f, 0.f, 0.f, 0.f};
            if (row < R) {
#pragma unroll
                for (int s = 0; s < 4; s++) {
                    const float u = S.sc[c4 + s] * sm_h1(a, row, c4 + s) + S.sh[c4 + s];
                    v[s] = u > 0.f ? u : a.alpha[c4 + s] * u;
                }
                if (a.x1) *(f32x4 *)(a.x1 + (long long)row * SM_H + c4) = v;
            }
            *(f32x4 *)&S.X[r * SM_LP + c4] = v;
        }
        sm_load_w(S, a.W3, false);
        __syncthreads();
        sm_gemm(S, acc);
        sm_put(S, acc, a.b3, false, a.f, r0, R);
        __syncthreads();
        sm_load_w(S, a.W4, false);
        __syncthreads();
        sm_gemm(S, acc);
        sm_put(S, acc, a.b4, true, (s1 == 0 || a.x1) ? a.y2 : nullptr, r0, R);
        __syncthreads();
        if (train) sm_tile_stats(S, nvalid, a.part + ((size_t)1 * G + blockIdx.x) * 2 * SM_H);
    }
    if (s0 <= 1 && s1 >= 1) {
        if (s0 == 1) sm_load_x(S, a.y2, r0, R);
        sm_bn_coef(S, a, 1, train, G, R);
        for (int e = t; e < SM_TR * 32; e += 256) {
            const int r = e >> 5, c4 = (e & 31) * 4, row = r0 + r;
            f32x4 v = *(const f32x4 *)&S.X[r * SM_LP + c4];
#pragma unroll
            for (int s = 0; s < 4; s++) v[s] = S.sc[c4 + s] * v[s] + S.sh[c4 + s];
            *(f32x4 *)&S.X[r * SM_LP + c4] = v;
            if (a.z2 && row < R) *(f32x4 *)(a.z2 + (long long)row * SM_H + c4) = v;
        }
        sm_load_w(S, a.W5, false);
        __syncthreads();
        sm_gemm(S, acc);
        sm_put(S, acc, a.b5, true, (s1 == 1 || a.x1) ? a.y3 : nullptr, r0, R);
        __syncthreads();
        if (train) sm_tile_stats(S, nvalid, a.part + ((size_t)2 * G + blockIdx.x) * 2 * SM_H);
    }
    if (s1 >= 2) {
        if (s0 == 2) sm_load_x(S, a.y3, r0, R);
        sm_bn_coef(S, a, 2, train, G, R);
        const int r = t >> 2, qd = t & 3;
        float v = 0.f;
        for (int c = qd * 32; c < qd * 32 + 32; c++) v += a.w6[c] * (S.sc[c] * S.X[r * SM_LP + c] + S.sh[c]);
        v += __shfl_xor(v, 1);
        v += __shfl_xor(v, 2);
        if (qd == 0 && r0 + r < R) a.conf[r0 + r] = v + a.b6[0];
    }
}

// ----------------------------------------------------------------------------------------------- backward
// partial sums of the backward: gpart (4, G, 3, 128) doubles; slot j is written by the kernel before its consumer
__device__ __forceinline__ void sm_reduce3(SmShared &S, const double *part, int G, double out[3]) {
    const int t = threadIdx.x;
    out[0] = out[1] = out[2] = 0.0;
    if (t < SM_H)
        for (int w = 0; w < G; w++)
#pragma unroll
            for (int q = 0; q < 3; q++) out[q] += part[((size_t)w * 3 + q) * SM_H + t];
}

// three per-channel sums over this workgroup's valid rows, halves combined in fixed order
__device__ __forceinline__ void sm_write3(SmShared &S, double s0, double s1, double s2, double *part) {
    const int c = threadIdx.x & 127, half = threadIdx.x >> 7;
    if (half) { S.red[0][c] = s0; S.red[1][c] = s1; S.red[2][c] = s2; }
    __syncthreads();
    if (!half) { part[c] = s0 + S.red[0][c]; part[SM_H + c] = s1 + S.red[1][c]; part[2 * SM_H + c] = s2 + S.red[2][c]; }
    __syncthreads();
}

// [bwd3a] sums for BatchNorm 3's backward: dz3[r,c] = dconf[r] w6[c], so S0 = sum_r dconf, S1[c] = sum_r dconf xhat3[r,c]
__global__ __launch_bounds__(256) void sm_bwd3_sums_kernel(const d3_srm_args a, const d3_srm_grads gr) {
    __shared__ double red[2][SM_H];
    const int R = a.N * a.K, r0 = blockIdx.x * SM_TR, c = threadIdx.x & 127, half = threadIdx.x >> 7;
    const float mean = a.bnstat[4 * SM_H + c], rstd = a.bnstat[5 * SM_H + c];
    double s = 0.0, sx = 0.0;
    const int rend = min(R, r0 + half * 32 + 32);
    for (int row = r0 + half * 32; row < rend; row++) {
        const float d = gr.dconf[row], xh = (a.y3[(long long)row * SM_H + c] - mean) * rstd;
        s += (double)d;
        sx += (double)(d * xh);
    }
    if (half) { red[0][c] = s; red[1][c] = sx; }
    __syncthreads();
    if (!half) {
        double *part = gr.part + (size_t)blockIdx.x * 3 * SM_H;
        part[c] = s + red[0][c];
        part[SM_H + c] = sx + red[1][c];
        part[2 * SM_H + c] = 0.0;
    }
}

// [bwd3b] BN3 backward + ReLU' -> dpre3 (stored) -> . W5 -> dz2 (stored) + sums for BN2's backward
__global__ __launch_bounds__(256) void sm_bwd3_kernel(const d3_srm_args a, const d3_srm_grads gr, int train) {
    __shared__ __attribute__((aligned(16))) SmShared S;
    const int t = threadIdx.x, R = a.N * a.K, G = gridDim.x, r0 = blockIdx.x * SM_TR;
    double sum[3];
    sm_reduce3(S, gr.part, G, sum);
    if (t < SM_H) {
        const float mean = a.bnstat[4 * SM_H + t], rstd = a.bnstat[5 * SM_H + t], w = a.w6[t];
        const float S0 = (float)sum[0], S1 = (float)sum[1];
        const float a3 = a.g3[t] * rstd;
        S.sc[t] = mean; S.sh[t] = rstd;
        S.c0[t] = a3 * w;
        S.c1[t] = train ? a3 * (w * S0 / (float)R) : 0.f;
        S.c2[t] = train ? a3 * (w * S1 / (float)R) : 0.f;
        if (blockIdx.x == 0) {
            gr.dg3[t] = w * S1;
            gr.dbe3[t] = w * S0;
            gr.dw6[t] = a.g3[t] * S1 + a.be3[t] * S0;
            if (t == 0) gr.db6[0] = S0;
        }
    }
    __syncthreads();
    for (int e = t; e < SM_TR * 32; e += 256) {
        const int r = e >> 5, c4 = (e & 31) * 4, row = r0 + r;
        f32x4 v = (f32x4){0.f, 0.f, 0.f, 0.f};
        if (row < R) {
            const f32x4 y = *(const f32x4 *)(a.y3 + (long long)row * SM_H + c4);
            const float d = gr.dconf[row];
#pragma unroll
            for (int s = 0; s < 4; s++) {
                const int c = c4 + s;
                const float xh = (y[s] - S.sc[c]) * S.sh[c];
                v[s] = y[s] > 0.f ? S.c0[c] * d - S.c1[c] - xh * S.c2[c] : 0.f;
            }
            *(f32x4 *)(gr.dpre3 + (long long)row * SM_H + c4) = v;
        }
        *(f32x4 *)&S.X[r * SM_LP + c4] = v;
    }
    sm_load_w(S, a.W5, true);
    __syncthreads();
    f32x4 acc[8];
    sm_gemm(S, acc);
    sm_put(S, acc, nullptr, false, gr.dz2, r0, R);
    __syncthreads();
    {
        const int c = t & 127, half = t >> 7;
        const float mean = a.bnstat[2 * SM_H + c], rstd = a.bnstat[3 * SM_H + c];
        double s = 0.0, sx = 0.0;
        const int rend = min(R - r0, half * 32 + 32);
        for (int r = half * 32; r < rend; r++) {
            const float d = S.X[r * SM_LP + c], xh = (a.y2[(long long)(r0 + r) * SM_H + c] - mean) * rstd;
            s += (double)d;
            sx += (double)(d * xh);
        }
        sm_write3(S, s, sx, 0.0, gr.part + ((size_t)1 * G + blockIdx.x) * 3 * SM_H);
    }
}

// [bwd2] BN2 backward + ReLU' -> dpre2 (stored) -> . W4 -> df (stored) -> . W3 -> dx1 -> PReLU' -> dbn1 (stored) + sums for BN1 / PReLU
__global__ __launch_bounds__(256) void sm_bwd2_kernel(const d3_srm_args a, const d3_srm_grads gr, int train) {
    __shared__ __attribute__((aligned(16))) SmShared S;
    const int t = threadIdx.x, R = a.N * a.K, G = gridDim.x, r0 = blockIdx.x * SM_TR;
    double sum[3];
    sm_reduce3(S, gr.part + (size_t)1 * G * 3 * SM_H, G, sum);
    if (t < SM_H) {
        const float mean = a.bnstat[2 * SM_H + t], rstd = a.bnstat[3 * SM_H + t];
        const float S0 = (float)sum[0], S1 = (float)sum[1];
        const float a2 = a.g2[t] * rstd;
        S.sc[t] = mean; S.sh[t] = rstd;
        S.c0[t] = a2;
        S.c1[t] = train ? a2 * (S0 / (float)R) : 0.f;
        S.c2[t] = train ? a2 * (S1 / (float)R) : 0.f;
        if (blockIdx.x == 0) { gr.dg2[t] = S1; gr.dbe2[t] = S0; }
    }
    __syncthreads();
    for (int e = t; e < SM_TR * 32; e += 256) {
        const int r = e >> 5, c4 = (e & 31) * 4, row = r0 + r;
        f32x4 v = (f32x4){0.f, 0.f, 0.f, 0.f};
        if (row < R) {
            const f32x4 y = *(const f32x4 *)(a.y2 + (long long)row * SM_H + c4);
            const f32x4 d = *(const f32x4 *)(gr.dz2 + (long long)row * SM_H + c4);
#pragma unroll
            for (int s = 0; s < 4; s++) {
                const int c = c4 + s;
                const float xh = (y[s] - S.sc[c]) * S.sh[c];
                v[s] = y[s] > 0.f ? S.c0[c] * d[s] - S.c1[c] - xh * S.c2[c] : 0.f;
            }
            *(f32x4 *)(gr.dpre2 + (long long)row * SM_H + c4) = v;
        }
        *(f32x4 *)&S.X[r * SM_LP + c4] = v;
    }
    sm_load_w(S, a.W4, true);
    __syncthreads();
    f32x4 acc[8];
    sm_gemm(S, acc);
    sm_put(S, acc, nullptr, false, gr.df, r0, R);
    __syncthreads();
    sm_load_w(S, a.W3, true);
    __syncthreads();
    sm_gemm(S, acc);
    sm_put(S, acc, nullptr, false, nullptr, r0, R);
    __syncthreads();
    {
        const int c = t & 127, half = t >> 7;
        const float mean = a.bnstat[c], rstd = a.bnstat[SM_H + c];
        const float sc = a.g1[c] * rstd, sh = a.be1[c] - mean * sc, al = a.alpha[c];
        double s = 0.0, sx = 0.0, sa = 0.0;
        const int rend = min(R - r0, half * 32 + 32);
        for (int r = half * 32; r < rend; r++) {
            const float h = sm_h1(a, r0 + r, c), u = sc * h + sh, d = S.X[r * SM_LP + c];
            const float db = u > 0.f ? d : al * d;
            gr.dbn1[(long long)(r0 + r) * SM_H + c] = db;
            s += (double)db;
            sx += (double)(db * ((h - mean) * rstd));
            if (!(u > 0.f)) sa += (double)(d * u);
        }
        sm_write3(S, s, sx, sa, gr.part + ((size_t)2 * G + blockIdx.x) * 3 * SM_H);
    }
}

// [bwd1] BN1 backward -> dh1, reduced to dQ[n] = sum_k mask dh1 (workgroups 0 .. N-1, which also keep the unmasked row sums
// for fuse.0.bias) and dP[b,k] = mask sum_{n in scene b} dh1 (the workgroups after them, 16 proposals each)
__global__ __launch_bounds__(256) void sm_bwd1_kernel(const d3_srm_args a, const d3_srm_grads gr, int train, int G) {
    __shared__ float fr[2][SM_H];
    const int t = threadIdx.x, R = a.N * a.K, c = t & 127, half = t >> 7;
    double sum[3] = {0.0, 0.0, 0.0};
    for (int w = 0; w < G; w++)
#pragma unroll
        for (int q = 0; q < 3; q++) sum[q] += gr.part[(((size_t)2 * G + w) * 3 + q) * SM_H + c];
    const float mean = a.bnstat[c], rstd = a.bnstat[SM_H + c];
    const float a1 = a.g1[c] * rstd;
    const float m0 = train ? a1 * ((float)sum[0] / (float)R) : 0.f, m1 = train ? a1 * ((float)sum[1] / (float)R) : 0.f;
    if (blockIdx.x == 0 && !half) { gr.dg1[c] = (float)sum[1]; gr.dbe1[c] = (float)sum[0]; gr.dalpha[c] = (float)sum[2]; }
    if ((int)blockIdx.x < a.N) {
        const int n = blockIdx.x, b = n / a.div;
        const int kh = (a.K + 1) / 2, k0 = half * kh, k1 = min(a.K, k0 + kh);
        float sm = 0.f, sall = 0.f;
        for (int k = k0; k < k1; k++) {
            const int row = n * a.K + k;
            const float xh = (sm_h1(a, row, c) - mean) * rstd;
            const float dh = a1 * gr.dbn1[(long long)row * SM_H + c] - m0 - xh * m1;
            const float mk = a.mask ? a.mask[(long long)b * a.K + k] : 1.f;
            sm += mk * dh;
            sall += dh;
        }
        if (half) { fr[0][c] = sm; fr[1][c] = sall; }
        __syncthreads();
        if (!half) {
            gr.dQ[(long long)n * SM_H + c] = sm + fr[0][c];
            gr.db0part[(long long)n * SM_H + c] = sall + fr[1][c];
        }
    } else {
        const int idx = blockIdx.x - a.N, KT = (a.K + 15) / 16, b = idx / KT, kt = idx - b * KT;
        for (int kk = half * 8; kk < half * 8 + 8; kk++) {
            const int k = kt * 16 + kk;
            if (k >= a.K) break;
            float s = 0.f;
            for (int j = 0; j < a.div; j++) {
                const int row = (b * a.div + j) * a.K + k;
                const float xh = (sm_h1(a, row, c) - mean) * rstd;
                s += a1 * gr.dbn1[(long long)row * SM_H + c] - m0 - xh * m1;
            }
            const float mk = a.mask ? a.mask[(long long)b * a.K + k] : 1.f;
            gr.dP[((long long)b * a.K + k) * SM_H + c] = mk * s;
        }
    }
}

// ------------------------------------------------------------------------------------------------- host
static int sm_check(const d3_srm_args *a) {
    if (!a || a->B < 1 || a->K < 1 || a->N < 1 || a->div < 1 || a->N != a->B * a->div || a->m < 4 || (a->m & 3) || a->L < 1) return D3_ERR_ARG;
    if ((long long)a->N * a->K > (1 << 24)) return D3_ERR_RANGE;      // rows are counted in int and in float
    if (!a->feats || !a->lang || !a->W0 || !a->b0 || !a->g1 || !a->be1 || !a->rm1 || !a->rv1 || !a->alpha || !a->W3 || !a->b3 || !a->W4 ||
        !a->b4 || !a->g2 || !a->be2 || !a->rm2 || !a->rv2 || !a->W5 || !a->b5 || !a->g3 || !a->be3 || !a->rm3 || !a->rv3 || !a->w6 || !a->b6 ||
        !a->PQ || !a->part || !a->conf) return D3_ERR_ARG;
    return 0;
}

static d3_gemm_prob sm_prob(const float *A, long long lda, int akm, const float *Bm, long long ldb, int bkm, int Kd, int M, int N, float *Cm,
                            long long ldc) {
    d3_gemm_prob p = {};
    p.seg[0].A = A; p.seg[0].lda = lda; p.seg[0].a_kmajor = akm;
    p.seg[0].B = Bm; p.seg[0].ldb = ldb; p.seg[0].b_kmajor = bkm;
    p.seg[0].K = Kd;
    p.nseg = 1; p.M = M; p.N = N; p.C = Cm; p.ldc = ldc;
    return p;
}

extern "C" int d3_scanrefer_match_groups(int N, int K) { return (int)(((long long)N * K + SM_TR - 1) / SM_TR); }

extern "C" int d3_scanrefer_match_fwd(const d3_srm_args *a, int train, void *stream) {
    D3_CLEAR();
    int rc = sm_check(a);
    if (rc) return rc;
    const int R = a->N * a->K, G = d3_scanrefer_match_groups(a->N, a->K);
    if (train && R < 2) return D3_ERR_ARG;
    if (train && (!a->y2 || !a->y3)) return D3_ERR_ARG;
    if (a->x1 && (!a->f || !a->y2 || !a->z2 || !a->y3 || !a->bnstat)) return D3_ERR_ARG;
    hipStream_t s = d3_stream(stream);
    const long long ld0 = a->m + a->L;
    d3_gemm_prob pq[2];
    pq[0] = sm_prob(a->feats, a->m, 0, a->W0, ld0, 0, a->m, a->B * a->K, SM_H, a->PQ, SM_H);
    pq[1] = sm_prob(a->lang, a->L, 0, a->W0 + a->m, ld0, 0, a->L, a->N, SM_H, a->PQ + (long long)a->B * a->K * SM_H, SM_H);
    if ((rc = hg_launch(pq, 2, s))) return rc;
    if (train) {
        sm_stats1_kernel<<<G, 256, 0, s>>>(*a);
        sm_fwd_kernel<<<G, 256, 0, s>>>(*a, 0, 0, 1);
        sm_fwd_kernel<<<G, 256, 0, s>>>(*a, 1, 1, 1);
        sm_fwd_kernel<<<G, 256, 0, s>>>(*a, 2, 2, 1);
    } else {
        sm_fwd_kernel<<<G, 256, 0, s>>>(*a, 0, 2, 0);
    }
    D3_LAUNCH_CHECK();
    return 0;
}

extern "C" size_t d3_scanrefer_match_bwd_ws_bytes(void) { return hg_colsum_ws_bytes(4, 128); }

extern "C" int d3_scanrefer_match_bwd(const d3_srm_args *a, const d3_srm_grads *g, int train, void *stream) {
    D3_CLEAR();
    int rc = sm_check(a);
    if (rc) return rc;
    if (!a->x1 || !a->f || !a->y2 || !a->z2 || !a->y3 || !a->bnstat) return D3_ERR_ARG;
    if (!g || !g->dconf || !g->dW0 || !g->db0 || !g->dg1 || !g->dbe1 || !g->dalpha || !g->dW3 || !g->db3 || !g->dW4 || !g->db4 || !g->dg2 ||
        !g->dbe2 || !g->dW5 || !g->db5 || !g->dg3 || !g->dbe3 || !g->dw6 || !g->db6 || !g->dpre3 || !g->dz2 || !g->dpre2 || !g->df ||
        !g->dbn1 || !g->dP || !g->dQ || !g->db0part || !g->part || !g->ws) return D3_ERR_ARG;
    if (g->ws_bytes < d3_scanrefer_match_bwd_ws_bytes()) return D3_ERR_WORKSPACE;
    const int R = a->N * a->K, G = d3_scanrefer_match_groups(a->N, a->K), BK = a->B * a->K;
    hipStream_t s = d3_stream(stream);
    sm_bwd3_sums_kernel<<<G, 256, 0, s>>>(*a, *g);
    sm_bwd3_kernel<<<G, 256, 0, s>>>(*a, *g, train);
    sm_bwd2_kernel<<<G, 256, 0, s>>>(*a, *g, train);
    sm_bwd1_kernel<<<a->N + a->B * ((a->K + 15) / 16), 256, 0, s>>>(*a, *g, train, G);
    D3_LAUNCH_CHECK();
    // bias gradients: fixed-order column sums
    const float *cx[4] = {g->dpre3, g->dpre2, g->df, g->db0part};
    float *co[4] = {g->db5, g->db4, g->db3, g->db0};
    const long long cld[4] = {SM_H, SM_H, SM_H, SM_H};
    const int cR[4] = {R, R, R, a->N}, cC[4] = {SM_H, SM_H, SM_H, SM_H};
    if ((rc = hg_colsum_multi(cx, cld, cR, cC, co, nullptr, 4, g->ws, g->ws_bytes, s))) return rc;
    // weight gradients dW = dy^T x (both operands k-major) and the two input gradients
    const long long ld0 = a->m + a->L;
    d3_gemm_prob p[4];
    p[0] = sm_prob(g->dpre3, SM_H, 1, a->z2, SM_H, 1, R, SM_H, SM_H, g->dW5, SM_H);
    p[1] = sm_prob(g->dpre2, SM_H, 1, a->f, SM_H, 1, R, SM_H, SM_H, g->dW4, SM_H);
    p[2] = sm_prob(g->df, SM_H, 1, a->x1, SM_H, 1, R, SM_H, SM_H, g->dW3, SM_H);
    if ((rc = hg_launch(p, 3, s))) return rc;
    p[0] = sm_prob(g->dP, SM_H, 1, a->feats, a->m, 1, BK, SM_H, a->m, g->dW0, ld0);
    p[1] = sm_prob(g->dQ, SM_H, 1, a->lang, a->L, 1, a->N, SM_H, a->L, g->dW0 + a->m, ld0);
    int np = 2;
    if (g->dfeats) p[np++] = sm_prob(g->dP, SM_H, 0, a->W0, ld0, 1, SM_H, BK, a->m, g->dfeats, a->m);
    if (g->dlang) p[np++] = sm_prob(g->dQ, SM_H, 0, a->W0 + a->m, ld0, 1, SM_H, a->N, a->L, g->dlang, a->L);
    return hg_launch(p, np, s);
}
