// optim.hip -- Adam and SGD over every parameter tensor of a group in ONE launch (gfx950), beside the AdamW of
// heads.hip and with its table design: a device table of 4 pointers per tensor, `numel` per tensor and a block map of
// (tensor, chunk) pairs, one workgroup of 256 threads per pair, chunk = d3_adamw_chunk() = 4096 elements.  All loads of a
// chunk are issued before the arithmetic; plain fp32 vector loads and stores, no LDS, no atomics.
// The reference builds torch.optim.Adam / SGD by name (model/pipeline.py:738-757, model/pointgroup.py:372-384); the
// arithmetic below is the library's, operation by operation (the build runs with -ffp-contract=off).
// HBM bound: Adam 4 reads + 3 writes of 4 B per element; SGD 3 + 2 with a momentum buffer (2 + 2 on a tensor's first
// update, which only writes the buffer), 2 + 1 without momentum.
//
// Global gradient-norm clipping (torch.nn.utils.clip_grad_norm_, what Lightning's `gradient_clip_val` switches on for the
// reference) over the same table: grad_sumsq_kernel leaves one double per (tensor, chunk) block, grad_clip_finish_kernel
// sums them into the d3_clip_ctl record (include/d3hip.h), and the CTL instantiations of the update kernels read the record:
// skip -> every workgroup returns before its first store; otherwise the gradient is used as g * coef (one fp32 multiply,
// not contracted) and stays unclipped in memory.  Both reductions run in double in a fixed order, without atomics: the
// record is bit-identical from run to run.  One more read of the gradients (4 B per element), no write pass.
#include "common.h"

#define OPT_CHUNK 4096   // = d3_adamw_chunk(): the host builds ONE block map for all three optimizers
#define OPT_PER (OPT_CHUNK / 256)

// sum over the 256 threads of a workgroup in a fixed order: lanes by shuffles, the 4 waves through LDS; every thread
// receives the total
__device__ __forceinline__ double opt_block_sum(double a, double *lds) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) a += __shfl_down(a, o, D3_WAVE);
    if (d3_lane() == 0) lds[threadIdx.x >> 6] = a;
    __syncthreads();
    return ((lds[0] + lds[1]) + lds[2]) + lds[3];
}

// partials[block] = sum of g^2 over the block's chunk of the gradient (table column 1), in double: squares of fp32 values
// neither overflow nor underflow there.  Out-of-range lanes contribute 0.
__global__ __launch_bounds__(256) void grad_sumsq_kernel(const long long *__restrict__ ptrs, const int *__restrict__ numel,
                                                        const int2 *__restrict__ blocks, double *__restrict__ partials) {
    __shared__ double lds[4];
    const int2 bm = blocks[blockIdx.x];
    const float *g = (const float *)ptrs[bm.x * 4 + 1];
    const int n = numel[bm.x], base = bm.y * OPT_CHUNK;
    float gv[OPT_PER];
#pragma unroll
    for (int j = 0; j < OPT_PER; j++) {   // all loads first
        const int i = base + j * 256 + threadIdx.x;
        gv[j] = i < n ? g[i] : 0.f;
    }
    double acc = 0.0;
#pragma unroll
    for (int j = 0; j < OPT_PER; j++) {
        const double d = (double)gv[j];
        acc += d * d;
    }
    acc = opt_block_sum(acc, lds);
    if (threadIdx.x == 0) partials[blockIdx.x] = acc;
}

// one workgroup: total = sum of partials[0..n) (thread t takes t, t + 256, ... in order, then opt_block_sum), and the record
__global__ __launch_bounds__(256) void grad_clip_finish_kernel(const double *__restrict__ partials, int n, float max_norm,
                                                              d3_clip_ctl *ctl) {
    __shared__ double lds[4];
    double acc = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) acc += partials[i];
    acc = opt_block_sum(acc, lds);
    if (threadIdx.x == 0) {
        const float norm = (float)sqrt(acc);
        // torch.nn.utils.clip_grad_norm_: clamp(max_norm / (total_norm + 1e-6), max=1.0) in fp32; a NaN stays a NaN
        const float c = max_norm / (norm + 1e-6f);
        const int skip = isfinite(norm) ? 0 : 1;
        ctl->norm = norm;
        ctl->coef = c > 1.0f ? 1.0f : c;
        ctl->skip = skip;
        ctl->nskipped += skip;
    }
}

// torch.optim.Adam (amsgrad = False, maximize = False), L2 weight decay folded into the gradient:
//   g' = g + wd p;  m = m + (1 - b1)(g' - m);  v = b2 v + (1 - b2) g'^2;  p = p - (lr / bc1) (m / (sqrt(v) / sqrt(bc2) + eps))
// table columns: param, grad, exp_avg, exp_avg_sq.  CTL: g is g * coef of the record, or the launch does nothing (skip).
template <bool CTL>
__global__ __launch_bounds__(256) void adam_kernel(const long long *__restrict__ ptrs, const int *__restrict__ numel,
                                                  const int2 *__restrict__ blocks, float step_size, float beta2, float omb1,
                                                  float omb2, float eps, float wd, float bc2_sqrt,
                                                  const d3_clip_ctl *__restrict__ ctl) {
    float coef = 1.f;
    if (CTL) {
        if (ctl->skip & ctl->enforce) return;
        coef = ctl->coef;
    }
    const int2 bm = blocks[blockIdx.x];
    float *p = (float *)ptrs[bm.x * 4 + 0];
    const float *g = (const float *)ptrs[bm.x * 4 + 1];
    float *m = (float *)ptrs[bm.x * 4 + 2], *v = (float *)ptrs[bm.x * 4 + 3];
    const int n = numel[bm.x], base = bm.y * OPT_CHUNK;
    float pv[OPT_PER], gv[OPT_PER], mv[OPT_PER], vv[OPT_PER];
#pragma unroll
    for (int j = 0; j < OPT_PER; j++) {   // all loads first
        const int i = base + j * 256 + threadIdx.x;
        const bool ok = i < n;
        pv[j] = ok ? p[i] : 0.f; gv[j] = ok ? g[i] : 0.f; mv[j] = ok ? m[i] : 0.f; vv[j] = ok ? v[i] : 0.f;
    }
#pragma unroll
    for (int j = 0; j < OPT_PER; j++) {
        const int i = base + j * 256 + threadIdx.x;
        if (i < n) {
            const float gc = CTL ? gv[j] * coef : gv[j];
            const float gg = gc + wd * pv[j];
            const float mm = mv[j] + omb1 * (gg - mv[j]);
            const float v2 = beta2 * vv[j] + omb2 * gg * gg;
            const float denom = sqrtf(v2) / bc2_sqrt + eps;
            p[i] = pv[j] - step_size * (mm / denom);
            m[i] = mm; v[i] = v2;
        }
    }
}

// torch.optim.SGD (dampening = 0, nesterov = False, maximize = False):
//   g' = g + wd p;  MOM: buf = FIRST ? g' : mu buf + g';  p = p - lr (MOM ? buf : g')
// table columns: param, grad, momentum_buffer, unused.  FIRST never reads the buffer (the library clones g' into it).
// CTL: as for adam_kernel.
template <bool MOM, bool FIRST, bool CTL>
__global__ __launch_bounds__(256) void sgd_kernel(const long long *__restrict__ ptrs, const int *__restrict__ numel,
                                                 const int2 *__restrict__ blocks, float lr, float mu, float wd,
                                                 const d3_clip_ctl *__restrict__ ctl) {
    float coef = 1.f;
    if (CTL) {
        if (ctl->skip & ctl->enforce) return;
        coef = ctl->coef;
    }
    const int2 bm = blocks[blockIdx.x];
    float *p = (float *)ptrs[bm.x * 4 + 0];
    const float *g = (const float *)ptrs[bm.x * 4 + 1];
    float *buf = MOM ? (float *)ptrs[bm.x * 4 + 2] : nullptr;
    const int n = numel[bm.x], base = bm.y * OPT_CHUNK;
    float pv[OPT_PER], gv[OPT_PER], bv[OPT_PER];
#pragma unroll
    for (int j = 0; j < OPT_PER; j++) {   // all loads first
        const int i = base + j * 256 + threadIdx.x;
        const bool ok = i < n;
        pv[j] = ok ? p[i] : 0.f; gv[j] = ok ? g[i] : 0.f;
        if (MOM && !FIRST) bv[j] = ok ? buf[i] : 0.f;
    }
#pragma unroll
    for (int j = 0; j < OPT_PER; j++) {
        const int i = base + j * 256 + threadIdx.x;
        if (i < n) {
            const float gc = CTL ? gv[j] * coef : gv[j];
            float d = gc + wd * pv[j];
            if (MOM) {
                if (!FIRST) d = mu * bv[j] + d;
                buf[i] = d;
            }
            p[i] = pv[j] - lr * d;
        }
    }
}

extern "C" int d3_grad_sumsq(const long long *ptrs, const int *numel, const void *blocks, int nblocks, double *partials,
                             void *stream) {
    D3_CLEAR();
    if (nblocks <= 0) return 0;
    if (d3_adamw_chunk() != OPT_CHUNK || !partials) return D3_ERR_ARG;
    grad_sumsq_kernel<<<nblocks, 256, 0, d3_stream(stream)>>>(ptrs, numel, (const int2 *)blocks, partials);
    D3_LAUNCH_CHECK();
    return 0;
}

extern "C" int d3_grad_clip_finish(const double *partials, int n, double max_norm, void *ctl, void *stream) {
    D3_CLEAR();
    if (n < 0 || (n > 0 && !partials) || !ctl || !(max_norm > 0.0)) return D3_ERR_ARG;
    grad_clip_finish_kernel<<<1, 256, 0, d3_stream(stream)>>>(partials, n, (float)max_norm, (d3_clip_ctl *)ctl);
    D3_LAUNCH_CHECK();
    return 0;
}

template <bool CTL>
static int adam_launch(const long long *ptrs, const int *numel, const void *blocks, int nblocks, double lr, double beta1,
                       double beta2, double eps, double weight_decay, double bias_correction1, double bias_correction2_sqrt,
                       const void *ctl, void *stream) {
    D3_CLEAR();
    if (nblocks <= 0) return 0;
    if (d3_adamw_chunk() != OPT_CHUNK || (CTL && !ctl)) return D3_ERR_ARG;
    // scalars derived in double, as the library does before it narrows them
    adam_kernel<CTL><<<nblocks, 256, 0, d3_stream(stream)>>>(ptrs, numel, (const int2 *)blocks, (float)(lr / bias_correction1),
                                                            (float)beta2, (float)(1.0 - beta1), (float)(1.0 - beta2), (float)eps,
                                                            (float)weight_decay, (float)bias_correction2_sqrt,
                                                            (const d3_clip_ctl *)ctl);
    D3_LAUNCH_CHECK();
    return 0;
}

template <bool CTL>
static int sgd_launch(const long long *ptrs, const int *numel, const void *blocks, int nblocks, double lr, double momentum,
                      double weight_decay, int first, const void *ctl, void *stream) {
    D3_CLEAR();
    if (nblocks <= 0) return 0;
    if (d3_adamw_chunk() != OPT_CHUNK || (CTL && !ctl)) return D3_ERR_ARG;
    if (first && momentum == 0.0) return D3_ERR_ARG;   // no buffer to initialise
    hipStream_t s = d3_stream(stream);
    const int2 *bm = (const int2 *)blocks;
    const d3_clip_ctl *c = (const d3_clip_ctl *)ctl;
    const float flr = (float)lr, fmu = (float)momentum, fwd = (float)weight_decay;
    if (momentum == 0.0) sgd_kernel<false, false, CTL><<<nblocks, 256, 0, s>>>(ptrs, numel, bm, flr, fmu, fwd, c);
    else if (first) sgd_kernel<true, true, CTL><<<nblocks, 256, 0, s>>>(ptrs, numel, bm, flr, fmu, fwd, c);
    else sgd_kernel<true, false, CTL><<<nblocks, 256, 0, s>>>(ptrs, numel, bm, flr, fmu, fwd, c);
    D3_LAUNCH_CHECK();
    return 0;
}

extern "C" int d3_adam(const long long *ptrs, const int *numel, const void *blocks, int nblocks, double lr, double beta1,
                       double beta2, double eps, double weight_decay, double bias_correction1, double bias_correction2_sqrt,
                       void *stream) {
    return adam_launch<false>(ptrs, numel, blocks, nblocks, lr, beta1, beta2, eps, weight_decay, bias_correction1,
                              bias_correction2_sqrt, nullptr, stream);
}

extern "C" int d3_adam_clipped(const long long *ptrs, const int *numel, const void *blocks, int nblocks, double lr, double beta1,
                               double beta2, double eps, double weight_decay, double bias_correction1,
                               double bias_correction2_sqrt, const void *ctl, void *stream) {
    return adam_launch<true>(ptrs, numel, blocks, nblocks, lr, beta1, beta2, eps, weight_decay, bias_correction1,
                             bias_correction2_sqrt, ctl, stream);
}

extern "C" int d3_sgd(const long long *ptrs, const int *numel, const void *blocks, int nblocks, double lr, double momentum,
                      double weight_decay, int first, void *stream) {
    return sgd_launch<false>(ptrs, numel, blocks, nblocks, lr, momentum, weight_decay, first, nullptr, stream);
}

extern "C" int d3_sgd_clipped(const long long *ptrs, const int *numel, const void *blocks, int nblocks, double lr, double momentum,
                              double weight_decay, int first, const void *ctl, void *stream) {
    return sgd_launch<true>(ptrs, numel, blocks, nblocks, lr, momentum, weight_decay, first, ctl, stream);
}
