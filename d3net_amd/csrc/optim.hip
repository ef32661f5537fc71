// optim.hip -- Adam and SGD over every parameter tensor of a group in ONE launch (gfx950), beside the AdamW of
// heads.hip and with its table design: a device table of 4 pointers per tensor, `numel` per tensor and a block map of
// (tensor, chunk) pairs, one workgroup of 256 threads per pair, chunk = d3_adamw_chunk() = 4096 elements.  All loads of a
// chunk are issued before the arithmetic; plain fp32 vector loads and stores, no LDS, no atomics.
// The reference builds torch.optim.Adam / SGD by name (model/pipeline.py:738-757, model/pointgroup.py:372-384); the
// arithmetic below is the library's, operation by operation (the build runs with -ffp-contract=off).
// HBM bound: Adam 4 reads + 3 writes of 4 B per element; SGD 3 + 2 with a momentum buffer (2 + 2 on a tensor's first
// update, which only writes the buffer), 2 + 1 without momentum.
#include "common.h"

#define OPT_CHUNK 4096   // = d3_adamw_chunk(): the host builds ONE block map for all three optimizers
#define OPT_PER (OPT_CHUNK / 256)

// torch.optim.Adam (amsgrad = False, maximize = False), L2 weight decay folded into the gradient:
//   g' = g + wd p;  m = m + (1 - b1)(g' - m);  v = b2 v + (1 - b2) g'^2;  p = p - (lr / bc1) (m / (sqrt(v) / sqrt(bc2) + eps))
// table columns: param, grad, exp_avg, exp_avg_sq
__global__ __launch_bounds__(256) void adam_kernel(const long long *__restrict__ ptrs, const int *__restrict__ numel,
                                                  const int2 *__restrict__ blocks, float step_size, float beta2, float omb1,
                                                  float omb2, float eps, float wd, float bc2_sqrt) {
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
            const float gg = gv[j] + wd * pv[j];
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
template <bool MOM, bool FIRST>
__global__ __launch_bounds__(256) void sgd_kernel(const long long *__restrict__ ptrs, const int *__restrict__ numel,
                                                 const int2 *__restrict__ blocks, float lr, float mu, float wd) {
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
            float d = gv[j] + wd * pv[j];
            if (MOM) {
                if (!FIRST) d = mu * bv[j] + d;
                buf[i] = d;
            }
            p[i] = pv[j] - lr * d;
        }
    }
}

extern "C" int d3_adam(const long long *ptrs, const int *numel, const void *blocks, int nblocks, double lr, double beta1,
                       double beta2, double eps, double weight_decay, double bias_correction1, double bias_correction2_sqrt,
                       void *stream) {
    D3_CLEAR();
    if (nblocks <= 0) return 0;
    if (d3_adamw_chunk() != OPT_CHUNK) return D3_ERR_ARG;
    // scalars derived in double, as the library does before it narrows them
    adam_kernel<<<nblocks, 256, 0, d3_stream(stream)>>>(ptrs, numel, (const int2 *)blocks, (float)(lr / bias_correction1),
                                                       (float)beta2, (float)(1.0 - beta1), (float)(1.0 - beta2), (float)eps,
                                                       (float)weight_decay, (float)bias_correction2_sqrt);
    D3_LAUNCH_CHECK();
    return 0;
}

extern "C" int d3_sgd(const long long *ptrs, const int *numel, const void *blocks, int nblocks, double lr, double momentum,
                      double weight_decay, int first, void *stream) {
    D3_CLEAR();
    if (nblocks <= 0) return 0;
    if (d3_adamw_chunk() != OPT_CHUNK) return D3_ERR_ARG;
    if (first && momentum == 0.0) return D3_ERR_ARG;   // no buffer to initialise
    hipStream_t s = d3_stream(stream);
    const int2 *bm = (const int2 *)blocks;
    const float flr = (float)lr, fmu = (float)momentum, fwd = (float)weight_decay;
    if (momentum == 0.0) sgd_kernel<false, false><<<nblocks, 256, 0, s>>>(ptrs, numel, bm, flr, fmu, fwd);
    else if (first) sgd_kernel<true, true><<<nblocks, 256, 0, s>>>(ptrs, numel, bm, flr, fmu, fwd);
    else sgd_kernel<true, false><<<nblocks, 256, 0, s>>>(ptrs, numel, bm, flr, fmu, fwd);
    D3_LAUNCH_CHECK();
    return 0;
}
