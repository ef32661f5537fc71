// common.h -- shared helpers for the gfx950 kernels of libd3hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include "../../include/d3hip.h"

#define D3_WAVE 64

#define D3_CHECK(expr)                                   \
    do {                                                 \
        hipError_t _e = (expr);                          \
        if (_e != hipSuccess) return (int)_e;            \
    } while (0)

#define D3_LAUNCH_CHECK()                                \
    do {                                                 \
        hipError_t _e = hipGetLastError();               \
        if (_e != hipSuccess) return (int)_e;            \
    } while (0)

// drop a stale (sticky) error left by an earlier, unrelated HIP call so that launch checks report our own
#define D3_CLEAR() (void)hipGetLastError()

static inline hipStream_t d3_stream(void *s) { return (hipStream_t)s; }

static inline size_t d3_align(size_t x, size_t a = 256) { return (x + a - 1) / a * a; }

// carve typed, 256-byte aligned regions out of a workspace.  A layout function lists the regions once; the run carves
// with it and checks ok() before its first launch, the *_ws_bytes query runs it on a null base (take() then returns
// nullptr and only advances off) and reads off.
struct D3Carver {
    char *base; size_t cap; size_t off;
    D3Carver(void *ws, size_t bytes) : base((char *)ws), cap(bytes), off(0) {}
    template <typename T> T *take(size_t count) {
        size_t bytes = d3_align(count * sizeof(T));
        T *p = base ? (T *)(base + off) : nullptr;
        off += bytes;
        return p;
    }
    bool ok() const { return base != nullptr && off <= cap; }
};

__device__ __forceinline__ int d3_lane() { return (int)(threadIdx.x & 63); }

__device__ __forceinline__ unsigned long long d3_lanemask_lt() {
    return (1ull << (threadIdx.x & 63)) - 1ull;
}

// measurement / test switches: ONE table parsed once from the environment (tuning.hip); launch paths read a slot
enum D3Tune { D3T_ATTN_SCALAR, D3T_BFS_NO_STAR, D3T_WG3, D3T_GRAD_BF16, D3T_BQ_GRID, D3T_BN_FUSED_ROWS, D3T_KMAP16, D3T_HG_SPLITK, D3T_BN_PART2, D3T_CL_SPEC,
              D3T_TD_FUSE_GATES, D3T_C3, D3T_COUNT };
int d3_tune(int key);

// exclusive int32 scan / total via rocPRIM (implemented in scan_sort.hip)
size_t d3_scan_temp_bytes(int n);
int d3_exclusive_scan_i32(const int *in, int *out, int n, void *temp, size_t temp_bytes, hipStream_t s);
size_t d3_sort_pairs_temp_bytes(int n);
// stable ascending sort of (key,val) int32 pairs on the low `bits` bits of key
int d3_sort_pairs_i32(const int *kin, int *kout, const int *vin, int *vout, int n, int bits, void *temp,
                      size_t temp_bytes, hipStream_t s);

// batched fp32-MFMA GEMMs and column sums (implemented in hgemm.hip)
int hg_launch(const d3_gemm_prob *probs, int nprobs, hipStream_t s);
size_t hg_colsum_ws_bytes(int njobs, int cmax);
// n column sums in two launches; ws >= hg_colsum_ws_bytes(n, max C)
int hg_colsum_multi(const float *const *x, const long long *ld, const int *R, const int *C, float *const *out, const int *accum, int n,
                    void *ws, size_t ws_bytes, hipStream_t s);
