// torch_argmax.h -- torch.argmax's CPU rule for one wave64, shared by grounding_eval.hip and submission.hip: a NaN ranks above every
// number, +0 == -0, the lowest index wins among equals (within a lane the indices ascend and only a strictly better value replaces
// the held one; across lanes the lower index wins a draw).
#pragma once
#include "common.h"

#define GE_NONE 0x7fffffff      // index of a lane that holds no element: loses every draw

// does (v, i) beat (bv, bi) under torch.argmax's CPU rule
__device__ __forceinline__ bool ge_beats(float v, int i, float bv, int bi) {
    if (i == GE_NONE) return false;
    if (bi == GE_NONE) return true;
    const bool vn = v != v, bn = bv != bv;
    if (vn || bn) return vn && (!bn || i < bi);
    return v > bv || (v == bv && i < bi);
}

__device__ __forceinline__ int ge_wave_argmax(float v, int i) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const float ov = __shfl_xor(v, m, 64);
        const int oi = __shfl_xor(i, m, 64);
        if (ge_beats(ov, oi, v, i)) { v = ov; i = oi; }
    }
    return i;
}
