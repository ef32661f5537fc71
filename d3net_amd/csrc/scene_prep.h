// scene_prep.h -- what scene_prep.hip (one scene at a time) and batch_prep.hip (a batch from the scene store) share: the limits and
// the order-preserving integer image of a double that carries the deterministic min / max reductions.
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
