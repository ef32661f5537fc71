// spconv2.hip -- second-generation sparse convolution kernels for gfx950: wave-autonomous gather -> MFMA.
//
// Same contraction as spconv.hip (MinkowskiConvolution / MinkowskiConvolutionTranspose forward and data gradient,
// reference call sites model/common.py:32,38,41,66,90,98; model/pointgroup.py:70):
//
//   out[u,:] = sum_k x[tbl[u,k],:] @ W[k]   (+ res[u,:])        tbl: dense (Mout,K) kernel map (coordmap.hip)
//
// Design (what changed against spconv.hip, and why -- profiles/r01_h: the 64-row LDS-staged tile spends one barrier
// and one LDS round trip per (offset, 32 channels) to feed a single 16x16x16 MFMA at C=16):
//   * a WAVE owns a 16-row output tile.  The MFMA A operand (16 rows x 32 reduction elements, 8 bf16 per lane) is
//     gathered straight from HBM/L2 into registers: lane (r = lane&15, g = lane>>4) loads 16 bytes (8 channels) of
//     input row tbl[row0+r][k]; no LDS staging of activations, no workgroup barrier in the main loop.
//   * the reduction index is the flattened list of (active offset, 8-channel group) "slots"; one
//     v_mfma_f32_16x16x32_bf16 consumes four slots (one per lane group), so Cin=16 packs two offsets into one MFMA
//     and offsets unused by the 16-row tile cost nothing (4x finer skipping than a 64-row tile).
//   * weights are pre-packed once per step into bf16 MFMA-B fragment order (d3_spconv_pack); a fragment is one
//     contiguous 16-byte read per lane, from LDS when the layer's weights fit (big levels, persistent workgroups)
//     or from L2 (deep levels).
//   * few-row levels: the waves of a workgroup split the slots of ONE tile and reduce through LDS -- no atomics,
//     no zero fill, deterministic, and the complete tile is available to the epilogue.
//   * epilogue fusions: residual add, accumulate-into, strided output (writes straight into a concatenated
//     buffer) and per-channel sum / sum-of-squares partials for the following BatchNorm.
// Roofline: HBM; algorithmic bytes per launch as in spconv.hip.
// (The weight gradients of these layers: wgrad.hip.)
#include "conv.h"
#include "prof.h"
#include <cstdlib>
#include <cstring>

#ifndef C2_UBIG
#define C2_UBIG 8
#endif
#ifndef C2_OCC_SMALL
#define C2_OCC_SMALL 4
#endif
#ifndef C2_PREFETCH
#define C2_PREFETCH 1   // prefetch the next tile's kernel-map rows into registers (7 VGPRs)
#endif
#define C2_U(NTV) ((NTV) <= 2 ? C2_UBIG : 4)   // MFMA steps whose gathers are issued together

// ------------------------------------------------------------------------------ weight packing
// Wp[((k*S + c8)*NT + n)*16 + col][8] = bf16(Weff[k][c8*8 + j][n*16 + col]),  Weff = W[flipk ? K-1-k : k] (or its
// transpose when W is laid out (K, Cout, Cin)); columns >= Cout are zero.
__global__ void spconv_pack_kernel(const float *__restrict__ W, uint4 *__restrict__ Wp, int K, int Cin, int Cout,
                                   int NT, int flipk, int transw) {
    const int S = Cin >> 3;
    const long long total = (long long)K * S * NT * 16;
    long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    const int col = (int)(e & 15);
    const int n = (int)((e >> 4) % NT);
    const int c8 = (int)((e / (16 * NT)) % S);
    const int k = (int)(e / ((long long)16 * NT * S));
    const int co = n * 16 + col, wk = flipk ? (K - 1 - k) : k;
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const int ci = c8 * 8 + j;
        v[j] = 0.f;
        if (co < Cout) v[j] = transw ? W[((long long)wk * Cout + co) * Cin + ci] : W[((long long)wk * Cin + ci) * Cout + co];
    }
    Wp[e] = make_uint4(pack2bf2(v[0], v[1]), pack2bf2(v[2], v[3]), pack2bf2(v[4], v[5]), pack2bf2(v[6], v[7]));
}

// fp32 fragments (D3_CONV_F32: the reference's precision on v_mfma_f32_16x16x4_f32): same element order, 8 floats per element
__global__ void spconv_pack_f32_kernel(const float *__restrict__ W, float4 *__restrict__ Wp, int K, int Cin, int Cout,
                                       int NT, int flipk, int transw) {
    const int S = Cin >> 3;
    const long long total = (long long)K * S * NT * 16;
    long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    const int col = (int)(e & 15);
    const int n = (int)((e >> 4) % NT);
    const int c8 = (int)((e / (16 * NT)) % S);
    const int k = (int)(e / ((long long)16 * NT * S));
    const int co = n * 16 + col, wk = flipk ? (K - 1 - k) : k;
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const int ci = c8 * 8 + j;
        v[j] = 0.f;
        if (co < Cout) v[j] = transw ? W[((long long)wk * Cout + co) * Cin + ci] : W[((long long)wk * Cin + ci) * Cout + co];
    }
    Wp[e * 2] = make_float4(v[0], v[1], v[2], v[3]);
    Wp[e * 2 + 1] = make_float4(v[4], v[5], v[6], v[7]);
}

extern "C" size_t d3_spconv_pack_bytes(int K, int Cin, int Cout) {
    return (size_t)K * (Cin / 8) * ((Cout + 15) / 16) * 256;
}
extern "C" size_t d3_spconv_pack_bytes_ex(int K, int Cin, int Cout, int flags) {
    return d3_spconv_pack_bytes(K, Cin, Cout) * ((flags & D3_CONV_F32) ? 2 : 1);
}

extern "C" int d3_spconv_pack(const float *W, void *Wp, int K, int Cin, int Cout, int flags, void *stream) {
    D3_CLEAR();
    if (K < 1 || K > C2_MAXK || Cin < 8 || (Cin & 7) || Cout < 1) return D3_ERR_ARG;
    const int NT = (Cout + 15) / 16;
    const long long total = (long long)K * (Cin / 8) * NT * 16;
    if (flags & D3_CONV_F32)
        spconv_pack_f32_kernel<<<(int)((total + 255) / 256), 256, 0, d3_stream(stream)>>>(
            W, (float4 *)Wp, K, Cin, Cout, NT, (flags & D3_CONV_FLIPK) ? 1 : 0, (flags & D3_CONV_TRANSW) ? 1 : 0);
    else
    spconv_pack_kernel<<<(int)((total + 255) / 256), 256, 0, d3_stream(stream)>>>(
        W, (uint4 *)Wp, K, Cin, Cout, NT, (flags & D3_CONV_FLIPK) ? 1 : 0, (flags & D3_CONV_TRANSW) ? 1 : 0);
    D3_LAUNCH_CHECK();
    return 0;
}

// Second-level BatchNorm partials (round 5).  Every BatchNorm launch used to reduce its producer's whole partial table (one row per
// convolution workgroup: ~1000 rows at the big levels) IN EVERY ONE of its <= 512 workgroups before it could touch a row: 8 - 19 us
// of dependent L2 round trips per launch, ~155 launches per step -- more than the normalisation passes themselves.  The producer
// now also adds its row into a 16-row fp64 table (hardware fp64 atomics, row = workgroup % 16: <= 64 adds per address); the
// consumer's reduction is ONE round trip over 16 rows.  Every addend is an fp32 value, so the fp64 sums are exact -- independent of
// the order the atomics land in -- unless the addends of one channel span more than 2^29 in magnitude (then: 2^-53 relative).
// (the 16 rows: D3_P2_ROWS, conv.h)
// ------------------------------------------------------------------------------ forward / data gradient
struct Conv2Args {
    const void *x;              // (Min, ldx) fp32 or bf16
    const int *tbl;             // (Mout, K) or NULL (identity, K = 1)
    const unsigned short *Wp;   // packed bf16 fragments
    float *out;                 // (Mout, ldo)
    const float *res;           // optional residual (Mout, ldr), added before the store
    float *part;                // optional BatchNorm partials: [nparts][2][NT*16] (sum, sum of squares per column)
    double *part2;              // optional (round 5): second-level table [D3_P2_ROWS][2][NT*16] of fp64 accumulators; workgroup b adds its
                                // partial row to row b % D3_P2_ROWS (zeroed by the caller), so a consumer reads 16 rows instead of ~1000
    int ldx, ldo, ldr;
    int Mout, K, Cout, S;       // S = Cin / 8 slots per offset
    unsigned int inv;           // ceil(65536 / S): i = (s * inv) >> 16 == s / S for s < 4096
    int xbf16, accum, ntiles, NT;   // NT = ceil(Cout / 16)
    int obf16;                      // D3_CONV_OUTBF16: out is (Mout, ldo) bf16
    int f32;                        // D3_CONV_F32: fp32 weight fragments, v_mfma_f32_16x16x4_f32 (host-side dispatch only)
    unsigned int xbytes;            // extent of x in bytes for the raw buffer gathers (0: beyond 2 GiB / 2^24 rows, refused for the wave-per-tile kernel)
    unsigned int invK;          // ceil(65536 / K): e / K for e < 16*27
    const unsigned int *tbl16;  // optional 16-bit delta form of tbl (coordmap.hip cm_pack16_kernel; validated by the caller), read as 32-bit
                                // words by the T16 instances of the wave-per-tile kernel
    // BatchNorm-backward epilogue (data gradient of a BN -> ReLU -> conv unit): the stored value is g = dy * relu'(bn(x))
    // and the partials are (sum g, sum g * xhat) -- the two reductions of the BatchNorm backward, fused here
    const float *bnx; const float *bn_mean, *bn_var, *bn_gamma, *bn_beta;
    int ldbx, bn_relu; float bn_eps;
    int bnx_bf16;               // D3_CONV_BNXBF16: bnx is stored as bf16 (a single-consumer convolution output, round 6)
};

__device__ __forceinline__ bf16x8_t c2_zero() {
    uint4 z = make_uint4(0u, 0u, 0u, 0u);
    return __builtin_bit_cast(bf16x8_t, z);
}
__device__ __forceinline__ bf16x8_t c2_load_a(const void *x, int xbf16, long long off) {
    if (xbf16) {
        uint4 v = *(const uint4 *)((const unsigned short *)x + off);
        return __builtin_bit_cast(bf16x8_t, v);
    }
    const float4 f0 = *(const float4 *)((const float *)x + off);
    const float4 f1 = *(const float4 *)((const float *)x + off + 4);
    uint4 v = make_uint4(pack2bf2(f0.x, f0.y), pack2bf2(f0.z, f0.w), pack2bf2(f1.x, f1.y), pack2bf2(f1.z, f1.w));
    return __builtin_bit_cast(bf16x8_t, v);
}

// Gathers are issued RAW (no conversion next to the load): a use right behind a load makes the compiler wait for it
// before the next load is issued, i.e. one memory round trip per gathered row instead of one per batch.
template <bool XBF>
__device__ __forceinline__ void c2_load_raw(const void *x, long long off, uint4 &lo, uint4 &hi) {
    if (XBF) lo = *(const uint4 *)((const unsigned short *)x + off);
    else { lo = *(const uint4 *)((const float *)x + off); hi = *(const uint4 *)((const float *)x + off + 4); }
}
__device__ __forceinline__ uint4 c2_from_u32x4(const u32x4_t v) { return make_uint4(v.x, v.y, v.z, v.w); }
template <bool XBF>
__device__ __forceinline__ bf16x8_t c2_cvt_raw(const uint4 lo, const uint4 hi) {
    if (XBF) return __builtin_bit_cast(bf16x8_t, lo);
    const uint4 v = make_uint4(pack2bf2(__uint_as_float(lo.x), __uint_as_float(lo.y)), pack2bf2(__uint_as_float(lo.z), __uint_as_float(lo.w)),
                               pack2bf2(__uint_as_float(hi.x), __uint_as_float(hi.y)), pack2bf2(__uint_as_float(hi.z), __uint_as_float(hi.w)));
    return __builtin_bit_cast(bf16x8_t, v);
}

// One reduction step of a 16x16 tile (transposed product: first operand = weight fragment, second = gathered rows).
// bf16: one v_mfma_f32_16x16x32_bf16 over the lane's 8 channels; F32M (D3_CONV_F32, fp32 gathers only): eight
// v_mfma_f32_16x16x4_f32 -- step j pairs float j of the weight element with float j of the gathered 8 channels, i.e. the
// reduction index (lane group, j) is the same channel on both sides: exact fp32 products, fp32 accumulation.
template <bool XBF, bool F32M>
__device__ __forceinline__ f32x4 c2_mma(f32x4 acc, const uint4 wlo, const uint4 whi, const uint4 rlo, const uint4 rhi) {
    if (F32M) {
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(wlo.x), __uint_as_float(rlo.x), acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(wlo.y), __uint_as_float(rlo.y), acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(wlo.z), __uint_as_float(rlo.z), acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(wlo.w), __uint_as_float(rlo.w), acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(whi.x), __uint_as_float(rhi.x), acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(whi.y), __uint_as_float(rhi.y), acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(whi.z), __uint_as_float(rhi.z), acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(whi.w), __uint_as_float(rhi.w), acc, 0, 0, 0);
        return acc;
    }
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, wlo), c2_cvt_raw<XBF>(rlo, rhi), acc, 0, 0, 0);
}
// weight element `e` (16-byte bf16 fragment, or 32-byte fp32 fragment) of a packed buffer
template <bool F32M>
__device__ __forceinline__ void c2_wload(const unsigned short *Wb, int e, uint4 &lo, uint4 &hi) {
    if (F32M) { const uint4 *p = (const uint4 *)Wb + (size_t)e * 2; lo = p[0]; hi = p[1]; }
    else { lo = *((const uint4 *)Wb + e); hi = lo; }
}

// LDS use of the wave-per-tile kernel besides the weights
#define C2_TBL_SENT (16 * C2_MAXK)        // one more slot per wave that always holds -1 (steps beyond the reduction read it)
#define C2_TBL_INTS (16 * C2_MAXK + 16)
#define C2_WAVE_LDS_BASE(NTV, NWV) ((NWV) * C2_TBL_INTS * 4 + (NWV) * 32 * 4 + (NWV) * 2 * (NTV) * 16 * 4)
#define C2_WAVE_LDS_BYTES(NTV, NWV) (C2_WAVE_LDS_BASE(NTV, NWV) + (NTV) * 16 * 16)   // + BatchNorm parameters, float4 per channel

// Wave-per-tile kernel (big levels): NW independent waves per workgroup (4, or 16 when the layer's packed weights are
// large: ONE LDS copy then serves 16 waves -- a 117 KB stem / 124 KB 48->48 weight set fits the CU's 160 KB once, and a
// 55 KB 32->32 set is staged by 256 workgroups instead of 1024), persistent over a contiguous range of
// NW-tile groups (XCD-contiguous: block b runs on XCD b % 8, so XCD x gets the x-th eighth of the rows and the
// neighbour rows its tiles gather stay in that XCD's L2).
// Every dependent global access of a wave is a full L2/HBM round trip and the MFMA work between them is tiny, so the
// kernel is organised around round trips, not FLOPs: (1) the kernel-map rows of the NEXT tile are prefetched into
// registers while the current tile computes; (2) all gathers of a batch are issued before the first MFMA; (3) no
// per-tile offset mask / compaction (its shuffle + LDS chain cost more than the skipped MFMAs: a 16-row tile uses
// nearly all offsets) -- absent neighbours simply gather nothing; (4) the MFMA is issued TRANSPOSED (A = weights,
// B = gathered rows), so a lane ends up with 4 consecutive output channels of one row: the tile is stored (and the
// residual read) as one contiguous float4 per lane instead of four 64-byte row fragments.
// (fp32 gathers hold twice the registers of bf16 ones until they are converted: one occupancy step less)
#ifndef C2_F32_U
#define C2_F32_U 8          // gathers per batch of the fp32-input variants with <= 2 column tiles (experiments: 4 with C2_F32_OCCDROP 0)
#endif
#ifndef C2_F32_OCCDROP
#define C2_F32_OCCDROP 1
#endif
#define C2_OCC(NTV, XB) ((NTV) <= 4 ? ((XB) ? C2_OCC_SMALL : C2_OCC_SMALL - C2_F32_OCCDROP) : (NTV) <= 9 ? ((XB) ? 3 : 2) : 2)
// KT / ST > 0: kernel size and slots per offset (Cin / 8) known at compile time (round 3: the shapes that carry the step -- K = 27
// with 16 / 32 / 64 input channels): the reduction loop is fully unrolled and every (offset, channel group) of a step is a
// constant per lane group -- the ~10 index instructions in front of each gather fold away.
// CMP (round 5, the statically shaped instances): the offsets NO row of the tile has are dropped before the reduction loop.  The
// kernel is bound by the dependent round trips of a wave (table -> gathers -> products, one per batch), not by a throughput: with
// the rows in raster order a 16-row tile of the 2 cm level uses 15.9 of the 27 offsets on average (a planar patch: 9), so the
// batches of a tile shrink from 14 to ~8 (stem) / from 2 to mostly 1 (16 -> 16).  One 27-lane pass over the tile's table in LDS
// gives the mask; the live offsets are then taken from it with scalar instructions (no list in memory).
template <int NT, bool WLDS, bool XBF, int NW, bool F32M, int KT, int ST, bool T16, bool CMP = false>
__device__ __forceinline__ void spconv_fwd2_body(const Conv2Args &a) {
    static_assert(!CMP || (KT == 27 && (ST == 2 || ST >= 4)), "offset compaction: the statically shaped instances");
    static_assert(!T16 || KT == 27, "the 16-bit kernel map is read by the statically shaped K = 27 instances");
    constexpr int NWT = NW;             // tiles of a workgroup's turn
    static_assert(!(F32M && XBF), "fp32 MFMA needs fp32 gathers");
    static_assert((KT > 0) == (ST > 0), "static shapes fix both the kernel size and the channel groups");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    // (16-wave workgroups run at 128 VGPRs: the fp32-input variants keep 4 gathers of 32 B in flight there instead of 8)
    // statically shaped, >= 32 input channels: a batch is KB whole offsets of Q = ceil(ST / 4) steps each
    constexpr int Q = ST >= 4 ? (ST + 3) / 4 : 1;
    constexpr int KB = ST >= 4 ? (Q >= 5 ? 2 : (8 / Q > 0 ? 8 / Q : 1)) : 1;
    constexpr int U = ST >= 4 ? KB * Q : (!XBF && NT <= 2) ? (NW == 16 ? 4 : C2_F32_U) : C2_U(NT);
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, r = lane & 15, g = lane >> 4;
    const int slot = wave;
    const int K = KT ? KT : a.K, S = ST ? ST : a.S;
    const size_t wbytes = WLDS ? (size_t)K * S * NT * (F32M ? 512 : 256) : 0;
    int *tblS = (int *)(smem + wbytes) + wave * C2_TBL_INTS;
    float *redS = (float *)(smem + wbytes + NW * C2_TBL_INTS * 4);
    const unsigned short *Wb = WLDS ? (const unsigned short *)smem : a.Wp;
    const int nb = gridDim.x, b = blockIdx.x;
    const int lb = ((nb & 7) == 0) ? (b & 7) * (nb >> 3) + (b >> 3) : b;
    const int ntg = (a.ntiles + NWT - 1) / NWT;
    const int per = (ntg + nb - 1) / nb;
    // Round 4: the nb / 8 workgroups of an XCD take the XCD's tile groups IN TURN (iteration i of workgroup j:
    // group xcd_base + i * (nb / 8) + j) instead of one contiguous range each: at any moment the XCD works on ONE window of
    // (nb / 8) * NW * 16 consecutive rows plus its neighbourhood, which fits its 4 MB L2, where 32 separate windows do not (the
    // stem gathers 272-byte rows from +-1 x-slab: measured 1032 MB of HBM-side traffic per launch against 245 MB algorithmic).
    const bool il = (nb & 7) == 0;
    const int tstride = il ? (nb >> 3) : 1;
    const int tg0 = il ? (b & 7) * (nb >> 3) * per + (b >> 3) : lb * per;
    const int tg1 = il ? min(ntg, ((b & 7) + 1) * (nb >> 3) * per) : min(ntg, tg0 + per);
    int v[7];
    // 16-bit table (round 4): entries (2d, 2d + 1) of the tile travel as ONE 32-bit word d = lane + it * 64 < 8 K; v[0..3] hold the
    // raw words, the LDS store decodes them (row + delta; 0x8000 = absent).  K is odd: the word that straddles the end of the
    // table's last row reads one of the two pad entries behind it.
    constexpr bool t16 = T16;                                  // (the host validated the table: ConvExtras, conv.h)
#define C2_LOAD_TBL(TILE)                                                                                     \
    {                                                                                                         \
        const int tile_ = (TILE);                                                                             \
        const long long base_ = (long long)tile_ * 16 * K, lim_ = (long long)a.Mout * K;                      \
        if constexpr (t16) {                                                                                  \
            _Pragma("unroll") for (int it = 0; it < 4; it++) {                                                \
                const int d = lane + it * 64;                                                                 \
                v[it] = (int)0x80008000u;                                                                     \
                if (tile_ < a.ntiles && d < 8 * K && base_ + 2 * d < lim_) v[it] = (int)a.tbl16[(base_ >> 1) + d]; \
            }                                                                                                 \
        } else {                                                                                              \
        _Pragma("unroll") for (int it = 0; it < 7; it++) {                                                    \
            const int e = lane + it * 64;                                                                     \
            v[it] = -1;                                                                                       \
            if (tile_ < a.ntiles && e < 16 * K && base_ + e < lim_) v[it] = a.tbl ? a.tbl[base_ + e] : (int)(base_ + e); \
        }                                                                                                     \
        }                                                                                                     \
    }
    if (C2_PREFETCH) C2_LOAD_TBL(tg0 * NWT + slot)
    float4 *bnS = (float4 *)(smem + wbytes + C2_WAVE_LDS_BASE(NT, NW));   // (mean, 1/std, gamma, beta) per channel
    if (a.bnx && t < NT * 16) {
        float4 bp = make_float4(0.f, 0.f, 0.f, 0.f);
        if (t < a.Cout) {
            bp.x = a.bn_mean[t]; bp.y = rsqrtf(a.bn_var[t] + a.bn_eps);
            if (a.bn_relu) { bp.z = a.bn_gamma[t]; bp.w = a.bn_beta[t]; }
        }
        bnS[t] = bp;
    }
    if (WLDS) {
        const uint4 *src = (const uint4 *)a.Wp;
        uint4 *dst = (uint4 *)smem;
        const int n16 = (int)(wbytes >> 4);
        for (int i0 = 0; i0 < n16; i0 += 4 * 64 * NW) {
            uint4 w4[4];
#pragma unroll
            for (int q = 0; q < 4; q++) { const int i = i0 + q * 64 * NW + t; w4[q] = make_uint4(0u, 0u, 0u, 0u); if (i < n16) w4[q] = src[i]; }
#pragma unroll
            for (int q = 0; q < 4; q++) { const int i = i0 + q * 64 * NW + t; if (i < n16) dst[i] = w4[q]; }
        }
    }
    if (WLDS || a.bnx) __syncthreads();
    f32x4 ssum[NT], ssq[NT];   // per lane: its row's values, channels n*16 + g*4 + q
#pragma unroll
    for (int n = 0; n < NT; n++) { ssum[n] = (f32x4){0.f, 0.f, 0.f, 0.f}; ssq[n] = (f32x4){0.f, 0.f, 0.f, 0.f}; }
    const int nsteps = (K * S + 3) >> 2;
    constexpr int NSTEPS_T = (KT * ST + 3) / 4;   // static shapes below 32 channels: steps of a tile
    const unsigned int xrowb = (unsigned int)a.ldx * (XBF ? 2u : 4u);
    const int rK = r * K;
    if (lane == 0) tblS[C2_TBL_SENT] = -1;
    const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc((void *)a.x, 0, a.xbytes, D3_RSRC_FLAGS);

    for (int tg = tg0; tg < tg1; tg += tstride) {
        const int tile = tg * NWT + slot;
        if (tile >= a.ntiles) continue;   // wave-uniform; there is no workgroup barrier inside this loop
        const int row0 = tile * 16;
        if (!C2_PREFETCH) C2_LOAD_TBL(tile)
        if constexpr (t16) {
#pragma unroll
            for (int it = 0; it < 4; it++) {
                const int d = lane + it * 64;
                if (d < 8 * K) {
                    const int e0 = 2 * d, e1 = e0 + 1;
                    const int lo = (int)(short)(v[it] & 0xFFFF), hi = v[it] >> 16;          // (arithmetic shift: sign-extended)
                    const int u0 = e0 / (KT ? KT : 1), u1 = e1 / (KT ? KT : 1);
                    // (entries behind the table's end are absent already: words not loaded are 0x80008000 and the one word
                    // that straddles the end carries a pad entry, which cm_pack16_kernel wrote as absent)
                    tblS[e0] = lo == -32768 ? -1 : row0 + u0 + lo;
                    tblS[e1] = hi == -32768 ? -1 : row0 + u1 + hi;
                }
            }
        } else {
#pragma unroll
        for (int it = 0; it < 7; it++) {
            const int e = lane + it * 64;
            if (e < 16 * K) tblS[e] = v[it];
        }
        }
        if (C2_PREFETCH && tg + tstride < tg1) C2_LOAD_TBL(tile + NWT * tstride)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        unsigned int kmask = 0u;
        if constexpr (CMP) {      // bit k: some row of the tile has offset k (absent entries are -1: the AND of a column keeps the sign bit)
            int av = -1;
            if (lane < KT) {
#pragma unroll
                for (int rr = 0; rr < 16; rr++) av &= tblS[rr * KT + lane];
            }
            kmask = (unsigned int)__builtin_amdgcn_readfirstlane((int)(unsigned int)__ballot(lane < KT && av >= 0));
        }

        f32x4 acc[NT];
#pragma unroll
        for (int n = 0; n < NT; n++) acc[n] = (f32x4){0.f, 0.f, 0.f, 0.f};
        // Epilogue operands (residual, accumulate target, BatchNorm input) do not depend on the gathers: for narrow
        // outputs they are requested BEFORE the gathers and arrive with them; wider outputs request them in chunks of
        // NB column tiles at the epilogue (one round trip per chunk, not one per operand).
        constexpr int NB = NT <= 4 ? NT : 4;
        constexpr bool HOIST = NT == 1 || (NT == 2 && !XBF);   // (register budget of the bf16 variants: 128)
        f32x4 e_res[NB], e_out[NB], e_bnx[NB];
        const int urow = row0 + r;
#define C2_EPI_LOAD(N0)                                                                                       \
        _Pragma("unroll") for (int j = 0; j < NB; j++) {                                                      \
            const int col = ((N0) + j) * 16 + g * 4;                                                          \
            e_res[j] = (f32x4){0.f, 0.f, 0.f, 0.f}; e_out[j] = e_res[j]; e_bnx[j] = e_res[j];                   \
            if ((N0) + j < NT && urow < a.Mout && col < a.Cout) {                                             \
                if (a.res) e_res[j] = *(const f32x4 *)(a.res + (long long)urow * a.ldr + col);                \
                if (a.accum) e_out[j] = *(const f32x4 *)(a.out + (long long)urow * a.ldo + col);              \
                if (a.bnx) {                                                                                  \
                    if (a.bnx_bf16) { const uint2 b2 = *(const uint2 *)((const unsigned short *)a.bnx + (long long)urow * a.ldbx + col); \
                        e_bnx[j] = (f32x4){__uint_as_float(b2.x << 16), __uint_as_float(b2.x & 0xFFFF0000u), __uint_as_float(b2.y << 16), __uint_as_float(b2.y & 0xFFFF0000u)}; } \
                    else e_bnx[j] = *(const f32x4 *)(a.bnx + (long long)urow * a.ldbx + col);                 \
                }                                                                                             \
            }                                                                                                 \
        }
        if (HOIST) { C2_EPI_LOAD(0) }
        // (CMP: ko[] = the live offsets of this batch, taken from the mask; KT = none)
        constexpr int NKO = !CMP ? 1 : (ST >= 4 ? KB : 2 * U);
        auto batch = [&](const int m0, const int (&ko)[NKO]) __attribute__((always_inline)) {
            uint4 rlo[U], rhi[U];
            int boff[U], idxv[U], c8v[U];
            // Round 3 (ISA review): the kernel-map entries of the whole batch are read from LDS back to back and unconditionally
            // (a clamped slot: a conditional read put an exec-masked branch and a full LDS wait in front of EVERY gather -- eight
            // serialized LDS round trips per batch), the row offset is one unsigned 32 x 32 -> 64 multiply-add (the signed
            // long long form took three), and the weight element of slot s is simply s * NT * 16 + r (k * S + c8 == s).
            int lidx[U];
#pragma unroll
            for (int u = 0; u < U; u++) {
                int s = 4 * (m0 + u) + g, k;
                bool ok;
                if constexpr (CMP && ST < 4) {
                    // 16 input channels: a step is two live offsets (lane groups 0-1 the first, 2-3 the second)
                    k = (g >> 1) ? ko[(2 * u + 1) % NKO] : ko[(2 * u) % NKO];
                    c8v[u] = g & 1;
                    ok = k < KT;
                    s = k * ST + c8v[u];
                } else if (ST >= 4) {
                    // static shapes with >= 32 input channels: a step stays inside ONE offset (here m0 is the first OFFSET of the
                    // batch; the channel group is a constant per lane group; 136 channels run 5 steps per offset, the last one
                    // with a single live lane group)
                    k = CMP ? ko[(u / Q) % NKO] : m0 + u / Q;
                    c8v[u] = 4 * (u % Q) + g;
                    ok = (k < KT) && (c8v[u] < ST);
                    s = k * ST + c8v[u];
                } else {
                    k = ST ? s / (ST ? ST : 1) : (int)(__umul24((unsigned int)s, a.inv) >> 16);      // (24-bit multiplies: full rate)
                    c8v[u] = s - (int)__umul24((unsigned int)k, (unsigned int)S);
                    ok = (m0 + u < nsteps) && (k < K);
                }
                lidx[u] = ok ? rK + k : C2_TBL_SENT;                              // (the sentinel slot holds -1)
                boff[u] = ok ? s * (NT * 16) + r : r;                 // weight ELEMENT index (16 B bf16 / 32 B fp32 each)
            }
#pragma unroll
            for (int u = 0; u < U; u++) idxv[u] = tblS[lidx[u]];
            // raw buffer gathers: an absent neighbour (-1) lands beyond the buffer's extent and the hardware returns zeros
            // without a memory request -- no exec-masked branch, no zero fill and no 64-bit address per gather
            // (inputs beyond 2 GiB are refused by the host: 32-bit offsets, absent rows at offset 2^31)
#pragma unroll
            for (int u = 0; u < U; u++) {
                if (CMP ? (ko[(ST >= 4 ? u / Q : 2 * u) % NKO] >= KT)
                        : ((ST > 0 && ST < 4 && m0 + u >= NSTEPS_T) || (ST >= 4 && m0 + u / Q >= KT))) {   // (folded where m0 is a constant; wave-uniform otherwise)
                    rlo[u] = make_uint4(0u, 0u, 0u, 0u); rhi[u] = rlo[u]; continue;
                }
                const unsigned int off = idxv[u] >= 0 ? __umul24((unsigned int)idxv[u], xrowb) + (unsigned int)c8v[u] * (XBF ? 16u : 32u) : 0x80000000u;
                rlo[u] = c2_from_u32x4(__builtin_amdgcn_raw_buffer_load_b128(rx, off, 0, 0));
                if (!XBF) rhi[u] = c2_from_u32x4(__builtin_amdgcn_raw_buffer_load_b128(rx, off + 16u, 0, 0));
                else rhi[u] = rlo[u];
            }
            if (WLDS || F32M) {
                __builtin_amdgcn_sched_barrier(0);   // every gather is in flight before the first conversion
                // (steps beyond nsteps gathered nothing: their products add zero, and without a branch per step the weight
                // fragments of the batch are read ahead of the products instead of one LDS round trip in front of each)
#pragma unroll
                for (int u = 0; u < U; u++) {
                    if (CMP ? (ko[(ST >= 4 ? u / Q : 2 * u) % NKO] >= KT)
                            : ((ST > 0 && ST < 4 && m0 + u >= NSTEPS_T) || (ST >= 4 && m0 + u / Q >= KT))) continue;
#pragma unroll
                    for (int n = 0; n < NT; n++) {
                        uint4 wl, wh;
                        c2_wload<F32M>(Wb, boff[u] + n * 16, wl, wh);
                        // transposed product: D[m = channel][n = row] += W^T[channel][k] * X^T[k][row]
                        acc[n] = c2_mma<XBF, F32M>(acc[n], wl, wh, rlo[u], rhi[u]);
                    }
                }
            } else {
                // weights from global memory (L2)
                if (NT <= 4) {   // the fragments of step u + 1 are requested before the MFMAs of step u
                    uint4 wnext[NT];
#pragma unroll
                    for (int n = 0; n < NT; n++) wnext[n] = *((const uint4 *)Wb + boff[0] + n * 16);
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int u = 0; u < U; u++) {
                        if (m0 + u < nsteps) {   // wave-uniform
                            uint4 wcur[NT];
#pragma unroll
                            for (int n = 0; n < NT; n++) wcur[n] = wnext[n];
                            if (u + 1 < U && m0 + u + 1 < nsteps) {
#pragma unroll
                                for (int n = 0; n < NT; n++) wnext[n] = *((const uint4 *)Wb + boff[u + 1] + n * 16);
                            }
                            const bf16x8_t A = c2_cvt_raw<XBF>(rlo[u], rhi[u]);
#pragma unroll
                            for (int n = 0; n < NT; n++)
                                acc[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, wcur[n]), A, acc[n], 0, 0, 0);
                        }
                    }
                } else {         // (registers) the fragments of a step in batches of 4: one round trip per batch
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int u = 0; u < U; u++) {
                        if (m0 + u < nsteps) {   // wave-uniform
                            const bf16x8_t A = c2_cvt_raw<XBF>(rlo[u], rhi[u]);
#pragma unroll
                            for (int nb = 0; nb < NT; nb += 4) {
                                uint4 wv[4];
#pragma unroll
                                for (int j = 0; j < 4; j++) if (nb + j < NT) wv[j] = *((const uint4 *)Wb + boff[u] + (nb + j) * 16);
                                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                                for (int j = 0; j < 4; j++)
                                    if (nb + j < NT) acc[nb + j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, wv[j]), A, acc[nb + j], 0, 0, 0);
                            }
                        }
                    }
                }
            }
        };
        const int ko0[NKO] = {0};
        if constexpr (CMP) {
            unsigned int m = kmask;
#pragma unroll 1
            while (m) {      // (wave-uniform: the mask lives in scalar registers)
                int ko[NKO];
#pragma unroll
                for (int j = 0; j < NKO; j++) { ko[j] = m ? (int)__builtin_ctz(m) : KT; m &= m - 1u; }
                batch(0, ko);
            }
        } else if constexpr (ST >= 4 && (KT * Q > 56 || NT >= 3)) {   // (the stem: 135 steps; >= 48 output channels -- unrolled completely they spill)
#pragma unroll 1
            for (int k0 = 0; k0 < KT; k0 += KB) batch(k0, ko0);
        } else if constexpr (ST >= 4) {
#pragma unroll
            for (int k0 = 0; k0 < KT; k0 += KB) batch(k0, ko0);
        } else if constexpr (ST > 0) {
#pragma unroll
            for (int m0 = 0; m0 < NSTEPS_T; m0 += U) batch(m0, ko0);
        } else {
            for (int m0 = 0; m0 < nsteps; m0 += U) batch(m0, ko0);
        }
        // D layout: column (= output row) lane & 15, rows (= channels) (lane >> 4) * 4 + q
#pragma unroll
        for (int n0 = 0; n0 < NT; n0 += NB) {
            if (!HOIST) { C2_EPI_LOAD(n0) __builtin_amdgcn_sched_barrier(0); }
#pragma unroll
            for (int j = 0; j < NB; j++) {
                const int n = n0 + j;
                if (n >= NT) continue;
                const int col = n * 16 + g * 4;
                if (urow < a.Mout && col < a.Cout) {   // Cout % 4 == 0 (checked on the host)
                    f32x4 vv = acc[n];
                    if (a.res) vv += e_res[j];
                    f32x4 *o = (f32x4 *)(a.out + (long long)urow * a.ldo + col);
                    if (a.accum) vv += e_out[j];
                    if (a.bnx) {
                        f32x4 xh;
#pragma unroll
                        for (int q = 0; q < 4; q++) {
                            const float4 bp = bnS[col + q];
                            xh[q] = (e_bnx[j][q] - bp.x) * bp.y;
                            if (a.bn_relu && fmaf(xh[q], bp.z, bp.w) <= 0.f) vv[q] = 0.f;
                        }
                        if (a.obf16) *(uint2 *)((unsigned short *)a.out + (long long)urow * a.ldo + col) = make_uint2(pack2bf2(vv[0], vv[1]), pack2bf2(vv[2], vv[3]));
                        else *o = vv;
                        ssum[n] += vv; ssq[n] += vv * xh;
                    } else {
                        if (a.obf16) *(uint2 *)((unsigned short *)a.out + (long long)urow * a.ldo + col) = make_uint2(pack2bf2(vv[0], vv[1]), pack2bf2(vv[2], vv[3]));
                        else *o = vv;
                        ssum[n] += vv; ssq[n] += vv * vv;
                    }
                }
            }
        }
#undef C2_EPI_LOAD
        __builtin_amdgcn_wave_barrier();   // tblS is rewritten by the next tile
    }
#undef C2_LOAD_TBL
    if (a.part) {   // per-workgroup BatchNorm partials (fixed order: deterministic)
#pragma unroll
        for (int n = 0; n < NT; n++) {
#pragma unroll
            for (int q = 0; q < 4; q++) {
                float s1 = ssum[n][q], s2 = ssq[n][q];
#pragma unroll
                for (int o = 1; o < 16; o <<= 1) { s1 += __shfl_xor(s1, o); s2 += __shfl_xor(s2, o); }
                if (r == 0) { redS[wave * 2 * NT * 16 + n * 16 + g * 4 + q] = s1; redS[wave * 2 * NT * 16 + NT * 16 + n * 16 + g * 4 + q] = s2; }
            }
        }
        __syncthreads();
        if (t < 2 * NT * 16) {
            float s = 0.f;
#pragma unroll
            for (int w = 0; w < NW; w++) s += redS[w * 2 * NT * 16 + t];
            a.part[(long long)b * 2 * NT * 16 + t] = s;
            if (a.part2) unsafeAtomicAdd(&a.part2[(b % D3_P2_ROWS) * 2 * NT * 16 + t], (double)s);
        }
    }
}
template <int NT, bool WLDS, bool XBF, int NW = 4, bool F32M = false, int KT = 0, int ST = 0, bool T16 = false>
__global__ __launch_bounds__(64 * NW) __attribute__((amdgpu_waves_per_eu(NW == 4 ? C2_OCC(NT, XBF) : 4, NW == 4 ? 8 : 4))) void spconv_fwd2_kernel(const Conv2Args a) {
    spconv_fwd2_body<NT, WLDS, XBF, NW, F32M, KT, ST, T16>(a);
}
// the statically shaped instances (K = 27, bf16 rows, weights in LDS) with the tile's dead offsets dropped (CMP above)
template <int NT, int NW, int ST, bool T16>
__global__ __launch_bounds__(64 * NW) __attribute__((amdgpu_waves_per_eu(NW == 4 ? C2_OCC(NT, true) : 4, NW == 4 ? 8 : 4))) void spconv_fwd2_c_kernel(const Conv2Args a) {
    spconv_fwd2_body<NT, true, true, NW, false, 27, ST, T16, true>(a);
}
// Workgroup-per-tile kernel (few-row levels): grid = (16-row tiles, column groups of NTW 16-wide tiles).  The
// W = blockDim.x/64 waves split the MFMA steps of the tile, their accumulators are summed through LDS in wave order,
// and the workgroup owns complete output columns: no atomics, no cross-workgroup reduction, deterministic.
template <int NTW, bool XBF, bool F32M = false>
__global__ __launch_bounds__(1024) void spconv_fwd2_split_kernel(const Conv2Args a) {
    static_assert(!(F32M && XBF), "fp32 MFMA needs fp32 gathers");
    constexpr int U = 4;
    constexpr int CW = NTW * 16;                     // output columns of this workgroup
    constexpr bool SMALL = !F32M && NTW <= (XBF ? 3 : 2);     // register budget: 128 VGPRs at 1024 threads
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, r = lane & 15, g = lane >> 4;
    const int W = blockDim.x >> 6, K = a.K, S = a.S;
    int *tblS = (int *)smem;                         // 16*27 ints
    int *actS = tblS + C2_TBL_INTS;                  // 32 ints
    unsigned int *kmaskS = (unsigned int *)(actS + 32);   // 1 (+3 pad)
    float *redS = (float *)(kmaskS + 4);             // W * NTW*256 floats
    float *finS = redS + (size_t)W * NTW * 256;      // 16 x NTW*16: stored values
    float *fin2S = finS + 16 * NTW * 16;             // 16 x NTW*16: second statistic (v*v, or g*xhat)
    const int row0 = blockIdx.x * 16, n0 = blockIdx.y * NTW;
    // The kernel is a short chain of dependent memory round trips (kernel-map rows -> gathers -> epilogue operands), so
    // everything whose address is known up front is requested up front: the kernel-map rows and, for narrow column
    // groups, the epilogue operands of this thread's output elements e = t + i * blockDim.x (blockDim.x >= 256: at most
    // NTW of them).  Wide groups request the epilogue operands in one batch at the epilogue instead (registers).
    float e_res[NTW], e_out[NTW], e_bnx[NTW], e_mean[NTW], e_var[NTW], e_gam[NTW], e_bet[NTW];
#define C2S_EPI_LOAD                                                                                          \
    _Pragma("unroll") for (int i = 0; i < NTW; i++) {                                                         \
        const int e = t + i * (int)blockDim.x;                                                                \
        const int row = e / CW, cl = e - row * CW;                                                            \
        const int u = row0 + row, col = n0 * 16 + cl;                                                         \
        e_res[i] = 0.f; e_out[i] = 0.f; e_bnx[i] = 0.f; e_mean[i] = 0.f; e_var[i] = 1.f; e_gam[i] = 0.f; e_bet[i] = 0.f; \
        if (e < 16 * CW && u < a.Mout && col < a.Cout) {                                                      \
            if (a.res) e_res[i] = a.res[(long long)u * a.ldr + col];                                          \
            if (a.accum) e_out[i] = a.out[(long long)u * a.ldo + col];                                        \
            if (a.bnx) {                                                                                      \
                {   /* fp32, or bf16 (round 6): ONE 32-bit load either way -- the word that holds the element */              \
                    const long long bi_ = (long long)u * a.ldbx + col;                                                \
                    const unsigned int bw_ = ((const unsigned int *)a.bnx)[a.bnx_bf16 ? (bi_ >> 1) : bi_];            \
                    e_bnx[i] = __uint_as_float(a.bnx_bf16 ? ((bi_ & 1) ? (bw_ & 0xFFFF0000u) : (bw_ << 16)) : bw_);   \
                }                                                                                                     \
                e_mean[i] = a.bn_mean[col]; e_var[i] = a.bn_var[col]; \
                if (a.bn_relu) { e_gam[i] = a.bn_gamma[col]; e_bet[i] = a.bn_beta[col]; }                     \
            }                                                                                                 \
        }                                                                                                     \
    }
    int v[2];
    const long long base = (long long)row0 * K, lim = (long long)a.Mout * K;
#pragma unroll
    for (int it = 0; it < 2; it++) {   // blockDim.x >= 256 and 16*K <= 432
        const int e = t + it * blockDim.x;
        v[it] = -1;
        if (e < 16 * K && base + e < lim) v[it] = a.tbl ? a.tbl[base + e] : (int)(base + e);
    }
    if (SMALL) { C2S_EPI_LOAD }
    if (t == 0) *kmaskS = 0u;
    __syncthreads();
    {
        unsigned int bits = 0u;
#pragma unroll
        for (int it = 0; it < 2; it++) {
            const int e = t + it * blockDim.x;
            if (e < 16 * K) {
                tblS[e] = v[it];
                if (v[it] >= 0) bits |= 1u << (e - (int)(((unsigned int)e * a.invK) >> 16) * K);
            }
        }
        if (bits) atomicOr(kmaskS, bits);
    }
    __syncthreads();
    const unsigned int kmask = *kmaskS;
    const int na = __popc(kmask);
    if (t < K && ((kmask >> t) & 1u)) actS[__popc(kmask & ((1u << t) - 1u))] = t;
    __syncthreads();
    f32x4 acc[NTW];
#pragma unroll
    for (int n = 0; n < NTW; n++) acc[n] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const int nsteps = (na * S + 3) >> 2;
    for (int m0 = wave; m0 < nsteps; m0 += W * U) {
        uint4 rlo[U], rhi[U];
        int boff[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int m = m0 + u * W;
            const int s = 4 * m + g;
            const int i = (int)(((unsigned int)s * a.inv) >> 16);
            const int c8 = s - i * S;
            const bool ok = (m < nsteps) && (i < na);
            const int k = actS[ok ? i : 0];
            const int idx = ok ? tblS[r * K + k] : -1;
            boff[u] = ((k * S + (ok ? c8 : 0)) * a.NT + n0) * 16 + r;      // weight ELEMENT index
            rlo[u] = make_uint4(0u, 0u, 0u, 0u); rhi[u] = rlo[u];
            if (idx >= 0) c2_load_raw<XBF>(a.x, (long long)idx * a.ldx + c8 * 8, rlo[u], rhi[u]);
        }
        if (SMALL) {
            // gathers and all weight fragments of the batch in flight together: one round trip per batch
            uint4 wv[U][NTW];
#pragma unroll
            for (int u = 0; u < U; u++)
#pragma unroll
                for (int n = 0; n < NTW; n++) {
                    wv[u][n] = make_uint4(0u, 0u, 0u, 0u);
                    if (m0 + u * W < nsteps && n0 + n < a.NT) wv[u][n] = *((const uint4 *)a.Wp + boff[u] + n * 16);
                }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int u = 0; u < U; u++) {
                if (m0 + u * W < nsteps) {
                    const bf16x8_t A = c2_cvt_raw<XBF>(rlo[u], rhi[u]);
#pragma unroll
                    for (int n = 0; n < NTW; n++)
                        if (n0 + n < a.NT) acc[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A, __builtin_bit_cast(bf16x8_t, wv[u][n]), acc[n], 0, 0, 0);
                }
            }
        } else {
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int u = 0; u < U; u++) {
                if (m0 + u * W < nsteps) {
                    uint4 wv[NTW], wh[NTW];
#pragma unroll
                    for (int n = 0; n < NTW; n++) {
                        wv[n] = make_uint4(0u, 0u, 0u, 0u); wh[n] = wv[n];
                        if (n0 + n < a.NT) c2_wload<F32M>(a.Wp, boff[u] + n * 16, wv[n], wh[n]);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                    if (F32M) {      // (not transposed here: first operand = gathered rows, second = weights)
#pragma unroll
                        for (int n = 0; n < NTW; n++)
                            if (n0 + n < a.NT) acc[n] = c2_mma<false, true>(acc[n], rlo[u], rhi[u], wv[n], wh[n]);
                    } else {
                    const bf16x8_t A = c2_cvt_raw<XBF>(rlo[u], rhi[u]);
#pragma unroll
                    for (int n = 0; n < NTW; n++)
                        if (n0 + n < a.NT) acc[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A, __builtin_bit_cast(bf16x8_t, wv[n]), acc[n], 0, 0, 0);
                    }
                }
            }
        }
    }
#pragma unroll
    for (int n = 0; n < NTW; n++)
#pragma unroll
        for (int q = 0; q < 4; q++) redS[(wave * NTW * 4 + n * 4 + q) * 64 + lane] = acc[n][q];
    if (!SMALL) { C2S_EPI_LOAD }
    __syncthreads();
    // final tile: element e = row * CW + col, summed in wave order
#pragma unroll
    for (int i = 0; i < NTW; i++) {
        const int e = t + i * (int)blockDim.x;
        if (e >= 16 * CW) continue;
        const int row = e / CW, cl = e - row * CW;
        const int n = cl >> 4, ln = (row >> 2) * 16 + (cl & 15), q = row & 3;
        float v = 0.f, w2 = 0.f;
        for (int w = 0; w < W; w++) v += redS[(w * NTW * 4 + n * 4 + q) * 64 + ln];
        const int u = row0 + row, col = n0 * 16 + cl;
        if (u < a.Mout && col < a.Cout) {
            if (a.res) v += e_res[i];
            if (a.accum) v += e_out[i];
            if (a.bnx) {
                const float xh = (e_bnx[i] - e_mean[i]) * rsqrtf(e_var[i] + a.bn_eps);
                if (a.bn_relu && fmaf(xh, e_gam[i], e_bet[i]) <= 0.f) v = 0.f;
                w2 = v * xh;
            } else w2 = v * v;
            if (a.obf16) ((unsigned short *)a.out)[(long long)u * a.ldo + col] = (unsigned short)(pack2bf2(v, 0.f) & 0xFFFFu);
            else a.out[(long long)u * a.ldo + col] = v;
        } else { v = 0.f; w2 = 0.f; }
        finS[e] = v; fin2S[e] = w2;
    }
#undef C2S_EPI_LOAD
    if (a.part) {
        __syncthreads();
        if (t < 2 * CW) {
            const int cl = (t < CW) ? t : t - CW;
            float s = 0.f;
            for (int row = 0; row < 16; row++) s += (t < CW) ? finS[row * CW + cl] : fin2S[row * CW + cl];
            if (n0 * 16 + cl < a.NT * 16) {
                float *pp = &a.part[(long long)blockIdx.x * 2 * a.NT * 16 + (t < CW ? 0 : a.NT * 16) + n0 * 16 + cl];
                *pp = s;
                if (a.part2) unsafeAtomicAdd(&a.part2[(long long)(blockIdx.x % D3_P2_ROWS) * 2 * a.NT * 16 + (t < CW ? 0 : a.NT * 16) + n0 * 16 + cl], (double)s);
            }
        }
    }
}

#define C2_NW16_MAXNT 4      // 16-wave variants are instantiated for <= 4 column tiles
#define C2_GRIDCAP 1024      // persistent workgroups per convolution launch; levels of fewer 16-row tiles run the workgroup-per-tile kernel
int d3_conv_ncu() {   // (conv.h)
    static int n = 0;
    if (!n) { int dev = 0; hipDeviceProp_t pr; n = (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&pr, dev) == hipSuccess && pr.multiProcessorCount > 0) ? pr.multiProcessorCount : 256; }
    return n;
}
struct Conv2Plan { int split, W, grid, wlds, ntw, gy, nw; size_t lds; };

static Conv2Plan conv2_plan(int Mout, int K, int Cin, int Cout, bool f32 = false) {
    Conv2Plan p;
    const int NT = (Cout + 15) / 16, ntiles = (Mout + 15) / 16;
    const size_t wbytes = (size_t)K * (Cin / 8) * NT * (f32 ? 512 : 256);
    p.ntw = NT; p.gy = 1; p.nw = 4;
    if (ntiles >= 1024) {
        p.split = 0; p.W = 1;
        // 16 waves around ONE LDS copy of a large weight set (one workgroup per CU), 4 waves per workgroup otherwise
        constexpr size_t big_from = (size_t)24 * 1024;      // packed weights of at least this many bytes: 16 waves share one LDS copy
        const size_t lds_max = (size_t)160 * 1024;
        if (NT <= C2_NW16_MAXNT && wbytes >= big_from && wbytes + C2_WAVE_LDS_BYTES(NT, 16) <= lds_max && wbytes + C2_WAVE_LDS_BYTES(NT, 16) <= 160 * 1024)
            p.nw = 16;
        const int ntg = (ntiles + p.nw - 1) / p.nw;
        int cap = C2_GRIDCAP;
        if (p.nw == 16) cap = d3_conv_ncu();      // LDS admits one such workgroup per CU
        const int per = (ntg + cap - 1) / cap;
        p.grid = (ntg + per - 1) / per;
        p.wlds = (p.nw == 16 || wbytes + C2_WAVE_LDS_BYTES(NT, 4) <= 72 * 1024) ? 1 : 0;
        p.lds = (p.wlds ? wbytes : 0) + C2_WAVE_LDS_BYTES(NT, p.nw);
    } else {
        p.split = 1; p.grid = ntiles; p.wlds = 0;
        // few tiles: one column tile per workgroup (the gather is repeated per column group, from L2)
        if (ntiles < 256) p.ntw = 1; else if (NT > 4) p.ntw = (NT + 1) / 2;
        if (p.ntw > 7) p.ntw = 7;
        // (round 6: the 4-tile instance of the workgroup-per-tile kernel spills at its 128-register budget since the last-block finalize left
        // its tail -- 78 registers before, 128 + 64 B of scratch after, 13 -> 20 us per launch; the 5-tile instance, 86 registers, serves 64
        // columns with its fifth tile idle)
        if (p.ntw == 4) p.ntw = 5;
        p.gy = (NT + p.ntw - 1) / p.ntw;
        const int steps = K * (Cin / 8) / 4 + 1;     // upper bound of MFMA steps per tile
        int W = ntiles * p.gy >= 512 ? 4 : 8;
        if (ntiles * p.gy < 128) W = 16;
        while (W > 4 && W * 2 > steps) W >>= 1;
        p.W = W;
        p.lds = (size_t)(C2_TBL_INTS + 32 + 4) * 4 + (size_t)W * p.ntw * 1024 + (size_t)p.ntw * 2048;
    }
    return p;
}

// rows of the BatchNorm partial table a forward / data-gradient call may write: the larger of the two kernels that can serve the
// shape (which one runs depends on the tables the call is handed); d3_spconv_last_nparts() says how many the call did write
extern "C" int d3_spconv_fwd2_nparts(int Mout, int K, int Cin, int Cout) {
    const int g2 = conv2_plan(Mout, K, Cin, Cout).grid, g3 = K == 27 ? d3_spconv_fwd3_nparts(Mout, Cin, Cout) : 0;
    return g2 > g3 ? g2 : g3;
}
// flags: D3_CONV_F32 changes the weight footprint and with it the workgroup shape
extern "C" int d3_spconv_fwd2_nparts_ex(int Mout, int K, int Cin, int Cout, int flags) {
    const int g2 = conv2_plan(Mout, K, Cin, Cout, (flags & D3_CONV_F32) != 0).grid;
    const int g3 = (K == 27 && !(flags & D3_CONV_F32)) ? d3_spconv_fwd3_nparts(Mout, Cin, Cout) : 0;
    return g2 > g3 ? g2 : g3;
}

// which kernel d3_spconv_fwd2* runs for this shape: out[6] = {split (1: spconv_fwd2_split_kernel), waves per workgroup,
// grid.x, weights resident in LDS, column tiles per workgroup, grid.y}
extern "C" int d3_spconv_fwd2_plan(int Mout, int K, int Cin, int Cout, int *out) {
    if (!out || K < 1 || K > C2_MAXK || Cin < 8 || (Cin & 7) || Cout < 1 || Cout > 224) return D3_ERR_ARG;
    const Conv2Plan p = conv2_plan(Mout, K, Cin, Cout);
    out[0] = p.split; out[1] = p.split ? p.W : p.nw; out[2] = p.grid; out[3] = p.wlds; out[4] = p.ntw; out[5] = p.gy;
    return 0;
}

#include <atomic>
static std::atomic<long long> g_t16_launches{0};       // launches that read a 16-bit kernel map (tests: the path really ran)
extern "C" long long d3_spconv_t16_launches(void) { return g_t16_launches.load(); }
void d3_conv_count_t16() { g_t16_launches++; }         // (conv.h: the weight gradients' launches, wgrad.hip)
// inst[7] (the caller's): template arguments of the instance a launch_fwd2* call runs: {NT, WLDS, XBF, NW, F32M, KT, ST} for
// spconv_fwd2_kernel, {NTW, XBF, F32M} for spconv_fwd2_split_kernel -- the profiling record names the kernel as rocprofv3 prints it
static inline void c2_inst(int *inst, int a0, int a1, int a2, int a3, int a4, int a5, int a6) {
    inst[0] = a0; inst[1] = a1; inst[2] = a2; inst[3] = a3; inst[4] = a4; inst[5] = a5; inst[6] = a6;
}
// one launch of an instance: its dynamic-LDS limit, the launch, the launch check
template <auto Kernel>
static int c2_launch(const Conv2Args &a, dim3 grid, int threads, size_t lds, int lds_limit, hipStream_t s) {
    if (const int rc = d3_allow_lds<Kernel>(lds_limit)) return rc;
    Kernel<<<grid, threads, lds, s>>>(a);
    D3_LAUNCH_CHECK();
    return 0;
}
template <int NT>
static int launch_fwd2_f32(const Conv2Args &a, const Conv2Plan &p, int *inst, hipStream_t s) {
    if constexpr (NT <= C2_NW16_MAXNT) {
        if (p.nw == 16) {
            c2_inst(inst, NT, 1, 0, 16, 1, 0, 0);
            return c2_launch<spconv_fwd2_kernel<NT, true, false, 16, true>>(a, p.grid, 1024, p.lds, 160 * 1024, s);
        }
    }
    c2_inst(inst, NT, p.wlds ? 1 : 0, 0, 4, 1, 0, 0);
    return d3_with_bools([&](auto wlds) { return c2_launch<spconv_fwd2_kernel<NT, wlds.value, false, 4, true>>(a, p.grid, 256, p.lds, 96 * 1024, s); },
                         p.wlds != 0);
}
// the statically shaped instances (K = 27, bf16 rows, weights in LDS)
template <int NT, int NW, int ST>
static int launch_fwd2_static(const Conv2Args &a, const Conv2Plan &p, int *inst, hipStream_t s) {
    // the stem (136 -> 16: five products per offset) drops the offsets no row of a 16-row tile has before its reduction loop
    // (spconv_fwd2_c_kernel: 266 -> 231 us at 649 k rows; for the 16 / 32-channel instances the mask pass cost more than the dropped
    // steps saved -- measured in round 5 -- and they run spconv_fwd3_kernel on the lane table since round 6 anyway)
    if constexpr (ST == 17) {
        // (the plain instance of the stem's shape stays in the code object: its limit is raised as before, nothing launches it)
        if (const int rc = d3_allow_lds<spconv_fwd2_kernel<NT, true, true, NW, false, 27, ST>>(160 * 1024)) return rc;
        c2_inst(inst, NT, 1, 1, NW, 0, 27, ST + (a.tbl16 ? 1000 : 0) + 4000);     // (+ 4000: spconv_fwd2_c_kernel, see bench.py's kernel naming)
        if (a.tbl16) g_t16_launches++;
        return d3_with_bools([&](auto t16) { return c2_launch<spconv_fwd2_c_kernel<NT, NW, ST, t16.value>>(a, p.grid, 64 * NW, p.lds, 160 * 1024, s); },
                             a.tbl16 != nullptr);
    }
    c2_inst(inst, NT, 1, 1, NW, 0, 27, ST);
    return c2_launch<spconv_fwd2_kernel<NT, true, true, NW, false, 27, ST>>(a, p.grid, 64 * NW, p.lds, 160 * 1024, s);
}
template <int NT>
static int launch_fwd2(const Conv2Args &a, const Conv2Plan &p, int *inst, hipStream_t s) {
    if (a.f32) return launch_fwd2_f32<NT>(a, p, inst, s);
    if (a.xbf16 && a.K == 27 && p.wlds) {
        if constexpr (NT == 1) {
            if (a.S == 2 && p.nw == 4) return launch_fwd2_static<1, 4, 2>(a, p, inst, s);      // 16 -> 16
            if (a.S == 4 && p.nw == 16) return launch_fwd2_static<1, 16, 4>(a, p, inst, s);    // 32 -> 16
            if (a.S == 17 && p.nw == 16) return launch_fwd2_static<1, 16, 17>(a, p, inst, s);  // the stem: 134 (+2) -> 16
        }
        if constexpr (NT == 2) {
            if (a.S == 2 && p.nw == 16) return launch_fwd2_static<2, 16, 2>(a, p, inst, s);    // 16 -> 32
            if (a.S == 4 && p.nw == 16) return launch_fwd2_static<2, 16, 4>(a, p, inst, s);    // 32 -> 32
            if (a.S == 8 && p.nw == 16) return launch_fwd2_static<2, 16, 8>(a, p, inst, s);    // 64 -> 32
        }
        // (48 -> 48 with the offset loop rolled: measured no faster than the generic instance -- 36 k rows are one tile per wave)
        // (32 -> 64 spills at 128 registers even with the rolled loop: generic instance)
    }
    if constexpr (NT <= C2_NW16_MAXNT) {
        if (p.nw == 16) {      // (16 waves: the weights are in LDS always)
            c2_inst(inst, NT, 1, a.xbf16 ? 1 : 0, 16, 0, 0, 0);
            return d3_with_bools([&](auto xbf) { return c2_launch<spconv_fwd2_kernel<NT, true, xbf.value, 16>>(a, p.grid, 1024, p.lds, 160 * 1024, s); },
                                 a.xbf16 != 0);
        }
    }
    c2_inst(inst, NT, p.wlds ? 1 : 0, a.xbf16 ? 1 : 0, 4, 0, 0, 0);
    return d3_with_bools([&](auto wlds, auto xbf) { return c2_launch<spconv_fwd2_kernel<NT, wlds.value, xbf.value>>(a, p.grid, 256, p.lds, 96 * 1024, s); },
                         p.wlds != 0, a.xbf16 != 0);
}
template <int NTW>
static int launch_fwd2_split(const Conv2Args &a, const Conv2Plan &p, int *inst, hipStream_t s) {
    c2_inst(inst, NTW, a.f32 ? 0 : (a.xbf16 ? 1 : 0), a.f32 ? 1 : 0, -1, 0, 0, 0);
    const dim3 grid(p.grid, p.gy);
    if (a.f32) return c2_launch<spconv_fwd2_split_kernel<NTW, false, true>>(a, grid, p.W * 64, p.lds, 128 * 1024, s);      // (fp32 MFMA needs fp32 gathers)
    return d3_with_bools([&](auto xbf) { return c2_launch<spconv_fwd2_split_kernel<NTW, xbf.value>>(a, grid, p.W * 64, p.lds, 128 * 1024, s); },
                         a.xbf16 != 0);
}

// internal forward / data-gradient entry (conv.h)
int d3_conv2_run(const void *x, int ldx, const int *tbl, const void *Wp, float *out, int ldo, const float *res, int ldr, float *part,
                 int Min, int Mout, int K, int Cin, int Cout, int flags, const ConvBn *bn, const ConvExtras &ex, int *nparts, void *stream) {
    D3_CLEAR();
    *nparts = 0;
    const void *tbl16 = ex.tbl16, *tblq = ex.tblq;
    double *part2 = ex.part2;
    if (Mout <= 0) return 0;
    if (K < 1 || K > C2_MAXK || Cin < 8 || (Cin & 7) || Cout < 1 || Cout > 224) return D3_ERR_ARG;
    if (tbl == nullptr && K != 1) return D3_ERR_ARG;
    const int xbf16 = (flags & D3_CONV_XBF16) ? 1 : 0;
    const int f32 = (flags & D3_CONV_F32) ? 1 : 0;
    if (f32 && xbf16) return D3_ERR_ARG;      // the reference-precision path gathers fp32 rows
    if ((xbf16 && (ldx & 7)) || (!xbf16 && (ldx & 3)) || ldx < Cin || ldo < Cout) return D3_ERR_ARG;
    if ((Cout & 3) || (ldo & 3) || (res && (ldr & 3))) return D3_ERR_ARG;   // float4 epilogue
    hipStream_t s = d3_stream(stream);
    // round 6: the big levels' K = 27 layers on the lane table (spconv3.hip) -- bf16 rows, no accumulate-into
    if (tblq && tbl && K == 27 && xbf16 && !f32 && !(flags & D3_CONV_ACCUM) && d3_tune(D3T_C3) != 0 &&
        Mout >= C2_GRIDCAP * 16 && d3_spconv_fwd3_nparts(Mout, Cin, Cout) > 0 && !(bn && res)) {
        const int rc3 = d3_conv3_run(x, ldx, tblq, Wp, out, ldo, res, ldr, part, part ? part2 : nullptr, Min, Mout, Cin, Cout,
                                     (flags & D3_CONV_OUTBF16) ? 1 : 0, bn, nparts, s);
        if (rc3 != D3_ERR_ARG) return rc3;
    }
    Conv2Args a;
    a.x = x; a.tbl = tbl; a.Wp = (const unsigned short *)Wp; a.out = out; a.res = res; a.part = part;
    a.part2 = part ? part2 : nullptr;
    a.ldx = ldx; a.ldo = ldo; a.ldr = ldr; a.Mout = Mout; a.K = K; a.Cout = Cout; a.S = Cin / 8;
    a.inv = (65536u + a.S - 1) / a.S;
    a.invK = (65536u + K - 1) / K;
    a.tbl16 = (tbl && tbl16 && K == 27 && !f32 && xbf16) ? (const unsigned int *)tbl16 : nullptr;   // (only the static instances launch with it)
    a.xbf16 = xbf16; a.f32 = f32; a.accum = (flags & D3_CONV_ACCUM) ? 1 : 0; a.ntiles = (Mout + 15) / 16;
    a.obf16 = (flags & D3_CONV_OUTBF16) ? 1 : 0;
    if (a.obf16 && (a.accum || res || f32)) return D3_ERR_ARG;
    {   // the last row of a column view ends after Cin elements; an absent neighbour's offset (2^32 - row bytes + ...) must stay outside
        const unsigned long long elt = xbf16 ? 2ull : 4ull, rowb = (unsigned long long)ldx * elt;
        const unsigned long long xb = Min > 0 ? ((unsigned long long)(Min - 1) * ldx + Cin) * elt : 0ull;
        a.xbytes = (Min > 0 && Min < (1 << 24) && rowb < (1ull << 24) && xb <= 0x7FFFFFFFull) ? (unsigned int)xb : 0u;   // (24-bit row x row-bytes multiply; absent rows address 2 GiB)
    }
    if (bn && (bn->ldx & 3)) return D3_ERR_ARG;
    d3_conv_bn_args(a, bn);
    a.bnx_bf16 = bn ? bn->xbf16 : 0;
    const Conv2Plan p = conv2_plan(Mout, K, Cin, Cout, f32 != 0);
    *nparts = p.grid;
    if (!p.split && a.xbytes == 0u) return D3_ERR_RANGE;   // the wave-per-tile kernel addresses x through a raw buffer: <= 2 GiB, < 2^24 rows
    const double bytes = (xbf16 ? 2.0 : 4.0) * (double)Min * Cin + (a.obf16 ? 2.0 : 4.0) * (double)Mout * Cout + (f32 ? 4.0 : 2.0) * (double)K * Cin * Cout +
                         (tbl ? 4.0 * (double)Mout * K : 0.0) + (res ? 4.0 * (double)Mout * Cout : 0.0);
    void *pr = d3_prof_begin(p.split ? 2 : 0, bytes, 0.0, s);
    int inst[7] = {0, 0, 0, 0, 0, 0, 0};      // filled by launch_fwd2*
    a.NT = (Cout + 15) / 16;
    // workgroup-per-tile: column tiles per workgroup, more than 7 run the 7 instance; wave-per-tile: one instance per count of column tiles
    const int rc = p.split ? d3_with_value<1, 2, 3, 4, 5, 6, 7>(p.ntw > 7 ? 7 : p.ntw, [&](auto ntw) { return launch_fwd2_split<ntw.value>(a, p, inst, s); })
                           : d3_with_value<1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14>(a.NT, [&](auto nt) { return launch_fwd2<nt.value>(a, p, inst, s); });
    if (pr) {
        const int dims[5] = {Min, Mout, K, Cin, Cout};
        for (int i = 0; i < 5; i++) d3_prof_tag(pr, i, dims[i]);
        for (int i = 0; i < 7; i++) d3_prof_tag(pr, 5 + i, inst[i]);
    }
    d3_prof_end(pr, s);
    return rc;
}

extern "C" int d3_spconv_fwd2(const void *x, int ldx, const int *tbl, const void *Wp, float *out, int ldo,
                              const float *res, int ldr, float *part, int Min, int Mout, int K, int Cin, int Cout,
                              int flags, void *stream) {
    return d3_conv2_run(x, ldx, tbl, Wp, out, ldo, res, ldr, part, Min, Mout, K, Cin, Cout, flags, nullptr, ConvExtras{}, &d3_conv_last_nparts, stream);
}

// Data gradient of a BatchNorm -> ReLU -> convolution unit with the BatchNorm backward reductions fused in: the stored
// value is g = (sum_k dy[tbl[u,k]] @ Wk) * relu'(bn(bnx[u])) and part receives (sum g, sum g * xhat) per channel, where
// xhat = (bnx - mean) * rsqrt(var + eps): exactly what d3_bn_relu_bwd's reduction pass computes from a second read of
// x and dy.  bnx (Mout, ldbx) fp32 is the BatchNorm INPUT.
extern "C" int d3_spconv_fwd2_bnbwd(const void *x, int ldx, const int *tbl, const void *Wp, float *out, int ldo, float *part,
                                    const float *bnx, int ldbx, const float *mean, const float *var, const float *gamma,
                                    const float *beta, float eps, int relu, int Min, int Mout, int K, int Cin, int Cout,
                                    int flags, void *stream) {
    ConvBn bn{bnx, mean, var, gamma, beta, ldbx, relu, (flags & D3_CONV_BNXBF16) ? 1 : 0, eps};
    return d3_conv2_run(x, ldx, tbl, Wp, out, ldo, nullptr, 0, part, Min, Mout, K, Cin, Cout, flags, &bn, ConvExtras{}, &d3_conv_last_nparts, stream);
}
