// wgrad.hip -- weight gradients of the sparse convolutions for gfx950: every weight-gradient kernel the second-generation path runs.
//
// Stands in for the weight gradient of MinkowskiConvolution / MinkowskiConvolutionTranspose backward (reference call sites as in
// spconv2.hip: model/common.py:32,38,41,66,90,98; model/pointgroup.py:70):
//
//   dW[k] = sum_u x[tbl[u,k],:]^T dy[u,:]                         tbl: the dense (Mout,K) kernel map of the forward (coordmap.hip)
//
// One entry, d3_conv2_wgrad (conv.h; the C ABI's d3_spconv_wgrad2 is the same call without a 16-bit map), picks one of three kernel
// families per call (wg2_plan_flags); each family's design text stands in front of its kernel:
//   * spconv_wgrad3_kernel: bf16 x, >= 2048 stationary rows and a shape of the instance table WG3_CONFIGS -- the K = 27 and stride-2
//     layers of levels 0 - 2.  Always row-split.
//   * spconv_wgrad2_kernel: everything else (small levels, 1x1, shapes without a wgrad3 instance), and its sibling
//     spconv_wgrad2_wide_kernel for one gathered tile against 5 - 9 stationary tiles at >= 4096 rows (the stem 136 -> 16).
//   * spconv_wgrad_f32_kernel: D3_CONV_F32, the reference's precision (fp32 operands, v_mfma_f32_16x16x4_f32).
// Row splits write partial dW into the caller's workspace; wgrad2_reduce_kernel sums them in split order (deterministic, no atomics)
// unless the caller sums the partials of its layers itself (D3_CONV_NOREDUCE: unet.hip).
// Roofline: HBM.  Algorithmic bytes per launch = e*(Min*Cin + Mout*Cout) + 4*K*CinW*Cout + 4*Ms*K, e = 2 (bf16) / 4
// (fp32): both operands once, dW once, the table once.
#include "conv.h"
#include "prof.h"
#include <cstring>

// ------------------------------------------------------------------------------ weight gradient
// dW[k] = sum_u x[tbl[u,k],:]^T dy[u,:].  One operand is read contiguously ("stationary": rows u of the table),
// the other is gathered through the table; the host gathers the narrower one (the gather is re-done per offset).
//   P[k] (Cg x Cs) = sum_rows G[tbl[row,k],:]^T S[row,:]       MFMA: M = gathered channel, N = stationary channel,
//                                                               reduction = 32 rows per v_mfma_f32_16x16x32_bf16
// Both MFMA operands need 8 consecutive ROWS per lane, i.e. columns of the row-major matrices: each wave stages its
// 32-row chunk transposed in a private LDS region (St once per chunk, shared by all offsets of the pass -- the
// spconv.hip kernel re-read dy once per offset: profiles/r01_h, 85 MB of traffic against 8 MB algorithmic).
// grid = (row splits R, offset groups, tile passes).  A wave keeps 16 accumulator tiles: OPW = 16/TPO offsets x
// TPO tiles per offset; the 4 waves of a workgroup take alternate chunks and are summed through LDS in wave order;
// with R > 1 the workgroup writes a partial dW that wgrad2_reduce_kernel sums in split order (deterministic; no
// atomics).
#ifndef WG2_TARGET_WGS
#define WG2_TARGET_WGS 512   // workgroups per launch the row split aims at
#endif
#ifndef WG2_PART_MB
#define WG2_PART_MB 8         // cap of the partial-dW buffer
#endif
#ifndef WG2_T
#define WG2_T 16        // accumulator tiles per wave (64 AGPRs): occupancy matters more than reuse here
#endif

struct Wg2Args {
    const void *G; const void *Sm; const int *tbl; float *dst;
    int ldg, lds, gbf16, sbf16;
    int Ms, K, mt, nt;          // mt / nt: 16-channel tiles of the gathered / stationary operand
    int Cg8, Cs8;               // 8-channel units per row
    unsigned int invg, invs;    // ceil(65536 / Cg8), ceil(65536 / Cs8)
    int cpw;                    // chunks per workgroup
    int gx, flipk, Cin, Cout;   // gx: the gathered operand is x (P = dW[k]); else it is dy (P = dW[k]^T)
    int rsg, dg, rss, dss;      // row-major LDS images: row stride and 8-row shift in bytes, per operand
    int imgg, imgs;             // image sizes in bytes
};

// Row-major LDS image of a 32-row chunk read back through gfx950's transposing LDS read.  ds_read_b64_tr_b16: the 16 lanes of
// a group address a 4 x 16 bf16 block (lane i: row i/4, columns 4(i%4)..+3) and lane i receives column i, rows 0..3 -- two
// reads give the 8 consecutive rows of one channel that both MFMA operands need, without the 8 x ds_write_b16 transposed
// staging (~80 instructions per MFMA in the first version of this kernel).  A 32-lane half of the wave holds the blocks of
// rows 8g.. and 8(g+1)..: the row stride RSB (a multiple of 32 B, odd multiple where C*2 is a multiple of 128) and a shift
// D per 8 rows keep the eight 32-byte row segments of a half on distinct banks.
typedef short v4s16_t __attribute__((ext_vector_type(4)));
typedef short v8s16_t __attribute__((ext_vector_type(8)));
static void wg2_img(int C8, int *rsb, int *d, int *bytes) {
    int r = (C8 * 16 + 31) / 32 * 32;
    if ((r & 127) == 0) r += 32;
    const int dd = (r & 63) == 0 ? 32 : 128;
    *rsb = r; *d = dd; *bytes = 32 * r + 3 * dd;
}
__device__ __forceinline__ void wg2_put_r(unsigned char *img, int rsb, int d, int c8, int row, uint4 v) {
    *(uint4 *)(img + row * rsb + (row >> 3) * d + c8 * 16) = v;
}
// lane base of the fragment reads: rows 8g + (r>>2) (+4 for the second read), 8 bytes per lane inside the 32-byte tile row
__device__ __forceinline__ int wg2_lane_base(int rsb, int d, int r, int g) { return (8 * g + (r >> 2)) * rsb + g * d + (r & 3) * 8; }
__device__ __forceinline__ bf16x8_t wg2_frag_tr(const unsigned char *img, int lane_base, int rsb, int tile) {
    typedef v4s16_t __attribute__((address_space(3))) *lds_p;
    const v4s16_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_p)(img + lane_base + tile * 32));
    const v4s16_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_p)(img + lane_base + tile * 32 + 4 * rsb));
    const v8s16_t v = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
    return __builtin_bit_cast(bf16x8_t, v);
}

__device__ __forceinline__ uint4 wg2_load8(const void *p, int bf16, long long off) {
    if (bf16) return *(const uint4 *)((const unsigned short *)p + off);
    const float4 f0 = *(const float4 *)((const float *)p + off);
    const float4 f1 = *(const float4 *)((const float *)p + off + 4);
    return make_uint4(pack2bf2(f0.x, f0.y), pack2bf2(f0.z, f0.w), pack2bf2(f1.x, f1.y), pack2bf2(f1.z, f1.w));
}

template <int TPO, int NU>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(WG2_T > 16 ? (NU <= 7 ? 2 : 1) : (NU <= 2 ? 3 : NU <= 7 ? 2 : 1), 8))) void spconv_wgrad2_kernel(const Wg2Args a) {
    constexpr int OPW = WG2_T / TPO;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, r = lane & 15, g = lane >> 4;
    const int K = a.K;
    // per-wave LDS: the two row-major operand images, table chunk 32*K ints
    const size_t gt_bytes = (size_t)a.imgg, st_bytes = (size_t)a.imgs;
    const size_t wave_bytes = gt_bytes + st_bytes + (size_t)32 * C2_MAXK * 4;
    unsigned short *Gt = (unsigned short *)(smem + (size_t)wave * wave_bytes);
    unsigned short *St = (unsigned short *)((unsigned char *)Gt + gt_bytes);
    int *tblW = (int *)((unsigned char *)St + st_bytes);
    const int lbg = wg2_lane_base(a.rsg, a.dg, r, g), lbs = wg2_lane_base(a.rss, a.dss, r, g);
    const int k0 = blockIdx.y * OPW;
    const int tile0 = blockIdx.z * TPO, ntl = a.mt * a.nt;
    const int nchunks = (a.Ms + 31) >> 5;
    const int c_begin = blockIdx.x * a.cpw, c_end = min(nchunks, c_begin + a.cpw);
    // stationary column window of this pass (8-channel units)
    int sc8lo = 0, sc8n = a.Cs8;
    {
        const int tlast = min(ntl, tile0 + TPO) - 1;
        if (tlast >= tile0 && tile0 / a.nt == tlast / a.nt) {
            sc8lo = (tile0 % a.nt) * 2;
            sc8n = min(a.Cs8, (tlast % a.nt + 1) * 2) - sc8lo;
        }
    }

    f32x4 acc[OPW][TPO];
#pragma unroll
    for (int j = 0; j < OPW; j++)
#pragma unroll
        for (int i = 0; i < TPO; i++) acc[j][i] = (f32x4){0.f, 0.f, 0.f, 0.f};

    for (int c = c_begin + wave; c < c_end; c += 4) {
        const int u0 = c * 32;
        // table chunk (32 rows x K, contiguous) -> LDS
        if (a.tbl) {   // loads first, LDS stores after (a rolled loop would serialise one round trip per pass)
            const long long base = (long long)u0 * K, lim = (long long)a.Ms * K;
            int v[14];
#pragma unroll
            for (int it = 0; it < 14; it++) {
                const int e = lane + it * 64;
                v[it] = -1;
                if (e < 32 * K && base + e < lim) v[it] = a.tbl[base + e];
            }
#pragma unroll
            for (int it = 0; it < 14; it++) {
                const int e = lane + it * 64;
                if (e < 32 * K) tblW[e] = v[it];
            }
        }
        // stationary rows, transposed (batches of 4 units per lane in flight); only the columns this pass's tiles
        // use (a wide stationary operand with a narrow gathered one is split into column passes by the host)
        for (int ub = 0; ub < 32 * sc8n; ub += 256) {
            uint4 sv[4];
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int unit = ub + q * 64 + lane;
                sv[q] = make_uint4(0u, 0u, 0u, 0u);
                if (unit < 32 * sc8n) {
                    const int row = unit / sc8n, c8 = sc8lo + unit - row * sc8n;
                    if (u0 + row < a.Ms) sv[q] = wg2_load8(a.Sm, a.sbf16, (long long)(u0 + row) * a.lds + c8 * 8);
                }
            }
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int unit = ub + q * 64 + lane;
                if (unit < 32 * sc8n) {
                    const int row = unit / sc8n, c8 = sc8lo + unit - row * sc8n;
                    wg2_put_r((unsigned char *)St, a.rss, a.dss, c8, row, sv[q]);
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        // offsets in groups of PF: the gathers of a group are issued together (memory-level parallelism -- every
        // offset is one dependent LDS -> L2/HBM -> LDS -> MFMA chain, and the MFMA work per offset is tiny)
#ifndef WG2_PF1
#define WG2_PF1 4
#endif
#ifndef WG2_PF2
#define WG2_PF2 2
#endif
        constexpr int PF = NU == 1 ? WG2_PF1 : NU == 2 ? WG2_PF2 : 1;
        uint4 pre[PF][NU];
        bool pre_any[PF];
#pragma unroll
        for (int j0 = 0; j0 < OPW; j0 += PF) {
#pragma unroll
            for (int pf = 0; pf < PF; pf++) {
                const int k = k0 + j0 + pf;
                bool any = false;
#pragma unroll
                for (int q = 0; q < NU; q++) {
                    const int unit = lane + q * 64;
                    pre[pf][q] = make_uint4(0u, 0u, 0u, 0u);
                    if (j0 + pf < OPW && k < K && unit < 32 * a.Cg8) {
                        const int row = (int)(((unsigned int)unit * a.invg) >> 16), c8 = unit - row * a.Cg8;
                        int idx = -1;
                        if (u0 + row < a.Ms) idx = a.tbl ? tblW[row * K + k] : (u0 + row);
                        if (idx >= 0) { pre[pf][q] = wg2_load8(a.G, a.gbf16, (long long)idx * a.ldg + c8 * 8); any = true; }
                    }
                }
                pre_any[pf] = __any(any) != 0;
            }
#pragma unroll
            for (int pf = 0; pf < PF; pf++) {
                const int j = j0 + pf;
                if (j < OPW && k0 + j < K && pre_any[pf]) {   // uniform
#pragma unroll
                    for (int q = 0; q < NU; q++) {
                        const int unit = lane + q * 64;
                        if (unit < 32 * a.Cg8) {
                            const int row = (int)(((unsigned int)unit * a.invg) >> 16), c8 = unit - row * a.Cg8;
                            wg2_put_r((unsigned char *)Gt, a.rsg, a.dg, c8, row, pre[pf][q]);
                        }
                    }
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
                    for (int i = 0; i < TPO; i++) {
                        const int tile = tile0 + i;
                        if (tile < ntl) {   // uniform
                            const int mi = tile / a.nt, ni = tile - mi * a.nt;
                            const bf16x8_t av = wg2_frag_tr((const unsigned char *)Gt, lbg, a.rsg, mi);
                            const bf16x8_t bv = wg2_frag_tr((const unsigned char *)St, lbs, a.rss, ni);
                            acc[j < OPW ? j : 0][i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av, bv, acc[j < OPW ? j : 0][i], 0, 0, 0);
                        }
                    }
                    __builtin_amdgcn_wave_barrier();
                }
            }
        }
        __builtin_amdgcn_wave_barrier();   // St / tblW are rewritten by the next chunk
    }
    // sum the four waves through LDS (8 tiles per round) and store
    __syncthreads();
    float *red = (float *)smem;   // 4 waves x 8 tiles x 256 floats = 32 KB
    const long long wsz = (long long)K * a.Cin * a.Cout;
    float *dst = a.dst + (long long)blockIdx.x * wsz;
#pragma unroll
    for (int rd = 0; rd < WG2_T / 8; rd++) {
#pragma unroll
        for (int q8 = 0; q8 < 8; q8++) {
            const int f = rd * 8 + q8, j = f / TPO, i = f % TPO;
#pragma unroll
            for (int q = 0; q < 4; q++) red[((wave * 8 + q8) * 4 + q) * 64 + lane] = acc[j][i][q];
        }
        __syncthreads();
        // wave w finishes tiles 2w, 2w+1 of the round
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const int q8 = wave * 2 + h, f = rd * 8 + q8, j = f / TPO, i = f % TPO;
            const int k = k0 + j, tile = tile0 + i;
            if (k < K && tile < ntl) {
                const int mi = tile / a.nt, ni = tile - mi * a.nt;
                const int wk = a.flipk ? (K - 1 - k) : k;
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    float v = 0.f;
#pragma unroll
                    for (int w = 0; w < 4; w++) v += red[((w * 8 + q8) * 4 + q) * 64 + lane];
                    const int cg = mi * 16 + g * 4 + q, cs = ni * 16 + r;
                    const int ci = a.gx ? cg : cs, co = a.gx ? cs : cg;
                    if (ci < a.Cin && co < a.Cout) dst[((long long)wk * a.Cin + ci) * a.Cout + co] = v;
                }
            }
        }
        __syncthreads();
    }
}

// Wide-stationary weight gradient (the stem: x 136 channels stationary, dy 16 channels gathered, K = 27).  The generic kernel
// above gives a workgroup 16 accumulator tiles, i.e. 4 offsets x 4 of the 9 column tiles: 21 (offset group, column pass)
// combinations, each of which re-reads its slice of x and RE-GATHERS dy -- 1.96 GB of fabric traffic per launch against 288 MB
// algorithmic (profiles/r02_g: 1.14 ms, alone on the GPU at the end of the backward, on the critical path).  Here ONE
// 16-wave workgroup holds all K x nt = 243 tiles: x's 32-row chunk is staged (transposed) once and shared by all waves; wave
// w owns offsets {w, w + 16} with all nt column tiles (18 accumulator tiles = 72 VGPRs), so every dy row is gathered exactly
// once per offset; the next chunk's kernel-map rows and x units are requested before the current chunk's MFMAs.  Each tile
// has a single owner: no cross-wave reduction; row splits write partial dW summed by the fixed-order reduction.
#define WGW_WAVES 16
#define WGW_MAXNT 9
template <int NTV>
__global__ __launch_bounds__(WGW_WAVES * 64) void spconv_wgrad2_wide_kernel(const Wg2Args a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, r = lane & 15, g = lane >> 4;
    const int K = a.K;
    const size_t st_bytes = (size_t)a.imgs;
    const size_t gslot = (size_t)a.imgg;          // one gathered 32 x 16 image
    unsigned short *St = (unsigned short *)smem;                                   // stationary chunk, shared by the waves
    int *tblS = (int *)(smem + st_bytes);                                          // 32 x K
    unsigned short *Gt = (unsigned short *)((unsigned char *)(tblS + 32 * C2_MAXK) + (size_t)wave * 2 * gslot);   // 2 slots per wave
    const int lbg = wg2_lane_base(a.rsg, a.dg, r, g), lbs = wg2_lane_base(a.rss, a.dss, r, g);
    const int nchunks = (a.Ms + 31) >> 5;
    const int c_begin = blockIdx.x * a.cpw, c_end = min(nchunks, c_begin + a.cpw);
    const int k0 = wave, k1 = wave + WGW_WAVES;                                    // this wave's offsets
    f32x4 acc[2][NTV];
#pragma unroll
    for (int j = 0; j < 2; j++)
#pragma unroll
        for (int i = 0; i < NTV; i++) acc[j][i] = (f32x4){0.f, 0.f, 0.f, 0.f};
    // prefetch registers: one kernel-map entry and one 8-channel unit of the stationary operand per thread
    const int sunits = 32 * a.Cs8;                      // <= 1024 (host check)
    int tv = -1;
    uint4 sv = make_uint4(0u, 0u, 0u, 0u);
    auto prefetch = [&](int c) {
        const int u0 = c * 32;
        tv = -1;
        if (a.tbl && t < 32 * K) { const long long e = (long long)u0 * K + t; if (e < (long long)a.Ms * K) tv = a.tbl[e]; }
        sv = make_uint4(0u, 0u, 0u, 0u);
        if (t < sunits) {
            const int row = t / a.Cs8, c8 = t - row * a.Cs8;
            if (u0 + row < a.Ms) sv = wg2_load8(a.Sm, a.sbf16, (long long)(u0 + row) * a.lds + c8 * 8);
        }
    };
    if (c_begin < c_end) prefetch(c_begin);
    for (int c = c_begin; c < c_end; c++) {
        const int u0 = c * 32;
        if (t < 32 * K) tblS[t] = a.tbl ? tv : (u0 + t < a.Ms ? u0 + t : -1);
        if (t < sunits) {
            const int row = t / a.Cs8, c8 = t - row * a.Cs8;
            wg2_put_r((unsigned char *)St, a.rss, a.dss, c8, row, sv);
        }
        __syncthreads();
        if (c + 1 < c_end) prefetch(c + 1);
        // gathers of this wave's two offsets (32 rows x 16 channels = 64 units: one per lane and offset)
        uint4 gv[2];
        bool any[2];
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const int k = j == 0 ? k0 : k1;
            gv[j] = make_uint4(0u, 0u, 0u, 0u);
            bool got = false;
            if (k < K) {
                const int row = lane >> 1, c8 = lane & 1;
                const int idx = (u0 + row < a.Ms) ? tblS[row * K + k] : -1;
                if (idx >= 0) { gv[j] = wg2_load8(a.G, a.gbf16, (long long)idx * a.ldg + c8 * 8); got = true; }
            }
            any[j] = __any(got) != 0;
        }
#pragma unroll
        for (int j = 0; j < 2; j++)
            if (any[j]) wg2_put_r((unsigned char *)Gt + j * gslot, a.rsg, a.dg, lane & 1, lane >> 1, gv[j]);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
        for (int j = 0; j < 2; j++) {
            if (!any[j]) continue;      // wave-uniform
            const bf16x8_t av = wg2_frag_tr((const unsigned char *)Gt + j * gslot, lbg, a.rsg, 0);
#pragma unroll
            for (int i = 0; i < NTV; i++) {
                const bf16x8_t bv = wg2_frag_tr((const unsigned char *)St, lbs, a.rss, i);
                acc[j][i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av, bv, acc[j][i], 0, 0, 0);
            }
        }
        __syncthreads();   // St / tblS are rewritten by the next chunk
    }
    // every tile has one owner: store (gathered operand = dy: P = dW[k]^T, rows = Cout channel, columns = Cin channel)
    const long long wsz = (long long)K * a.Cin * a.Cout;
    float *dst = a.dst + (long long)blockIdx.x * wsz;
#pragma unroll
    for (int j = 0; j < 2; j++) {
        const int k = j == 0 ? k0 : k1;
        if (k >= K) continue;
        const int wk = a.flipk ? (K - 1 - k) : k;
#pragma unroll
        for (int i = 0; i < NTV; i++)
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int cg = g * 4 + q, cs = i * 16 + r;
                const int ci = a.gx ? cg : cs, co = a.gx ? cs : cg;
                if (ci < a.Cin && co < a.Cout) dst[((long long)wk * a.Cin + ci) * a.Cout + co] = acc[j][i][q];
            }
    }
}

// dW[e] = sum_r part[r][e]: 32 elements x 8 split groups per workgroup; group sums are combined in group order
__global__ __launch_bounds__(256) void wgrad2_reduce_kernel(const float *__restrict__ part, float *__restrict__ dW, long long n, int R, int accum) {
    __shared__ float sh[8][32];
    const int el = threadIdx.x & 31, rg = threadIdx.x >> 5;
    const long long e = (long long)blockIdx.x * 32 + el;
    float v = 0.f;
    if (e < n)
        for (int r = rg; r < R; r += 8) v += part[(long long)r * n + e];
    sh[rg][el] = v;
    __syncthreads();
    if (rg == 0 && e < n) {
        float s = accum ? dW[e] : 0.f;
#pragma unroll
        for (int q = 0; q < 8; q++) s += sh[q][el];
        dW[e] = s;
    }
}

// ------------------------------------------------------------------------------ weight gradient, third generation
// What bounds spconv_wgrad2_kernel at the big levels is instruction issue, not memory: ~110 VALU/SALU instructions per
// (32-row chunk, offset) and lane for one MFMA -- run-time operand types (both conversion paths compiled in), bounds checks
// and exec-mask juggling around every gather, 64-bit address arithmetic -- and every offset group re-reads the stationary
// chunk and the kernel-map rows (profiles/r02_i: 75 MB of HBM traffic per launch against 32 MB algorithmic).  This kernel
// generalises the wide-stationary kernel above to every shape of levels 0-2:
//   * one workgroup of NW waves shares an iteration's rows (S sub-chunks of 32): kernel-map rows and the stationary operand are
//     staged ONCE (row-major, converted to bf16 on the way), double-buffered in LDS, the next iteration's requested from
//     memory before this iteration's gathers (one barrier per iteration);
//   * wave w owns the offsets kbase + w + j*NW (j < OW) with all MT x NT tiles: no cross-wave reduction, every gathered row
//     is fetched once per offset;
//   * gathers are raw buffer loads (an absent neighbour, index -1, is an out-of-range offset: the hardware returns zeros;
//     rows past the end likewise), all OW*S*MT of a wave's iteration in flight together; compile-time shapes, 32-bit offsets:
//     ~10 instructions per gathered unit;
//   * transposing LDS reads (ds_read_b64_tr_b16) deliver both MFMA operands from the row-major images.
// Row splits write partial dW (single owner per tile and split: deterministic) summed by the fixed-order reduction.
struct Wg3Args {
    const void *G; const void *Sm; const int *tbl; float *dst;
    unsigned int gbytes, sbytes, tbytes;   // buffer extents in bytes
    int growb, srowb;                      // row pitch in bytes
    int Ms, Cs8, cpw, flipk, Cin, Cout, K;
    unsigned int invs;                     // ceil(65536 / Cs8)
    int rss, dss, imgs;                    // stationary image (wg2_img)
    const void *tbl16; unsigned int t16bytes;   // optional 16-bit delta form of tbl (KV = 27; see spconv_fwd2_kernel)
};

__device__ __forceinline__ uint4 wg3_cvt8(const u32x4_t lo, const u32x4_t hi) {
    return make_uint4(pack2bf2(__uint_as_float(lo.x), __uint_as_float(lo.y)), pack2bf2(__uint_as_float(lo.z), __uint_as_float(lo.w)),
                      pack2bf2(__uint_as_float(hi.x), __uint_as_float(hi.y)), pack2bf2(__uint_as_float(hi.z), __uint_as_float(hi.w)));
}

// GX: the gathered operand is x (bf16), the stationary one dy; else dy is gathered and x (bf16) stationary.  DYBF: dy is stored
// as bf16 (the executor's single-consumer gradient buffers), else fp32 and converted on the way into LDS.
// NW * OW * KG >= KV; with equality (27 = 9 waves x 3 offsets, 8 = 4 x 2 = 8 x 1) no wave carries an idle offset slot.
typedef v4s16_t __attribute__((address_space(3))) *wg3_lds_p;
template <int MT, int NT, int KV, int NW, int OW, int KG, int S, bool GX, bool DYBF, bool T16>
__global__ __launch_bounds__(NW * 64) void spconv_wgrad3_kernel(const Wg3Args a) {
    static_assert(!T16 || KV == 27, "the 16-bit table exists for the 27-offset maps only");
    constexpr int NTH = NW * 64;
    constexpr int TE = S * 32 * KV;                                    // kernel-map entries per iteration
    constexpr int TL = (TE + NTH - 1) / NTH;                           //   ... per thread
    constexpr int SU = (S * 32 * NT * 2 + NTH - 1) / NTH;              // stationary 8-channel units per thread and iteration
    constexpr int RSBG = (MT * 32) % 128 == 0 ? MT * 32 + 32 : MT * 32, DG = RSBG % 64 == 0 ? 32 : 128;
    constexpr int IMGG = (32 * RSBG + 3 * DG + 15) & ~15;
    constexpr int GE = (GX || DYBF) ? 1 : 2, SE = (GX && !DYBF) ? 2 : 1;   // 16-byte loads per gathered / stationary 8-channel unit
    constexpr int CG8 = 2 * MT;
    constexpr bool FULL = NW * OW * KG == KV;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int t = threadIdx.x, lane = t & 63, r = lane & 15, g = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    // LDS (byte offsets): 2 x stationary images | 2 x kernel-map rows | one gather image per wave
    const int st_bytes = S * a.imgs;
    const int tb_base = 2 * st_bytes;
    const int gs_off = tb_base + 2 * TE * 4 + wave * IMGG;
    const int lbg = gs_off + wg2_lane_base(RSBG, DG, r, g), lbs = wg2_lane_base(a.rss, a.dss, r, g);
    const __amdgpu_buffer_rsrc_t rg = __builtin_amdgcn_make_buffer_rsrc((void *)a.G, 0, a.gbytes, D3_RSRC_FLAGS);
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void *)a.Sm, 0, a.sbytes, D3_RSRC_FLAGS);
    constexpr bool t16 = T16;                             // (a compile-time form: a run-time choice put both table loops into the iteration
                                                          //  and a full vmcnt(0) between the table loads and the gathers)
    const __amdgpu_buffer_rsrc_t rt = t16 ? __builtin_amdgcn_make_buffer_rsrc((void *)a.tbl16, 0, a.t16bytes, D3_RSRC_FLAGS)
                                          : __builtin_amdgcn_make_buffer_rsrc((void *)a.tbl, 0, a.tbytes, D3_RSRC_FLAGS);
    const int nit = (a.Ms + 32 * S - 1) / (32 * S);
    const int it_begin = blockIdx.x * a.cpw, it_end = min(nit, it_begin + a.cpw);
    const int k0 = blockIdx.y * (NW * OW) + wave;                      // this wave's offsets: k0 + j * NW

    f32x4 acc[OW][MT][NT];
#pragma unroll
    for (int j = 0; j < OW; j++)
#pragma unroll
        for (int mi = 0; mi < MT; mi++)
#pragma unroll
            for (int ni = 0; ni < NT; ni++) acc[j][mi][ni] = (f32x4){0.f, 0.f, 0.f, 0.f};

    // the stationary units this thread stages (the same image slots every iteration)
    int s_img[SU];
    unsigned int s_off[SU];
#pragma unroll
    for (int i = 0; i < SU; i++) {
        const int u = t + i * NTH;
        s_img[i] = -1; s_off[i] = 0xFFFFFFE0u;                          // out of range: the loads return zeros
        if (u < S * 32 * a.Cs8) {
            const int srow = (int)(((unsigned int)u * a.invs) >> 16), c8 = u - srow * a.Cs8, r32 = srow & 31;
            s_img[i] = (srow >> 5) * a.imgs + r32 * a.rss + (r32 >> 3) * a.dss + c8 * 16;
            s_off[i] = (unsigned int)(srow * a.srowb + c8 * (SE == 2 ? 32 : 16));
        }
    }
    // gather lanes: row / unit of this lane's q-th gathered unit; byte offset of its kernel-map entry (offset k0, sub-chunk 0)
    int g_row[MT], g_c8[MT];
#pragma unroll
    for (int q = 0; q < MT; q++) { const int unit = lane + q * 64; g_row[q] = unit / CG8; g_c8[q] = unit - g_row[q] * CG8; }

    int tv[TL];
    int erow[TL];                     // row (inside the iteration's 32 * S rows) of this thread's i-th kernel-map entry
#pragma unroll
    for (int i = 0; i < TL; i++) erow[i] = (t + i * NTH) / KV;
    u32x4_t sv[SU][SE];
    auto prefetch = [&](int it) {
        const unsigned int row0 = (unsigned int)it * (32 * S);
        if constexpr (t16) {
#pragma unroll
            for (int i = 0; i < TL; i++) {
                const int e = t + i * NTH;
                tv[i] = 0;
                if (TL * NTH == TE || e < TE) tv[i] = (int)(short)__builtin_amdgcn_raw_buffer_load_b16(rt, (row0 * KV + e) * 2u, 0, 0);   // (beyond the table: 0; decoded where it is stored)
            }
        } else {
#pragma unroll
        for (int i = 0; i < TL; i++) {
            const int e = t + i * NTH;
            tv[i] = 0;
            if (TL * NTH == TE || e < TE) tv[i] = __builtin_amdgcn_raw_buffer_load_b32(rt, (row0 * KV + e) * 4u, 0, 0);
        }
        }
#pragma unroll
        for (int i = 0; i < SU; i++) {
            const unsigned int off = s_img[i] >= 0 ? row0 * (unsigned int)a.srowb + s_off[i] : 0xFFFFFFE0u;
#pragma unroll
            for (int h = 0; h < SE; h++) sv[i][h] = __builtin_amdgcn_raw_buffer_load_b128(rs, off + 16u * h, 0, 0);
        }
    };
    if (it_begin < it_end) prefetch(it_begin);
    for (int it = it_begin; it < it_end; it++) {
        const int buf = (it - it_begin) & 1;
        const int st_off = buf * st_bytes, tb_off = tb_base + buf * (TE * 4);
#pragma unroll
        for (int i = 0; i < TL; i++) {
            const int e = t + i * NTH;
            // (the 16-bit delta is decoded HERE, an iteration after its load was issued: decoding in prefetch() made every wave wait for the
            // table's round trip before it could issue its gathers)
            if (TL * NTH == TE || e < TE) *(int *)(smem + tb_off + e * 4) = !t16 ? tv[i] : (tv[i] == -32768 ? -1 : it * (32 * S) + erow[i] + tv[i]);
        }
#pragma unroll
        for (int i = 0; i < SU; i++)
            if (s_img[i] >= 0) {
                uint4 v;
                if constexpr (SE == 2) v = wg3_cvt8(sv[i][0], sv[i][SE - 1]);
                else v = make_uint4(sv[i][0].x, sv[i][0].y, sv[i][0].z, sv[i][0].w);
                *(uint4 *)(smem + st_off + s_img[i]) = v;
            }
        __syncthreads();
        if (it + 1 < it_end) prefetch(it + 1);
        // this wave's gathers: OW offsets x S sub-chunks x MT units per lane, all in flight together
        u32x4_t gv[OW][S][MT][GE];
#pragma unroll
        for (int j = 0; j < OW; j++) {
            const int k = k0 + j * NW;
            if (FULL || k < KV) {   // wave-uniform (scalar)
#pragma unroll
                for (int s = 0; s < S; s++)
#pragma unroll
                    for (int q = 0; q < MT; q++) {
                        const int idx = *(const int *)(smem + tb_off + ((s * 32 + g_row[q]) * KV + k) * 4);
                        const unsigned int off = (unsigned int)idx * (unsigned int)a.growb + g_c8[q] * (GE == 2 ? 32 : 16);
#pragma unroll
                        for (int h = 0; h < GE; h++) gv[j][s][q][h] = __builtin_amdgcn_raw_buffer_load_b128(rg, off + 16u * h, 0, 0);
                    }
            }
        }
#pragma unroll
        for (int s = 0; s < S; s++) {
            bf16x8_t af[OW][MT];
#pragma unroll
            for (int j = 0; j < OW; j++) {
                const int k = k0 + j * NW;
                if (FULL || k < KV) {
#pragma unroll
                    for (int q = 0; q < MT; q++) {
                        uint4 v;
                        if constexpr (GE == 1) v = make_uint4(gv[j][s][q][0].x, gv[j][s][q][0].y, gv[j][s][q][0].z, gv[j][s][q][0].w);
                        else v = wg3_cvt8(gv[j][s][q][0], gv[j][s][q][GE - 1]);
                        *(uint4 *)(smem + gs_off + g_row[q] * RSBG + (g_row[q] >> 3) * DG + g_c8[q] * 16) = v;
                    }
#pragma unroll
                    for (int mi = 0; mi < MT; mi++) {
                        const v4s16_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((wg3_lds_p)(smem + lbg + mi * 32));
                        const v4s16_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((wg3_lds_p)(smem + lbg + mi * 32 + 4 * RSBG));
                        af[j][mi] = __builtin_bit_cast(bf16x8_t, (v8s16_t)__builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
                    }
                }
            }
#pragma unroll
            for (int ni = 0; ni < NT; ni++) {
                const int bo = st_off + s * a.imgs + lbs + ni * 32;
                const v4s16_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((wg3_lds_p)(smem + bo));
                const v4s16_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((wg3_lds_p)(smem + bo + 4 * a.rss));
                const bf16x8_t bv = __builtin_bit_cast(bf16x8_t, (v8s16_t)__builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
#pragma unroll
                for (int j = 0; j < OW; j++) {
                    const int k = k0 + j * NW;
                    if (FULL || k < KV) {
#pragma unroll
                        for (int mi = 0; mi < MT; mi++)
                            acc[j][mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[j][mi], bv, acc[j][mi][ni], 0, 0, 0);
                    }
                }
            }
        }
    }
    const long long wsz = (long long)KV * a.Cin * a.Cout;
    float *dst = a.dst + (long long)blockIdx.x * wsz;
#pragma unroll
    for (int j = 0; j < OW; j++) {
        const int k = k0 + j * NW;
        if (!FULL && k >= KV) continue;
        const int wk = a.flipk ? (KV - 1 - k) : k;
#pragma unroll
        for (int mi = 0; mi < MT; mi++)
#pragma unroll
            for (int ni = 0; ni < NT; ni++)
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const int cg = mi * 16 + g * 4 + q, cs = ni * 16 + r;
                    const int ci = GX ? cg : cs, co = GX ? cs : cg;
                    if (ci < a.Cin && co < a.Cout) dst[((long long)wk * a.Cin + ci) * a.Cout + co] = acc[j][mi][ni][q];
                }
    }
}

// shapes the third-generation kernel is instantiated for: (MT, NT, K, gx) -> (NW, OW, S)
struct Wg3Cfg { int mt, nt, k, gx, nw, ow, kg, s; };
#define WG3_CONFIGS(X)                                                        \
    X(1, 1, 27, 1, 9, 3, 1, 8)   /* 16 -> 16, level 0 */                       \
    X(1, 2, 27, 0, 9, 3, 1, 4)   /* 32 -> 16 (first conv behind a concatenation) */ \
    X(1, 2, 8, 1, 4, 2, 1, 4)    /* down 16 -> 32 */                           \
    X(1, 2, 8, 0, 4, 2, 1, 4)    /* up 32 -> 16 */                             \
    X(2, 2, 27, 1, 9, 3, 1, 4)   /* 32 -> 32, level 1 */                       \
    X(2, 2, 27, 1, 9, 1, 3, 4)   /*   ... three offset groups (more workgroups per partial dW) */ \
    X(2, 4, 27, 0, 9, 3, 1, 1)   /* 64 -> 32 */                                \
    X(2, 4, 27, 0, 9, 1, 3, 4)                                                 \
    X(2, 3, 8, 1, 8, 1, 1, 4)    /* down 32 -> 48 */                           \
    X(2, 3, 8, 0, 8, 1, 1, 4)    /* up 48 -> 32 */                             \
    X(3, 3, 27, 1, 9, 3, 1, 1)   /* 48 -> 48, level 2 */                       \
    X(3, 3, 27, 1, 9, 1, 3, 2)                                                 \
    X(3, 6, 27, 0, 9, 1, 3, 2)   /* 96 -> 48 */
/* (S: sub-chunks of 32 rows per iteration, i.e. gathers in flight per wave -- swept per shape in round 3.)  Measured and left to
 * the other kernels (tools/wgrad_bench.py, profiles/r02_k): the stem 136 -> 16 (the 16-wave wide-stationary kernel: 208 us against
 * 273 us here at 649 k rows) and the stride-2 pairs of level 2 and deeper (within noise).  Round 6: two 7-wave workgroups per compute unit for
 * 16 -> 16 (4 offsets per wave, S = 3: 128 VGPRs) ran 68 us against 45 us for the one 9-wave workgroup (gpurun_out/r06_j30): not kept */
#define WG3_ROW(MT, NT, KV, GXV, NW, OW, KG, SV) {MT, NT, KV, GXV, NW, OW, KG, SV},
static const Wg3Cfg wg3_cfgs[] = {WG3_CONFIGS(WG3_ROW)};
#undef WG3_ROW
static bool wg3_enabled() { return d3_tune(D3T_WG3) != 0; }   // D3_WG3=0: A/B measurements
// Row splits of a configuration.  One workgroup per compute unit: measured on MI355X (tools/wgrad_bench.py, 649 k rows, 16 -> 16)
// 256 / 384 / 512 / 1024 workgroups = 57 / 75 / 68 / 90 us -- a multiple of the CU count keeps the CUs evenly loaded, every extra
// split is another partial dW written and read back.  The partials stay below max(16 MB, 25 % of the algorithmic bytes).
static int wg3_splits(const Wg3Cfg &c, int Ms, int Mg, int K, int Cg, int Cs, int Cin, int Cout, bool gbf, bool sbf, int *cpw, bool *capped) {
    const int nit = (Ms + 32 * c.s - 1) / (32 * c.s);
    const long long wsz = (long long)K * Cin * Cout * 4;
    const double alg = (double)Ms * K * 4 + (double)Mg * Cg * (gbf ? 2 : 4) + (double)Ms * Cs * (sbf ? 2 : 4);
    double cap = 0.25 * alg; if (cap < 16.0 * 1048576) cap = 16.0 * 1048576;
    int target = d3_conv_ncu();
    int R = target / c.kg; if (R < 1) R = 1;
    const int capR = (int)(cap / (double)wsz);
    *capped = R > capR;
    if (R > capR) R = capR;
    if (R > (nit + 1) / 2) R = (nit + 1) / 2;
    if (R < 2) R = 2;            // (always row-split: the partials go through the reduction; Ms >= 2048 gives nit >= 8)
    *cpw = (nit + R - 1) / R;
    return (nit + *cpw - 1) / *cpw;
}
static const Wg3Cfg *wg3_pick(int Ms, int Mg, int K, int Cg, int Cs, int Cin, int Cout, bool gx, bool gbf, bool sbf) {
    if (!wg3_enabled() || Ms < 2048 || (Cg & 15) || (Cs & 7)) return nullptr;
    if (gx ? !gbf : !sbf) return nullptr;                            // x bf16 only (dy fp32 or bf16)
    // 32-bit buffer offsets: operand extents with up to 2x row pitch (views of concatenated buffers)
    if ((long long)Mg * Cg * 2 * (gbf ? 2 : 4) >= (1ll << 31) || (long long)Ms * Cs * 2 * (sbf ? 2 : 4) >= (1ll << 31) || (long long)Ms * K * 4 >= (1ll << 31)) return nullptr;
    const int mt = Cg / 16, nt = (Cs + 15) / 16;
    const Wg3Cfg *best = nullptr;
    int best_wgs = 0;
    for (const Wg3Cfg &c : wg3_cfgs)
        if (c.mt == mt && c.nt == nt && c.k == K && c.gx == (gx ? 1 : 0)) {
            int cpw; bool capped;
            const int wgs = wg3_splits(c, Ms, Mg, K, Cg, Cs, Cin, Cout, gbf, sbf, &cpw, &capped) * c.kg;
            if (!capped) return &c;              // the first (fewest offset groups) whose splits fill the chip within the budget
            if (wgs > best_wgs) { best = &c; best_wgs = wgs; }
        }
    return best;
}


// ------------------------------------------------------------------------------ weight gradient, reference precision
// D3_CONV_F32: dW[k] = sum_u G[tbl[u,k]]^T (x) Sm[u] with exact fp32 products on v_mfma_f32_16x16x4_f32.  No LDS staging:
// the MFMA operands are read straight from memory -- A[i = lane & 15][kk = lane >> 4] = (x side)[row kk][ci0 + i],
// B[kk][j = lane & 15] = (dy side)[row kk][co0 + j], four rows per step, 64 contiguous bytes per row and tile.
// A workgroup owns (a row range, a group of OW offsets, a BG x BS block of tiles): the stationary operand's rows are read
// ONCE per step and serve all OW offsets (one workgroup per offset re-read them 27 times: 2.3 GB per level-0 launch); its
// 4 waves take interleaved 4-row groups, keep OW x BG x BS accumulator tiles (<= 18), and are summed through LDS in
// wave order; row ranges write partial dW that wgrad2_reduce_kernel adds in range order: deterministic, no atomics.
struct WgfArgs {
    const float *G, *Sm;        // gathered operand (rows tbl[u][k]) and stationary operand (row u)
    const int *tbl;             // (Ms, K) or NULL (identity, K == 1)
    float *dst;                 // partials [R][K][CinW][Cout]
    int ldg, lds, Ms, K, gx;    // gx: the gathered operand is x (else dy: D3_CONV_XSTAT)
    int Cg, Cs;                 // channels of the gathered / stationary operand
    int CinW, Cout, flipk, rows_per;   // rows per range (multiple of 16)
    int ngb, nsb;               // tile blocks of the gathered / stationary side
};
template <int BG, int BS, int OW>
__global__ __launch_bounds__(256) void spconv_wgrad_f32_kernel(const WgfArgs a) {
    __shared__ float redS[4][4][64];     // wave, q, lane: one tile at a time
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i16 = lane & 15, kk = lane >> 4;
    const int r = blockIdx.x;
    const int k0 = blockIdx.y * OW;
    const int gb = (int)blockIdx.z / a.nsb, sb = (int)blockIdx.z - gb * a.nsb;
    const int u0 = r * a.rows_per, u1 = min(a.Ms, u0 + a.rows_per);
    f32x4 acc[OW][BG][BS];
#pragma unroll
    for (int o = 0; o < OW; o++)
#pragma unroll
        for (int p = 0; p < BG; p++)
#pragma unroll
            for (int q = 0; q < BS; q++) acc[o][p][q] = (f32x4){0.f, 0.f, 0.f, 0.f};
    int cg[BG], cs[BS];
#pragma unroll
    for (int p = 0; p < BG; p++) cg[p] = (gb * BG + p) * 16 + i16;
#pragma unroll
    for (int q = 0; q < BS; q++) cs[q] = (sb * BS + q) * 16 + i16;
    for (int u = u0 + wave * 4; u < u1; u += 16) {
        const int row = u + kk;
        const bool live = row < u1;
        const long long sr = live ? row : 0;
        float sv[BS];
#pragma unroll
        for (int q = 0; q < BS; q++) { sv[q] = a.Sm[sr * a.lds + (cs[q] < a.Cs ? cs[q] : 0)]; if (!live || cs[q] >= a.Cs) sv[q] = 0.f; }
        // every load of the step is issued before the first MFMA (a use right behind a load serialises the round trips):
        // the OW kernel-map entries, then the OW x BG gathered values -- absent neighbours / offsets read row 0 and are zeroed
        int g[OW];
#pragma unroll
        for (int o = 0; o < OW; o++) g[o] = (live && k0 + o < a.K) ? (a.tbl ? a.tbl[(long long)row * a.K + k0 + o] : row) : -1;
        float gv[OW][BG];
#pragma unroll
        for (int o = 0; o < OW; o++) {
            const long long gr = g[o] >= 0 ? g[o] : 0;
#pragma unroll
            for (int p = 0; p < BG; p++) gv[o][p] = a.G[gr * a.ldg + (cg[p] < a.Cg ? cg[p] : 0)];
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int o = 0; o < OW; o++) {
#pragma unroll
            for (int p = 0; p < BG; p++) {
                const float v = (g[o] < 0 || cg[p] >= a.Cg) ? 0.f : gv[o][p];
#pragma unroll
                for (int q = 0; q < BS; q++)     // D[x-side channel][dy-side channel]: the x operand goes first
                    acc[o][p][q] = a.gx ? __builtin_amdgcn_mfma_f32_16x16x4f32(v, sv[q], acc[o][p][q], 0, 0, 0)
                                        : __builtin_amdgcn_mfma_f32_16x16x4f32(sv[q], v, acc[o][p][q], 0, 0, 0);
            }
        }
    }
    // D layout: row (= ci) (lane >> 4) * 4 + e, column (= co) lane & 15
#pragma unroll
    for (int o = 0; o < OW; o++) {
        if (k0 + o >= a.K) break;      // (uniform)
        const int kd = a.flipk ? a.K - 1 - (k0 + o) : k0 + o;
        float *out = a.dst + ((size_t)r * a.K + kd) * a.CinW * a.Cout;
#pragma unroll
        for (int p = 0; p < BG; p++)
#pragma unroll
            for (int q = 0; q < BS; q++) {
                __syncthreads();
#pragma unroll
                for (int e = 0; e < 4; e++) redS[wave][e][lane] = acc[o][p][q][e];
                __syncthreads();
                const int t = threadIdx.x, ln = t & 63, e = t >> 6;
                const float v = redS[0][e][ln] + redS[1][e][ln] + redS[2][e][ln] + redS[3][e][ln];
                const int tg = (gb * BG + p) * 16, ts = (sb * BS + q) * 16;
                const int ci = (a.gx ? tg : ts) + (ln >> 4) * 4 + e, co = (a.gx ? ts : tg) + (ln & 15);
                if (ci < a.CinW && co < a.Cout) out[(size_t)ci * a.Cout + co] = v;
            }
    }
}
struct WgfCfg { int bg, bs, ow; };
// block of tiles per workgroup and offsets per group: OW * BG * BS <= 18 accumulator tiles
static WgfCfg wgf_cfg(int Cg, int Cs, int K) {
    const int tg = (Cg + 15) / 16, ts = (Cs + 15) / 16;
    WgfCfg c;
    c.bg = tg >= 3 ? 3 : tg; c.bs = ts >= 3 ? 3 : ts;
    // (register budget: accumulators + the step's gathered values must leave room for >= 2 waves per SIMD -- the kernel is a
    // chain of memory round trips, one wave per SIMD left it at 400 us for a level-0 16 -> 16 layer)
    static const int ow_of[4][4] = {{0, 0, 0, 0}, {0, 14, 9, 5}, {0, 9, 4, 3}, {0, 5, 3, 2}};
    c.ow = ow_of[c.bg][c.bs];
    if (K <= 8 && c.ow > 8) c.ow = 8;
    if (K == 1) c.ow = 1;
    return c;
}
static int launch_wgf(const WgfArgs &a, const WgfCfg &c, int R, hipStream_t s) {
    const dim3 grid(R, (a.K + c.ow - 1) / c.ow, a.ngb * a.nsb);
#define WGF_CASE(BGV, BSV, OWV) if (c.bg == BGV && c.bs == BSV && c.ow == OWV) { spconv_wgrad_f32_kernel<BGV, BSV, OWV><<<grid, 256, 0, s>>>(a); D3_LAUNCH_CHECK(); return 0; }
    WGF_CASE(1, 1, 14) WGF_CASE(1, 1, 8) WGF_CASE(1, 2, 9) WGF_CASE(1, 2, 8) WGF_CASE(2, 1, 9) WGF_CASE(2, 1, 8) WGF_CASE(1, 3, 5)
    WGF_CASE(3, 1, 5) WGF_CASE(2, 2, 4) WGF_CASE(2, 3, 3) WGF_CASE(3, 2, 3) WGF_CASE(3, 3, 2)
    WGF_CASE(1, 1, 1) WGF_CASE(1, 2, 1) WGF_CASE(2, 1, 1) WGF_CASE(1, 3, 1) WGF_CASE(3, 1, 1) WGF_CASE(2, 2, 1) WGF_CASE(2, 3, 1) WGF_CASE(3, 2, 1) WGF_CASE(3, 3, 1)
#undef WGF_CASE
    return D3_ERR_ARG;
}

struct Wg2Plan { int tpo, nu, opw, kg, passes, R, cpw, wide; int rsg, dg, imgg, rss, dss, imgs; size_t lds, ws_bytes; const Wg3Cfg *w3; };

static Wg2Plan wg2_plan(int Ms, int Mg, int K, int Cg, int Cs, int Cin, int Cout, bool gx, bool gbf, bool sbf) {
    Wg2Plan p;
    const int mt = (Cg + 15) / 16, nt = (Cs + 15) / 16, ntl = mt * nt;
    p.wide = 0;
    wg2_img(Cg / 8, &p.rsg, &p.dg, &p.imgg);
    wg2_img(Cs / 8, &p.rss, &p.dss, &p.imgs);
    p.imgg = (p.imgg + 15) & ~15; p.imgs = (p.imgs + 15) & ~15;
    p.w3 = wg3_pick(Ms, Mg, K, Cg, Cs, Cin, Cout, gx, gbf, sbf);
    if (p.w3) {
        const Wg3Cfg &c = *p.w3;
        p.kg = c.kg;
        bool capped;
        p.R = wg3_splits(c, Ms, Mg, K, Cg, Cs, Cin, Cout, gbf, sbf, &p.cpw, &capped);
        const long long wsz = (long long)K * Cin * Cout * 4;
        p.lds = (size_t)2 * c.s * p.imgs + (size_t)2 * c.s * 32 * K * 4 + (size_t)c.nw * (((32 * ((c.mt * 32) % 128 == 0 ? c.mt * 32 + 32 : c.mt * 32) + 3 * 128) + 15) & ~15);
        p.ws_bytes = (size_t)p.R * wsz;
        p.tpo = 0; p.nu = 0; p.opw = c.ow; p.passes = 1;
        return p;
    }
    if (mt == 1 && nt > 4 && nt <= WGW_MAXNT && K <= 2 * WGW_WAVES && 32 * (Cs / 8) <= WGW_WAVES * 64 && Ms >= 4096) {
        // one 16-wave workgroup per row split holds all K x nt tiles (spconv_wgrad2_wide_kernel)
        p.wide = 1; p.tpo = nt; p.nu = 1; p.opw = 2; p.kg = 1; p.passes = 1;
        const int nchunks = (Ms + 31) / 32;
        int R = 256; if (R > (nchunks + 3) / 4) R = (nchunks + 3) / 4; if (R < 1) R = 1;
        p.cpw = (nchunks + R - 1) / R;
        p.R = (nchunks + p.cpw - 1) / p.cpw;
        p.lds = (size_t)p.imgs + (size_t)32 * C2_MAXK * 4 + (size_t)WGW_WAVES * 2 * p.imgg;
        p.ws_bytes = (size_t)p.R * K * Cin * Cout * 4;
        return p;
    }
    p.tpo = ntl <= 1 ? 1 : ntl <= 2 ? 2 : ntl <= 4 ? 4 : ntl <= 8 ? 8 : 16;
    if (mt == 1 && nt > 4) p.tpo = 4;   // column passes of 4 tiles, 4 offsets per wave (the stem: 16 x 136 channels)
    p.nu = (Cg / 8 * 32 + 63) / 64;    // 16-byte units per lane per offset
    p.opw = WG2_T / p.tpo;
    p.kg = (K + p.opw - 1) / p.opw;
    p.passes = (ntl + p.tpo - 1) / p.tpo;
    const int nchunks = (Ms + 31) / 32;
    // row splits: ~2048 waves in flight, at least 2 chunks per wave, partial buffer <= 8 MB
    const long long wsz = (long long)K * Cin * Cout * 4;
    int R = WG2_TARGET_WGS / (p.kg * p.passes); if (R < 1) R = 1;
    const int maxR_rows = (nchunks + 7) / 8; if (R > maxR_rows) R = maxR_rows;
    const long long maxR_mem = ((long long)WG2_PART_MB << 20) / wsz; if (R > maxR_mem) R = (int)maxR_mem;
    if (R < 1) R = 1;
    p.cpw = (nchunks + R - 1) / R;
    p.cpw = (p.cpw + 3) / 4 * 4;
    p.R = (nchunks + p.cpw - 1) / p.cpw;
    const size_t wave_bytes = (size_t)p.imgg + p.imgs + (size_t)32 * C2_MAXK * 4;
    p.lds = 4 * wave_bytes; if (p.lds < 32 * 1024) p.lds = 32 * 1024;
    p.ws_bytes = p.R > 1 ? (size_t)p.R * wsz : 0;
    return p;
}

static Wg2Plan wg2_plan_flags(int Min, int Mout, int K, int Cin, int Cout, int flags) {
    const bool xstat = (flags & D3_CONV_XSTAT) != 0, xbf = (flags & D3_CONV_XBF16) != 0, dybf = (flags & D3_CONV_DYBF16) != 0;
    if (flags & D3_CONV_F32) {       // spconv_wgrad_f32_kernel: (row ranges) x (offset groups) x (tile blocks), always through the partials
        Wg2Plan p;
        memset(&p, 0, sizeof(p));
        const int Ms = xstat ? Min : Mout;
        const WgfCfg cf = wgf_cfg(xstat ? Cout : Cin, xstat ? Cin : Cout, K);
        const int per_range = ((K + cf.ow - 1) / cf.ow) * ((((xstat ? Cout : Cin) + 15) / 16 + cf.bg - 1) / cf.bg) * ((((xstat ? Cin : Cout) + 15) / 16 + cf.bs - 1) / cf.bs);
        int R = (1536 + per_range - 1) / per_range;
        const int maxR = (Ms + 255) / 256; if (R > maxR) R = maxR;
        const long long wsz = (long long)K * Cin * Cout * 4;
        const long long maxR_mem = (64ll << 20) / wsz; if (R > maxR_mem) R = (int)maxR_mem;
        if (R < 1) R = 1;
        p.cpw = ((Ms + R - 1) / R + 15) / 16 * 16;          // rows per range
        if (p.cpw < 16) p.cpw = 16;
        p.R = (Ms + p.cpw - 1) / p.cpw; if (p.R < 1) p.R = 1;
        p.ws_bytes = (size_t)p.R * wsz;
        return p;
    }
    return xstat ? wg2_plan(Min, Mout, K, Cout, Cin, Cin, Cout, false, dybf, xbf) : wg2_plan(Mout, Min, K, Cin, Cout, Cin, Cout, true, xbf, dybf);
}

// flags: the D3_CONV_XSTAT / D3_CONV_XBF16 / D3_CONV_DYBF16 bits of the d3_spconv_wgrad2 call (the kernel choice depends on them)
extern "C" size_t d3_spconv_wgrad2_ws_bytes(int Min, int Mout, int K, int Cin, int Cout, int flags) {
    return wg2_plan_flags(Min, Mout, K, Cin, Cout, flags).ws_bytes;
}

// number of row splits d3_spconv_wgrad2 uses for this shape (its partials: splits x K*CinW*Cout floats in ws)
extern "C" int d3_spconv_wgrad2_splits(int Min, int Mout, int K, int Cin, int Cout, int flags) {
    return wg2_plan_flags(Min, Mout, K, Cin, Cout, flags).R;
}

template <int MT, int NT, int KV, int NW, int OW, int KG, int S, bool GX>
static int launch_wg3(const Wg3Args &a, const Wg2Plan &p, bool dybf, hipStream_t s) {
    static_assert(NW * OW * KG >= KV, "offsets not covered");
    return d3_with_bools([&](auto dy16, auto t16) {
        if constexpr (KV != 27 && t16.value) return (int)D3_ERR_ARG;      // the 16-bit kernel map is K = 27's: no other instances
        else {
            constexpr auto kernel = spconv_wgrad3_kernel<MT, NT, KV, NW, OW, KG, S, GX, dy16.value, t16.value>;
            if (const int rc = d3_allow_lds<kernel>(128 * 1024)) return rc;
            kernel<<<dim3(p.R, KG), NW * 64, p.lds, s>>>(a);
            D3_LAUNCH_CHECK();
            return 0;
        }
    }, dybf, KV == 27 && a.tbl16 != nullptr);
}

// the one 16-wave workgroup per row split that holds all K x nt tiles (wg2_plan: p.wide)
static int launch_wgw(const Wg2Args &a, const Wg2Plan &p, hipStream_t s) {
    return d3_with_value<5, 6, 7, 8, 9>(a.nt, [&](auto nt) {
        if (const int rc = d3_allow_lds<spconv_wgrad2_wide_kernel<nt.value>>(128 * 1024)) return rc;
        spconv_wgrad2_wide_kernel<nt.value><<<p.R, WGW_WAVES * 64, p.lds, s>>>(a);
        D3_LAUNCH_CHECK();
        return 0;
    });
}

// tiles per offset group: 1, 2, 4, 8, anything else runs 16; 16-byte units per lane per offset: the first of 1, 2, 4, 7, 14 that holds p.nu
static int launch_wg2(const Wg2Args &a, const Wg2Plan &p, hipStream_t s) {
    const int tpo = (p.tpo == 1 || p.tpo == 2 || p.tpo == 4 || p.tpo == 8) ? p.tpo : 16;
    const int nu = p.nu <= 1 ? 1 : p.nu <= 2 ? 2 : p.nu <= 4 ? 4 : p.nu <= 7 ? 7 : 14;
    return d3_with_value<1, 2, 4, 8, 16>(tpo, [&](auto t) {
        constexpr int TPO = decltype(t)::value;
        return d3_with_value<1, 2, 4, 7, 14>(nu, [&](auto u) {
            if (const int rc = d3_allow_lds<spconv_wgrad2_kernel<TPO, u.value>>(128 * 1024)) return rc;
            spconv_wgrad2_kernel<TPO, u.value><<<dim3(p.R, p.kg, p.passes), 256, p.lds, s>>>(a);
            D3_LAUNCH_CHECK();
            return 0;
        });
    });
}

// x (Min, ldx) and dy (Mout, ldy), each fp32 or bf16 (D3_CONV_XBF16 / D3_CONV_DYBF16); tbl as for d3_spconv_wgrad
// (the forward map, or with D3_CONV_XSTAT the transposed map); dW (K,CinW,Cout) fp32 (CinW <= Cin: x may carry
// zero-padded channels), written (or accumulated into
// with D3_CONV_ACCUM).  ws >= d3_spconv_wgrad2_ws_bytes().  Cin % 8 == 0 and Cout % 8 == 0, else D3_ERR_ARG.
// tbl16 (internal entry, conv.h): the validated 16-bit delta form of tbl, or NULL
// Each family builds its arguments and launches its kernel into rc; everything behind d3_prof_begin leaves through the closing block
// (a record left open hands d3_prof_collect / d3_prof_dump an event that was never recorded, or one recorded by an earlier region).
int d3_conv2_wgrad(const void *x, int ldx, const int *tbl, const void *tbl16, const void *dy, int ldy, float *dW, int Min, int Mout,
                   int K, int Cin, int Cout, int CinW, int flags, void *ws, size_t ws_bytes, void *stream) {
    D3_CLEAR();
    if (K < 1 || K > C2_MAXK || Cin < 8 || Cout < 8 || (Cin & 7) || (Cout & 7) || Cin > 224 || Cout > 224) return D3_ERR_ARG;
    if (tbl == nullptr && K != 1) return D3_ERR_ARG;
    hipStream_t s = d3_stream(stream);
    const int xstat = (flags & D3_CONV_XSTAT) ? 1 : 0, accum = (flags & D3_CONV_ACCUM) ? 1 : 0;
    const int xbf = (flags & D3_CONV_XBF16) ? 1 : 0, dybf = (flags & D3_CONV_DYBF16) ? 1 : 0;
    if ((xbf ? (ldx & 7) : (ldx & 3)) || (dybf ? (ldy & 7) : (ldy & 3))) return D3_ERR_ARG;
    if (CinW < 1 || CinW > Cin) return D3_ERR_ARG;
    const long long wn = (long long)K * CinW * Cout;   // dW is (K, CinW, Cout): x may carry zero-padded channels
    const int Ms = xstat ? Min : Mout;
    if (Ms <= 0) { if (!accum) D3_CHECK(hipMemsetAsync(dW, 0, wn * 4, s)); return 0; }
    const bool f32 = (flags & D3_CONV_F32) != 0;
    if (f32 && (xbf || dybf)) return D3_ERR_ARG;
    const int Cg = xstat ? Cout : Cin, Cs = xstat ? Cin : Cout;
    const int flipk = (flags & D3_CONV_FLIPK) ? 1 : 0;
    const Wg2Plan p = wg2_plan_flags(Min, Mout, K, Cin, Cout, flags);
    if (f32 ? (size_t)p.R * wn * 4 > ws_bytes : p.ws_bytes > ws_bytes) return D3_ERR_WORKSPACE;
    const bool direct = !f32 && (p.R == 1 && !accum) && !p.wide && !p.w3;   // the kernel writes dW itself: no partials
    const bool noreduce = (flags & D3_CONV_NOREDUCE) != 0;   // the caller sums the partials (batched over its layers)
    if (!f32 && !direct && p.R == 1 && ws_bytes < (size_t)wn * 4) return D3_ERR_WORKSPACE;
    const double bytes = (xbf ? 2.0 : 4.0) * (double)Min * Cin + (dybf ? 2.0 : 4.0) * (double)Mout * Cout + 4.0 * (double)wn +
                         (tbl ? 4.0 * (double)Ms * K : 0.0);
    void *pr = d3_prof_begin(1, bytes, 0.0, s);
    { const int dims[6] = {Min, Mout, K, Cin, Cout, f32 ? 32 : p.w3 ? 3 : (p.wide ? 1 : 2)}; for (int i = 0; i < 6; i++) d3_prof_tag(pr, i, dims[i]); }
    int rc = D3_ERR_ARG;
    if (f32) {
        WgfArgs f;
        if (xstat) { f.Sm = (const float *)x; f.lds = ldx; f.G = (const float *)dy; f.ldg = ldy; f.gx = 0; }
        else { f.Sm = (const float *)dy; f.lds = ldy; f.G = (const float *)x; f.ldg = ldx; f.gx = 1; }
        f.Cs = Cs; f.Cg = Cg;
        f.tbl = tbl; f.dst = (float *)ws; f.Ms = Ms; f.K = K; f.CinW = CinW; f.Cout = Cout;
        f.flipk = flipk; f.rows_per = p.cpw;
        const WgfCfg cf = wgf_cfg(f.Cg, f.Cs, K);
        f.ngb = ((f.Cg + 15) / 16 + cf.bg - 1) / cf.bg; f.nsb = ((f.Cs + 15) / 16 + cf.bs - 1) / cf.bs;
        rc = launch_wgf(f, cf, p.R, s);
    } else {
        Wg2Args a;
        if (xstat) { a.Sm = x; a.lds = ldx; a.sbf16 = xbf; a.G = dy; a.ldg = ldy; a.gbf16 = dybf; a.gx = 0; }
        else { a.Sm = dy; a.lds = ldy; a.sbf16 = dybf; a.G = x; a.ldg = ldx; a.gbf16 = xbf; a.gx = 1; }
        a.tbl = tbl; a.dst = direct ? dW : (float *)ws;
        a.Ms = Ms; a.K = K; a.mt = (Cg + 15) / 16; a.nt = (Cs + 15) / 16; a.Cg8 = Cg / 8; a.Cs8 = Cs / 8;
        a.invg = (65536u + a.Cg8 - 1) / a.Cg8; a.invs = (65536u + a.Cs8 - 1) / a.Cs8;
        a.cpw = p.cpw; a.flipk = flipk; a.Cin = CinW; a.Cout = Cout;
        a.rsg = p.rsg; a.dg = p.dg; a.imgg = p.imgg; a.rss = p.rss; a.dss = p.dss; a.imgs = p.imgs;
        if (p.w3) {
            const int Mg = xstat ? Mout : Min;
            const long long gb = ((long long)(Mg - 1) * a.ldg + Cg) * (a.gbf16 ? 2 : 4), sb = ((long long)(Ms - 1) * a.lds + Cs) * (a.sbf16 ? 2 : 4);
            if (gb < (1ll << 31) && sb < (1ll << 31) && Mg >= 1) {   // 32-bit buffer offsets; else rc stays D3_ERR_ARG
                const Wg3Cfg &c = *p.w3;
                Wg3Args b;
                b.G = a.G; b.Sm = a.Sm; b.tbl = tbl; b.dst = (float *)ws;
                b.gbytes = (unsigned int)gb; b.sbytes = (unsigned int)sb; b.tbytes = (unsigned int)((long long)Ms * K * 4);
                b.tbl16 = (tbl16 && K == 27) ? tbl16 : nullptr; b.t16bytes = (unsigned int)((long long)Ms * K * 2);
                if (b.tbl16) d3_conv_count_t16();
                b.growb = a.ldg * (a.gbf16 ? 2 : 4); b.srowb = a.lds * (a.sbf16 ? 2 : 4);
                b.Ms = Ms; b.Cs8 = Cs / 8; b.cpw = p.cpw; b.flipk = a.flipk; b.Cin = CinW; b.Cout = Cout; b.K = K;
                b.invs = a.invs; b.rss = p.rss; b.dss = p.dss; b.imgs = p.imgs;
#define WG3_CASE(MT, NT, KV, GXV, NW, OW, KG, SV)                                                                \
                if (c.mt == MT && c.nt == NT && c.k == KV && c.gx == GXV && c.kg == KG && c.ow == OW && c.s == SV) rc = launch_wg3<MT, NT, KV, NW, OW, KG, SV, (GXV != 0)>(b, p, dybf != 0, s);
                WG3_CONFIGS(WG3_CASE)
#undef WG3_CASE
            }
        } else if (p.wide) {
            rc = launch_wgw(a, p, s);
        } else {
            rc = launch_wg2(a, p, s);
        }
    }
    // the closing block: the partials' reduction when it is due, the profiling record's end
    if (rc == 0 && !direct && !noreduce) {
        wgrad2_reduce_kernel<<<(int)((wn + 31) / 32), 256, 0, s>>>((const float *)ws, dW, wn, p.R, accum);
        rc = (int)hipGetLastError();
    }
    d3_prof_end(pr, s);
    return rc;
}
extern "C" int d3_spconv_wgrad2(const void *x, int ldx, const int *tbl, const void *dy, int ldy, float *dW, int Min,
                                int Mout, int K, int Cin, int Cout, int CinW, int flags, void *ws, size_t ws_bytes,
                                void *stream) {
    return d3_conv2_wgrad(x, ldx, tbl, nullptr, dy, ldy, dW, Min, Mout, K, Cin, Cout, CinW, flags, ws, ws_bytes, stream);
}
