// enet.hip -- ENet frame features on the device (reference: model/enet.py create_enet / create_enet_for_3d, run by
// data/scannet/compute_multiview_features.py:27-96), driven by d3net_amd/enet.py.
//
// Inference only.  The host folds every BatchNorm (eval) and the Dropout2d x(1 - p) scale into the convolutions in float64 and
// uploads one fp32 parameter blob (layout: enet_layers below, every segment padded to 4 floats).  One batch of F frames is
//   * d3_enet_preprocess: uint8 (F,H0,W0,3) -> normalized fp32 (F,3,H,W) through per-size source row / column tables that the host
//     derives from Pillow's NEAREST resize and the centre crop (x / 255 and (x - mean) / std, true float32 divisions);
//   * d3_enet_forward: the initial block in one launch, then three convolution launches per bottleneck (66), each an implicit GEMM
//     on NHWC fp32 activations with v_mfma_f32_16x16x4_f32 (exact fp32 fma chains) and a fused epilogue:
//       conv a / conv b: folded bias, PReLU;
//       conv c         : folded bias (BN and x(1 - p)), + side branch (identity, or 2x2 max pool of the block input with zero
//                        channels appended), PReLU -- the last one writes the (F,128,H/8,W/8) NCHW output directly.
//     The asymmetric 1x5 (no bias) -> 5x1 pair is folded on the host into one 5x5 convolution (exact in exact arithmetic).
// A workgroup never spans two frames and every output element is one fixed k-ordered fma chain, so a frame's output is bitwise
// independent of the batch it runs in; no atomics, no split-K.  67 launches per batch, no host synchronisation.
#include "common.h"

#define EN_NLAYERS 67            // initial block + 22 bottlenecks x 3 convolutions
#define EN_TAB 7                 // per layer: cin, cout, kh, kw, stride, pad, dilation
#define EN_MAX_FRAMES 65535      // grid.y
#define EN_BLOCK 256

// conv b of blocks 10..25 (model/enet.py): dilation, 0 = asymmetric 1x5 + 5x1 (folded to 5x5, pad 2)
static const int EN_DIL[16] = {1, 2, 0, 4, 1, 8, 0, 16, 1, 2, 0, 4, 1, 8, 0, 16};

static void enet_table(int *t) {
    int *r = t;
    auto row = [&](int ci, int co, int kh, int kw, int s, int p, int d) {
        r[0] = ci; r[1] = co; r[2] = kh; r[3] = kw; r[4] = s; r[5] = p; r[6] = d; r += EN_TAB;
    };
    row(3, 16, 3, 3, 2, 1, 1);                                   // initial: conv 3->13 3x3/2 + max pool of the 3 inputs
    for (int b = 4; b <= 25; b++) {
        bool down = (b == 4 || b == 9);
        int co = b < 9 ? 64 : 128, inner = b < 9 ? 16 : 32, ci = b == 4 ? 16 : (b == 9 ? 64 : co);
        if (down) row(ci, inner, 2, 2, 2, 0, 1); else row(ci, inner, 1, 1, 1, 0, 1);
        int d = b >= 10 ? EN_DIL[b - 10] : 1;
        if (d == 0) row(inner, inner, 5, 5, 1, 2, 1); else row(inner, inner, 3, 3, 1, d, d);
        row(inner, co, 1, 1, 1, 0, 1);
    }
}

static inline long long en_pad4(long long n) { return (n + 3) / 4 * 4; }

// float offsets of each layer's segments in the blob: initial = W[13][3][3][3], bias 13, pool scale 3, pool shift 3, slope 16;
// convolutions = W[kh*kw][cout][cin], bias[cout], slope[cout]
static long long enet_offsets(const int *t, long long *w, long long *b, long long *s, long long *extra) {
    long long o = 0;
    for (int l = 0; l < EN_NLAYERS; l++) {
        const int *r = t + l * EN_TAB;
        if (l == 0) {
            w[0] = o; o += en_pad4(13 * 27);
            b[0] = o; o += en_pad4(13);
            extra[0] = o; o += en_pad4(3);
            extra[1] = o; o += en_pad4(3);
            s[0] = o; o += en_pad4(16);
        } else {
            w[l] = o; o += en_pad4((long long)r[2] * r[3] * r[1] * r[0]);
            b[l] = o; o += en_pad4(r[1]);
            s[l] = o; o += en_pad4(r[1]);
        }
    }
    return o;
}

int d3_enet_layers(int *table, int cap) {
    if (table) {
        if (cap < EN_NLAYERS * EN_TAB) return D3_ERR_ARG;
        enet_table(table);
    }
    return EN_NLAYERS;
}

long long d3_enet_param_count(void) {
    int t[EN_NLAYERS * EN_TAB];
    long long w[EN_NLAYERS], b[EN_NLAYERS], s[EN_NLAYERS], e[2];
    enet_table(t);
    return enet_offsets(t, w, b, s, e);
}

// ---- preprocessing (compute_multiview_features.py:53-73) ---------------------------------------------------------------------------
__global__ void __launch_bounds__(EN_BLOCK) enet_pre_kernel(const unsigned char *__restrict__ src, int H0, int W0,
                                                            const int *__restrict__ rows, const int *__restrict__ cols, int H, int W,
                                                            float *__restrict__ out) {
    int f = blockIdx.y;
    int i = blockIdx.x * EN_BLOCK + threadIdx.x;
    if (i >= H * W) return;
    int y = i / W, x = i - y * W;
    int sy = min(max(rows[y], 0), H0 - 1), sx = min(max(cols[x], 0), W0 - 1);   // the host validated both tables
    const unsigned char *p = src + (size_t)f * H0 * W0 * 3 + ((size_t)sy * W0 + sx) * 3;
    const float mean[3] = {0.496342f, 0.466664f, 0.440796f}, stdv[3] = {0.277856f, 0.28623f, 0.291129f};
    float *o = out + (size_t)f * 3 * H * W + i;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        float v = __fdiv_rn((float)p[c], 255.0f);
        o[(size_t)c * H * W] = __fdiv_rn(v - mean[c], stdv[c]);
    }
}

int d3_enet_preprocess(const unsigned char *frames, int F, int H0, int W0, const int *rows, const int *cols, int H, int W, float *out,
                       void *stream) {
    if (F < 0 || H0 <= 0 || W0 <= 0 || H <= 0 || W <= 0 || (F > 0 && (!frames || !rows || !cols || !out))) return D3_ERR_ARG;
    if (F > EN_MAX_FRAMES || (long long)H0 * W0 * 3 >= (1ll << 31) || (long long)H * W * 3 >= (1ll << 31)) return D3_ERR_RANGE;
    if (F == 0) return 0;
    D3_CLEAR();
    dim3 grid((H * W + EN_BLOCK - 1) / EN_BLOCK, F);
    enet_pre_kernel<<<grid, EN_BLOCK, 0, d3_stream(stream)>>>(frames, H0, W0, rows, cols, H, W, out);
    D3_LAUNCH_CHECK();
    return 0;
}

// ---- initial block (elements 0-3): conv 3->13 3x3/2 pad 1 || max pool 2x2/2 of the input, BN, PReLU -> NHWC 16 channels ----------
__global__ void __launch_bounds__(EN_BLOCK) enet_initial_kernel(const float *__restrict__ x, int H, int W, const float *__restrict__ w,
                                                                const float *__restrict__ bias, const float *__restrict__ pscale,
                                                                const float *__restrict__ pshift, const float *__restrict__ slope,
                                                                float *__restrict__ y) {
    int f = blockIdx.y;
    int Ho = H / 2, Wo = W / 2;
    int i = blockIdx.x * EN_BLOCK + threadIdx.x;
    if (i >= Ho * Wo) return;
    int oy = i / Wo, ox = i - oy * Wo;
    const float *xf = x + (size_t)f * 3 * H * W;
    float in[3][3][3];
#pragma unroll
    for (int c = 0; c < 3; c++)
#pragma unroll
        for (int ky = 0; ky < 3; ky++)
#pragma unroll
            for (int kx = 0; kx < 3; kx++) {
                int iy = 2 * oy - 1 + ky, ix = 2 * ox - 1 + kx;
                in[c][ky][kx] = (iy >= 0 && iy < H && ix >= 0 && ix < W) ? xf[((size_t)c * H + iy) * W + ix] : 0.0f;
            }
    float v[16];
#pragma unroll
    for (int co = 0; co < 13; co++) {
        float a = 0.0f;
#pragma unroll
        for (int c = 0; c < 3; c++)
#pragma unroll
            for (int ky = 0; ky < 3; ky++)
#pragma unroll
                for (int kx = 0; kx < 3; kx++) a = fmaf(w[((co * 3 + c) * 3 + ky) * 3 + kx], in[c][ky][kx], a);
        v[co] = a + bias[co];
    }
#pragma unroll
    for (int c = 0; c < 3; c++) {   // the pool window is input rows 2oy, 2oy+1 = in[c][1..2][1..2]
        float m = in[c][1][1];
        m = in[c][1][2] > m ? in[c][1][2] : m;
        m = in[c][2][1] > m ? in[c][2][1] : m;
        m = in[c][2][2] > m ? in[c][2][2] : m;
        v[13 + c] = fmaf(m, pscale[c], pshift[c]);
    }
    float4 *o = (float4 *)(y + ((size_t)f * Ho * Wo + i) * 16);
#pragma unroll
    for (int q = 0; q < 4; q++) {
        float r[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            float t = v[4 * q + k];
            r[k] = t > 0.0f ? t : slope[4 * q + k] * t;
        }
        o[q] = make_float4(r[0], r[1], r[2], r[3]);
    }
}

// ---- convolution as an implicit GEMM: rows = output pixels of one frame, columns = output channels, k = (tap, input channel) --------
// A wave owns MT x 16 output pixels and all NT x 16 output channels.  Per tap and 16-channel chunk, lane l (r = l & 15, g = l >> 4)
// loads channels c0 + 4g .. c0 + 4g + 3 of pixel r (one float4) for every pixel tile and of weight row r for every channel tile; MFMA
// kk sums channels c0 + kk, c0 + 4 + kk, c0 + 8 + kk, c0 + 12 + kk (the k slots g = 0..3), so the order of the chain is fixed.
enum { EN_EPI_PRELU = 0, EN_EPI_RESID = 1 };

struct EnConv {
    const float *x, *w, *bias, *slope, *side;
    float *y;
    int Cin, Hin, Win, Hout, Wout, KH, KW, stride, pad, dil;
    int side_pool, Cside;   // RESID: side = block input (identity, same size / Cout channels) or (2Hout, 2Wout, Cside) max-pooled
    int nchw;               // RESID: write (F, Cout, Hout, Wout) instead of NHWC
};

typedef float en_f4 __attribute__((ext_vector_type(4)));

template <int MT, int NT, int EPI>
__global__ void __launch_bounds__(EN_BLOCK) enet_conv_kernel(EnConv a) {
    constexpr int Cout = NT * 16;
    const int f = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 15, g = lane >> 4;
    const int HWo = a.Hout * a.Wout;
    const int p0 = (blockIdx.x * (EN_BLOCK / 64) + wave) * (MT * 16);
    if (p0 >= HWo) return;
    const int Cin = a.Cin;
    const float *xf = a.x + (size_t)f * a.Hin * a.Win * Cin;

    int oy[MT], ox[MT];
    bool ok[MT];
#pragma unroll
    for (int t = 0; t < MT; t++) {
        int p = p0 + t * 16 + r;
        ok[t] = p < HWo;
        p = ok[t] ? p : 0;
        oy[t] = p / a.Wout;
        ox[t] = p - oy[t] * a.Wout;
    }
    en_f4 acc[MT][NT];
#pragma unroll
    for (int t = 0; t < MT; t++)
#pragma unroll
        for (int j = 0; j < NT; j++) acc[t][j] = (en_f4){0.0f, 0.0f, 0.0f, 0.0f};

    for (int ky = 0; ky < a.KH; ky++)
        for (int kx = 0; kx < a.KW; kx++) {
            const float *ap[MT];
#pragma unroll
            for (int t = 0; t < MT; t++) {
                int iy = oy[t] * a.stride - a.pad + ky * a.dil, ix = ox[t] * a.stride - a.pad + kx * a.dil;
                bool v = ok[t] && iy >= 0 && iy < a.Hin && ix >= 0 && ix < a.Win;
                ap[t] = v ? xf + (iy * a.Win + ix) * Cin + 4 * g : nullptr;
            }
            const float *wp = a.w + (size_t)(ky * a.KW + kx) * Cout * Cin + r * Cin + 4 * g;
            for (int c0 = 0; c0 < Cin; c0 += 16) {
                float4 A[MT], B[NT];
#pragma unroll
                for (int t = 0; t < MT; t++) A[t] = ap[t] ? *(const float4 *)(ap[t] + c0) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll
                for (int j = 0; j < NT; j++) B[j] = *(const float4 *)(wp + j * 16 * Cin + c0);
#pragma unroll
                for (int t = 0; t < MT; t++)
#pragma unroll
                    for (int j = 0; j < NT; j++) {
                        acc[t][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(A[t].x, B[j].x, acc[t][j], 0, 0, 0);
                        acc[t][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(A[t].y, B[j].y, acc[t][j], 0, 0, 0);
                        acc[t][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(A[t].z, B[j].z, acc[t][j], 0, 0, 0);
                        acc[t][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(A[t].w, B[j].w, acc[t][j], 0, 0, 0);
                    }
            }
        }

    // epilogue: lane holds rows 4g + i of each pixel tile, column r of each channel tile
    const size_t fo = (size_t)f * HWo * Cout;
#pragma unroll
    for (int j = 0; j < NT; j++) {
        const int n = j * 16 + r;
        const float bn = a.bias[n], sl = a.slope[n];
#pragma unroll
        for (int t = 0; t < MT; t++)
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const int p = p0 + t * 16 + 4 * g + i;
                if (p >= HWo) continue;
                float v = acc[t][j][i] + bn;
                if (EPI == EN_EPI_RESID) {
                    float s;
                    if (!a.side_pool) {
                        s = a.side[fo + (size_t)p * Cout + n];
                    } else if (n < a.Cside) {
                        int py = p / a.Wout, px = p - py * a.Wout;
                        int Ws = 2 * a.Wout;
                        const float *sp = a.side + (size_t)f * (2 * a.Hout) * Ws * a.Cside + ((2 * py) * Ws + 2 * px) * a.Cside + n;
                        float m = sp[0];
                        float q = sp[a.Cside];
                        m = q > m ? q : m;
                        q = sp[Ws * a.Cside];
                        m = q > m ? q : m;
                        q = sp[(Ws + 1) * a.Cside];
                        m = q > m ? q : m;
                        s = m;
                    } else {
                        s = 0.0f;
                    }
                    v = v + s;
                }
                v = v > 0.0f ? v : sl * v;
                if (EPI == EN_EPI_RESID && a.nchw)
                    a.y[((size_t)f * Cout + n) * HWo + p] = v;
                else
                    a.y[fo + (size_t)p * Cout + n] = v;
            }
    }
}

template <int MT, int NT, int EPI>
static int en_launch(const EnConv &c, int F, hipStream_t s) {
    int rows = (EN_BLOCK / 64) * MT * 16;
    dim3 grid((c.Hout * c.Wout + rows - 1) / rows, F);
    enet_conv_kernel<MT, NT, EPI><<<grid, EN_BLOCK, 0, s>>>(c);
    D3_LAUNCH_CHECK();
    return 0;
}

static int en_conv(const EnConv &c, int Cout, int epi, int F, hipStream_t s) {
    if (epi == EN_EPI_PRELU) {
        if (Cout == 16) return en_launch<4, 1, EN_EPI_PRELU>(c, F, s);
        if (Cout == 32) return en_launch<4, 2, EN_EPI_PRELU>(c, F, s);
    } else {
        if (Cout == 64) return en_launch<2, 4, EN_EPI_RESID>(c, F, s);
        if (Cout == 128) return en_launch<2, 8, EN_EPI_RESID>(c, F, s);
    }
    return D3_ERR_ARG;
}

// two block-I/O buffers of H*W*4 floats per frame (16 ch at H/2, 64 at H/4, 128 at H/8 all fit) + two inner buffers of H*W
// (H and W are multiples of 8, so every region is a multiple of 256 bytes and the four lie back to back)
struct EnWs { float *bufA, *bufB, *in1, *in2; };
static void en_layout(D3Carver &c, int F, int H, int W, EnWs &w) {
    const size_t per = (size_t)H * W;
    w.bufA = c.take<float>(F * per * 4); w.bufB = c.take<float>(F * per * 4);
    w.in1 = c.take<float>(F * per); w.in2 = c.take<float>(F * per);
}

size_t d3_enet_ws_bytes(int F, int H, int W) {
    if (F <= 0 || H <= 0 || W <= 0 || (H % 8) || (W % 8)) return 0;
    D3Carver c(nullptr, 0);
    EnWs w;
    en_layout(c, F, H, W, w);
    return c.off;
}

int d3_enet_forward(const float *x, int F, int H, int W, const float *params, long long n_params, const int *table, int n_table,
                    int upto, float *out, void *ws, size_t ws_bytes, void *stream) {
    int tab[EN_NLAYERS * EN_TAB];
    enet_table(tab);
    if (!table || n_table != EN_NLAYERS * EN_TAB) return D3_ERR_ARG;
    for (int i = 0; i < EN_NLAYERS * EN_TAB; i++)
        if (table[i] != tab[i]) return D3_ERR_ARG;
    long long wo[EN_NLAYERS], bo[EN_NLAYERS], so[EN_NLAYERS], eo[2];
    if (n_params != enet_offsets(tab, wo, bo, so, eo)) return D3_ERR_ARG;
    if (F < 0 || H <= 0 || W <= 0 || (H % 8) || (W % 8) || upto < 3 || upto > 25) return D3_ERR_ARG;
    if (F > EN_MAX_FRAMES || (long long)H * W * 4 >= (1ll << 31)) return D3_ERR_RANGE;
    if (F == 0) return 0;
    if (!x || !params || !out || !ws) return D3_ERR_ARG;
    D3Carver cv(ws, ws_bytes);
    EnWs lw;
    en_layout(cv, F, H, W, lw);
    if (!cv.ok()) return D3_ERR_WORKSPACE;
    hipStream_t s = d3_stream(stream);
    D3_CLEAR();

    float *bufA = lw.bufA, *bufB = lw.bufB, *in1 = lw.in1, *in2 = lw.in2;

    int H2 = H / 2, W2 = W / 2;
    dim3 g0((H2 * W2 + EN_BLOCK - 1) / EN_BLOCK, F);
    enet_initial_kernel<<<g0, EN_BLOCK, 0, s>>>(x, H, W, params + wo[0], params + bo[0], params + eo[0], params + eo[1], params + so[0],
                                                upto == 3 ? out : bufA);
    D3_LAUNCH_CHECK();
    if (upto == 3) return 0;

    float *cur = bufA, *nxt = bufB;
    int h = H2, w = W2;
    for (int b = 4; b <= 25; b++) {
        int l = 1 + 3 * (b - 4);
        const int *ra = tab + l * EN_TAB, *rb = ra + EN_TAB, *rc = rb + EN_TAB;
        bool down = ra[4] == 2;
        int ho = down ? h / 2 : h, wo2 = down ? w / 2 : w;
        EnConv c = {};
        // conv a: 1x1, or 2x2 stride 2 in the downsampling blocks
        c.x = cur; c.w = params + wo[l]; c.bias = params + bo[l]; c.slope = params + so[l]; c.y = in1;
        c.Cin = ra[0]; c.Hin = h; c.Win = w; c.Hout = ho; c.Wout = wo2; c.KH = ra[2]; c.KW = ra[3];
        c.stride = ra[4]; c.pad = ra[5]; c.dil = ra[6];
        int rc_ = en_conv(c, ra[1], EN_EPI_PRELU, F, s);
        if (rc_) return rc_;
        // conv b: 3x3 dilated, or the folded 5x5
        c.x = in1; c.w = params + wo[l + 1]; c.bias = params + bo[l + 1]; c.slope = params + so[l + 1]; c.y = in2;
        c.Cin = rb[0]; c.Hin = ho; c.Win = wo2; c.KH = rb[2]; c.KW = rb[3]; c.stride = 1; c.pad = rb[5]; c.dil = rb[6];
        rc_ = en_conv(c, rb[1], EN_EPI_PRELU, F, s);
        if (rc_) return rc_;
        // conv c: 1x1 + side branch + PReLU; block 25 writes the NCHW output (an earlier `upto` block: NHWC)
        bool last = b == upto;
        c.x = in2; c.w = params + wo[l + 2]; c.bias = params + bo[l + 2]; c.slope = params + so[l + 2]; c.y = last ? out : nxt;
        c.Cin = rc[0]; c.KH = 1; c.KW = 1; c.pad = 0; c.dil = 1;
        c.side = cur; c.side_pool = down ? 1 : 0; c.Cside = ra[0]; c.nchw = b == 25 ? 1 : 0;
        rc_ = en_conv(c, rc[1], EN_EPI_RESID, F, s);
        if (rc_) return rc_;
        if (last) return 0;
        float *t = cur; cur = nxt; nxt = t;
        h = ho; w = wo2;
    }
    return 0;
}
