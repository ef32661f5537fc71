// conv.h -- internal interface (C++ linkage) of the convolution family: what the kernel files (spconv.hip, spconv2.hip, spconv3.hip,
// wgrad.hip) share, and what the dispatchers and the U-Net executor (unet.hip) hand each other beyond the C ABI of include/d3hip.h
// -- it travels as arguments.
#pragma once
#include "common.h"
#include "dispatch.h"

// ------------------------------------------------------------------------------ shared by the kernels
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ unsigned int pack2bf2(float lo, float hi) {   // v_cvt_pk_bf16_f32: round to nearest even
    const bf16x2_t p = {(__bf16)lo, (__bf16)hi};
    return __builtin_bit_cast(unsigned int, p);
}
#define D3_RSRC_FLAGS 0x00020000          // raw buffer, 32-bit data format (gfx90a / gfx94x / gfx950)
#define C2_MAXK 27                        // most offsets a kernel map has (3^3)
// rows of a second-level fp64 BatchNorm partial table: a producing convolution workgroup adds its partial row to row workgroup % 16
// (spconv2.hip tells why), the consuming BatchNorm (unet.hip) reads the 16 rows
#define D3_P2_ROWS 16

// compute units of the device (asked once; 256 when the query fails).  spconv2.hip
int d3_conv_ncu();
// one more launch that read a 16-bit kernel map: what d3_spconv_t16_launches() counts (spconv2.hip)
void d3_conv_count_t16();

// ------------------------------------------------------------------------------ dispatchers <-> executor
// fused BatchNorm backward of a data-gradient call (d3_spconv_fwd2_bnbwd): x is the BatchNorm INPUT, fp32, or bf16 with xbf16
struct ConvBn { const void *x; const float *mean, *var, *gamma, *beta; int ldx, relu, xbf16; float eps; };
// the BatchNorm fields of a kernel's argument struct (Conv2Args, Conv3Args) from bn; all zero for no BatchNorm (bn NULL).  Whether
// the BatchNorm input is bf16 (bn->xbf16) stays with the caller: a field of one struct, a template argument for the other
template <typename Args>
static inline void d3_conv_bn_args(Args &a, const ConvBn *bn) {
    static const ConvBn none{};
    const ConvBn &b = bn ? *bn : none;
    a.bnx = (decltype(a.bnx))b.x; a.bn_mean = b.mean; a.bn_var = b.var; a.bn_gamma = b.gamma; a.bn_beta = b.beta;
    a.ldbx = b.ldx; a.bn_relu = b.relu; a.bn_eps = b.eps;
}

// optional tables of one forward / data-gradient call (all NULL: what a caller of the C ABI gets).  The caller has VALIDATED
// tbl16 / tblq (d3_kmap_k3_pack16's / d3_kmap_k3_packq's flag read on the host).
struct ConvExtras {
    const void *tbl16 = nullptr;   // 16-bit delta form of the K = 27 kernel map
    const void *tblq = nullptr;    // lane table of the K = 27 kernel map (spconv3.hip)
    double *part2 = nullptr;       // second-level BatchNorm partial table [D3_P2_ROWS][2][ceil(Cout / 16) * 16] fp64, zeroed by the
                                   // caller; ignored when the call takes no partials
};

// spconv2.hip: d3_spconv_fwd2 (bn NULL) / d3_spconv_fwd2_bnbwd (res NULL).  *nparts: the BatchNorm partial rows the launch wrote
// -- the kernel depends on the tables at hand -- written on every return path, 0 for Mout <= 0
int d3_conv2_run(const void *x, int ldx, const int *tbl, const void *Wp, float *out, int ldo, const float *res, int ldr, float *part,
                 int Min, int Mout, int K, int Cin, int Cout, int flags, const ConvBn *bn, const ConvExtras &ex, int *nparts, void *stream);
// wgrad.hip: d3_spconv_wgrad2 with the (validated) 16-bit delta form of tbl, or NULL
int d3_conv2_wgrad(const void *x, int ldx, const int *tbl, const void *tbl16, const void *dy, int ldy, float *dW, int Min, int Mout,
                   int K, int Cin, int Cout, int CinW, int flags, void *ws, size_t ws_bytes, void *stream);
// spconv3.hip: one K = 27 launch on the lane table tq; D3_ERR_ARG for shapes without an instance.  *nparts as above
int d3_conv3_run(const void *x, int ldx, const void *tq, const void *Wp, void *out, int ldo, const float *res, int ldr, float *part,
                 double *part2, int Min, int Mout, int Cin, int Cout, int obf16, const ConvBn *bn, int *nparts, hipStream_t s);

// what d3_spconv_last_nparts() returns (spconv3.hip): written by the C ABI wrappers d3_spconv_fwd2* / d3_spconv_fwd3* only
extern thread_local int d3_conv_last_nparts;
