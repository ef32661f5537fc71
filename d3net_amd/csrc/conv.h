// conv.h -- internal interface (C++ linkage) between the convolution dispatchers (spconv2.hip, spconv3.hip) and the U-Net
// executor (unet.hip): what a call needs beyond the C ABI of include/d3hip.h travels as arguments.
#pragma once
#include "common.h"

// fused BatchNorm backward of a data-gradient call (d3_spconv_fwd2_bnbwd): x is the BatchNorm INPUT, fp32, or bf16 with xbf16
struct ConvBn { const void *x; const float *mean, *var, *gamma, *beta; int ldx, relu, xbf16; float eps; };

// optional tables of one forward / data-gradient call (all NULL: what a caller of the C ABI gets).  The caller has VALIDATED
// tbl16 / tblq (d3_kmap_k3_pack16's / d3_kmap_k3_packq's flag read on the host).
struct ConvExtras {
    const void *tbl16 = nullptr;   // 16-bit delta form of the K = 27 kernel map
    const void *tblq = nullptr;    // lane table of the K = 27 kernel map (spconv3.hip)
    double *part2 = nullptr;       // second-level BatchNorm partial table [C2_P2_ROWS][2][ceil(Cout / 16) * 16] fp64, zeroed by the
                                   // caller; ignored when the call takes no partials
};

// spconv2.hip: d3_spconv_fwd2 (bn NULL) / d3_spconv_fwd2_bnbwd (res NULL).  *nparts: the BatchNorm partial rows the launch wrote
// -- the kernel depends on the tables at hand -- written on every return path, 0 for Mout <= 0
int d3_conv2_run(const void *x, int ldx, const int *tbl, const void *Wp, float *out, int ldo, const float *res, int ldr, float *part,
                 int Min, int Mout, int K, int Cin, int Cout, int flags, const ConvBn *bn, const ConvExtras &ex, int *nparts, void *stream);
// spconv2.hip: d3_spconv_wgrad2 with the (validated) 16-bit delta form of tbl, or NULL
int d3_conv2_wgrad(const void *x, int ldx, const int *tbl, const void *tbl16, const void *dy, int ldy, float *dW, int Min, int Mout,
                   int K, int Cin, int Cout, int CinW, int flags, void *ws, size_t ws_bytes, void *stream);
// spconv3.hip: one K = 27 launch on the lane table tq; D3_ERR_ARG for shapes without an instance.  *nparts as above
int d3_conv3_run(const void *x, int ldx, const void *tq, const void *Wp, void *out, int ldo, const float *res, int ldr, float *part,
                 double *part2, int Min, int Mout, int Cin, int Cout, int obf16, const ConvBn *bn, int *nparts, hipStream_t s);

// what d3_spconv_last_nparts() returns (spconv3.hip): written by the C ABI wrappers d3_spconv_fwd2* / d3_spconv_fwd3* only
extern thread_local int d3_conv_last_nparts;
