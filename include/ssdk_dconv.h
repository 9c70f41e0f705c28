/*
 * ssdk_dconv.h -- C-ABI of the dilated 3x3 convolution (csrc/ssdk_dconv.hip), part of libssdk.so.
 *
 * A header of its own next to ssdk.h, like ssdk_convt.h, ssdk_cat.h and ssdk_dkres.h: the entry points of ssdk.h and the layout of
 * ssdk_op are a closed list under SSDK_VERSION 245, and this addition changes neither.  Conventions (pointers, streams, return
 * values, zero-initialised descriptors, ssdk_last_error) are those of ssdk.h.
 *
 * The layer (the last convolution of each branch of ssds/modeling/layers/rfb_layers.py BasicRFB): a 3x3 convolution of dilation d,
 * stride 1, padding d, on NHWC tensors of dtype SSDK_BF16 | SSDK_F16, with a folded BatchNorm (scale, bias) in fp32 and an activation:
 *   y[n][oy][ox][co] = act( scale[co] * sum_{ky,kx,ci} x[n][oy + d(ky-1)][ox + d(kx-1)][ci] * w[co][ky][kx][ci] + bias[co] )
 * Positions outside the image contribute nothing (and are never read).  fp32 accumulation on v_mfma_f32_16x16x32_{bf16,f16}, ONE
 * rounding at the store.  One launch: no workspace, no allocation, no atomics, no synchronisation between workgroups,
 * hipGraph-capturable, bit-reproducible.  The output map has the size of the input map; y must not overlap x.
 *
 * The layer is a convolution, not an op kind of its own: it is described by an ssdk_conv_desc whose res_mode carries the dilation
 * (below), ssdk_conv hands such a descriptor to ssdk_dconv3x3, and inside a recorded plan it is an SSDK_OP_CONV.
 */
#ifndef SSDK_DCONV_H_
#define SSDK_DCONV_H_

#include "ssdk.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ssdk_conv_desc.res_mode, bits 8-11: dilation - 1 (0: an ordinary convolution, what every descriptor written before this header
 * means).  dilation = ((res_mode & SSDK_CONV_DILATION_MASK) >> SSDK_CONV_DILATION_SHIFT) + 1.  (3840 = 0xF00.) */
#define SSDK_CONV_DILATION_SHIFT 8
#define SSDK_CONV_DILATION_MASK 3840

/* The kernel's tiling (tests choose their ragged shapes from it): a workgroup owns SSDK_DCONV_TILE_PIXELS consecutive pixels of the
 * flattened [N * H * W] pixel index (a group may straddle rows and images) times at most SSDK_DCONV_TILE_COUT output channels (a
 * multiple of SSDK_DCONV_FRAG_COUT, chosen per launch), and its SSDK_DCONV_KSPLIT waves share the k-steps of 32. */
#define SSDK_DCONV_TILE_PIXELS 16
#define SSDK_DCONV_FRAG_COUT 16
#define SSDK_DCONV_TILE_COUT 64
#define SSDK_DCONV_KSPLIT 4
/* the predicate's bounds */
#define SSDK_DCONV_MIN_DILATION 2
#define SSDK_DCONV_MAX_DILATION 8
#define SSDK_DCONV_MAX_CHANNELS 1024
#define SSDK_DCONV_MAX_SIDE 32768

/* desc: x NHWC [N][H][W][Cin], y NHWC [N][H][W][Cout], scale (may be NULL = 1) / bias fp32 [Cout], act SSDK_ACT_NONE | SSDK_ACT_RELU,
 * w the KRSC tensor [Cout][3][3][Cin] (required non-NULL as for every ssdk_conv kind; the kernel does not read it), and
 * w_frag (REQUIRED) = the fragment-major image (ssdk.h) of the matrix [Cout][Kpad], k = tap * Cin + ci, tap = 3 ky + kx,
 * Kpad = 32 * ceil(9 Cin / 32), zeros in the columns >= 9 Cin and in the rows >= Cout: ssdk_weight_frag_bytes(Cout, Kpad) bytes.
 * Accepted: res_mode bits 8-11 = dilation - 1 with every other bit zero, k = 3, stride = 1, groups <= 1, NHWC in and out,
 * residual = y2 = NULL, what ssdk_dconv3x3_supported accepts, N >= 1, N * H * W < 2^31, every pointer 16-byte aligned, y not
 * overlapping x.  Anything else is SSDK_E_BADARG with a message, before any launch (and before any other device call). */
int ssdk_dconv3x3(const ssdk_conv_desc* desc, void* stream);
/* 1 when ssdk_dconv3x3 takes the layer, else 0:  Cin % 8 == 0 and Cout % 8 == 0, each 8 ... SSDK_DCONV_MAX_CHANNELS;
 * SSDK_DCONV_MIN_DILATION <= dilation <= SSDK_DCONV_MAX_DILATION;  1 <= H, W <= SSDK_DCONV_MAX_SIDE;  dtype SSDK_BF16 | SSDK_F16.
 * Host only, touches no device: the single source of the rule. */
int ssdk_dconv3x3_supported(int Cin, int Cout, int H, int W, int dilation, int dtype);

#ifdef __cplusplus
}
#endif
#endif /* SSDK_DCONV_H_ */
