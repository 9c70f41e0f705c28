/*
 * ssdk_convt.h -- C-ABI of the transposed convolution of the Shelf neck (csrc/ssdk_convt.hip), part of libssdk.so.
 *
 * A header of its own next to ssdk.h: the entry points of ssdk.h and the layout of ssdk_op are a closed list under
 * SSDK_VERSION 245, and this addition changes neither.  Conventions (pointers, streams, return values, zero-initialised
 * descriptors, ssdk_last_error) are those of ssdk.h.
 */
#ifndef SSDK_CONVT_H_
#define SSDK_CONVT_H_

#include "ssdk.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Transposed 3x3 convolution, stride 2, padding 1, no output padding, + bias (+ skip): the decoder step of the Shelf neck
 * (ssds/shelf.py ShelfPyramid: ConvTranspose2d(C_{i-1}, C_i, 3, stride=2, padding=1, bias=True)(x) + xx[i]; csrc/ssdk_convt.hip).
 *   y [N][2H-1][2W-1][Cout] = act(convT(x [N][H][W][Cin]) + bias[Cout]) (+ skip [N][2H-1][2W-1][Cout])
 * NHWC, dtype SSDK_BF16 | SSDK_F16 (x, weights, skip, y), bias fp32; fp32 accumulation on v_mfma_f32_16x16x32, ONE rounding,
 * after the skip add.  The output is computed by parity class (py, px) = (oy & 1, ox & 1) -- no zero-inserted tensor and no
 * border masking: with oy = 2 iy - 1 + ky an even row takes ky = 1 from iy = oy / 2, an odd row ky = 2 from iy = (oy - 1) / 2 and
 * ky = 0 from iy + 1 (columns alike), so a class has (1 + py)(1 + px) taps and (H - py) x (W - px) pixels, every tap in range.
 *   w_pack  the four parity images of the weight w[Cin][Cout][3][3] (the ConvTranspose2d layout), class 2 py + px, one behind the
 *           other: image c is the fragment-major image (ssdk_weight_frag_bytes) of a [Cout][Kc] matrix, row = output channel,
 *           k = tap * Cin + ci, Kc = taps * Cin rounded up to 32 with zeros; tap = dy * (1 + px) + dx reads input pixel
 *           (iy + dy, ix + dx) with ky = py ? 2 - 2 dy : 1, kx = px ? 2 - 2 dx : 1.  ssdk_convt_pack_bytes(Cin, Cout) is its size
 *           (0 for arguments ssdk_convt3x3s2 does not take); the Python host builds it in fused_conv.ConvTPack.
 * Accepted: Cin, Cout multiples of 8, any H, W >= 1 (H == 1 or W == 1: the odd classes are empty), N <= 65535, fewer than 2^31
 * input pixels; x, w_pack, y, skip, bias 16-byte aligned; skip and bias may be NULL.  Anything else is SSDK_E_BADARG with a
 * message before any launch.  One launch, no allocation, no synchronisation, no atomics: bit-reproducible, hipGraph-capturable.
 * Not part of ssdk_struct_size(): ssdk_convt_desc_bytes() reports its size.  Inside a recorded plan the same call is executor op
 * SSDK_OP_CONVT, described by the op's ssdk_conv_desc member (include/ssdk.h). */
typedef struct ssdk_convt_desc {
  const void* x;
  const void* w_pack;
  const float* bias;
  const void* skip;
  void* y;
  int32_t N, Cin, H, W, Cout, act, dtype, pad;
} ssdk_convt_desc;
int ssdk_convt3x3s2(const ssdk_convt_desc* desc, void* stream);
size_t ssdk_convt_pack_bytes(int Cin, int Cout);
size_t ssdk_convt_desc_bytes(void);

#ifdef __cplusplus
}
#endif
#endif /* SSDK_CONVT_H_ */
