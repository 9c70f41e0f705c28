/*
 * ssdk_convttrain.h -- C-ABI of the transposed 3x3 / stride 2 / pad 1 convolution of the SSDShelf TRAINING step: forward with bias
 * and skip map, input gradient, weight + bias gradient (csrc/ssdk_convttrain.hip), part of libssdk.so.
 *
 * A header of its own next to ssdk.h, like ssdk_convt.h and ssdk_cattrain.h: the entry points of ssdk.h are a closed list under
 * SSDK_VERSION 245, and this addition changes neither.  Conventions (pointers, streams, return values, ssdk_last_error) are those
 * of ssdk.h.
 *
 * The layer is nn.ConvTranspose2d(Cin, Cout, 3, stride=2, padding=1, output_padding=0): x [N][Cin][H][W] -> y [N][Cout][2H-1][2W-1],
 * weight w [Cin][Cout][3][3].  All tensors are contiguous NCHW of dtype SSDK_BF16 | SSDK_F16 (ssdk_convt.h is the NHWC,
 * forward-only form the recorded plan runs); the weight master, the bias and all parameter gradients are fp32.  No allocation, no
 * synchronisation, no atomics, sums in a fixed order (bit-reproducible), hipGraph-capturable.  Cin and Cout are multiples of 16 in
 * 16 .. 4096, any N, H, W >= 1 (H == 1 or W == 1: the odd output rows / columns do not exist) with fewer than 2^31 elements per
 * tensor; tensors need the 2-byte alignment of an element (the odd map sides leave rows and planes at any such address), images
 * and the workspace 16 bytes, fp32 arrays 4.  Anything else is SSDK_E_BADARG with a message before any launch.
 *
 * The layer is the adjoint of the dense 3x3 / stride 2 / pad 1 convolution Cout -> Cin on the (2H-1) x (2W-1) map whose OIHW weight
 * is w as it lies in memory; the two images below are that convolution's "dense 3x3 images" (ssdk.h).
 */
#ifndef SSDK_CONVTTRAIN_H_
#define SSDK_CONVTTRAIN_H_

#include "ssdk.h"

#ifdef __cplusplus
extern "C" {
#endif

/* fp32 w [Cin][Cout][3][3] -> the 16-bit images the forward (w_fwd: [Cout / 16][KS(Cin)][4][16][8], rows = output channels, k = tap *
 * Cin + input channel, taps flipped) and the input gradient (w_dgrad: [Cin / 16][KS(Cout)][4][16][8], rows = input channels) read;
 * KS(C) = ceil(9 C / 32).  One launch; either image may be NULL (not written), not both. */
int ssdk_convt_train_prepare(const float* w32, void* w_fwd, void* w_dgrad, int Cin, int Cout, int dtype, void* stream);

/* y = convT(x, w) + bias[Cout] + skip [N][Cout][2H-1][2W-1]: fp32 accumulation on the matrix cores by output parity class (1 / 2 / 2
 * / 4 taps, no zero-inserted tensor), bias and skip added in fp32, ONE rounding.  bias and skip may each be NULL.  One launch. */
int ssdk_convt_train_forward(const void* x, const void* w_fwd, const float* bias, const void* skip, void* y, int N, int Cin, int Cout,
                             int H, int W, int dtype, void* stream);

/* gx [N][Cin][H][W] = the 3x3 / stride 2 / pad 1 convolution of gy [N][Cout][2H-1][2W-1] with w.  One launch.  (The gradient of the
 * skip map is gy itself: no call.) */
int ssdk_convt_train_dgrad(const void* gy, const void* w_dgrad, void* gx, int N, int Cin, int Cout, int H, int W, int dtype,
                           void* stream);

/* Bytes of caller-owned workspace ssdk_convt_train_wgrad needs (0: the shape is not accepted). */
size_t ssdk_convt_train_wgrad_workspace_bytes(int N, int Cin, int Cout, int H, int W);

/* gw [Cin][Cout][3][3] and gb [Cout] (may be NULL: not computed) in fp32 from x and gy: the bias gradient is summed by the
 * workgroups of the weight-gradient pass from the gy rows they stage anyway; the partial sums of both lie in the workspace and are
 * added in index order. */
int ssdk_convt_train_wgrad(const void* x, const void* gy, float* gw, float* gb, void* workspace, size_t workspace_bytes, int N, int Cin,
                           int Cout, int H, int W, int dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SSDK_CONVTTRAIN_H_ */
