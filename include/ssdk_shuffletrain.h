/*
 * ssdk_shuffletrain.h -- C-ABI of the ShuffleNetV2 TRAINING step (csrc/ssdk_shuffletrain.hip), part of libssdk.so: the 1x1
 * convolution on channel SLICES of any width (forward, input gradient, weight gradient) and the interleaving join of a unit's two
 * branches, forward and backward.
 *
 * A header of its own next to ssdk.h, like ssdk_cattrain.h: the entry points of ssdk.h are a closed list under SSDK_VERSION 245, and
 * this addition changes neither.  Conventions (pointers, streams, return values, ssdk_last_error) are those of ssdk.h.
 *
 * All tensors are NCHW of dtype SSDK_BF16 | SSDK_F16, HW = H * W, accumulation is fp32.  A tensor with an "image stride" is a channel
 * slice of a wider tensor: the caller folds the channel offset into the pointer and passes the distance in ELEMENTS between two
 * images (>= channels * HW of the slice; equal to it for a contiguous tensor).  Tensor pointers need the 2-byte alignment of an
 * element only (a slice starts Cb * HW * 2 bytes into its tensor); weight matrices and workspaces need 16 bytes.  No allocation, no
 * synchronisation, no atomics, hipGraph-capturable; sums are in a fixed order: the results are bit-reproducible.  Every argument is
 * checked before any launch: null pointers, K or M < 8, a bad lda, an image stride smaller than the slice, a dtype that is not
 * 16 bit, a tensor of 2^32 elements or more (counted over the image strides) are SSDK_E_BADARG with a message, a small workspace is
 * SSDK_E_WORKSPACE.
 */
#ifndef SSDK_SHUFFLETRAIN_H_
#define SSDK_SHUFFLETRAIN_H_

#include "ssdk.h"

#ifdef __cplusplus
extern "C" {
#endif

/* w32 [Cout][Cin] fp32 (the master weights) -> w16 [Cout][Kp] and wt16 [Cin][Mp] (the transpose) in the compute dtype, with
 * Kp = 8 ceil(Cin / 8), Mp = 8 ceil(Cout / 8); the padding columns hold zeros.  One launch.  Cout, Cin >= 1. */
int ssdk_pws_prepare(const float* w32, void* w16, void* wt16, int Cout, int Cin, int dtype, void* stream);

/* Bytes of workspace ssdk_pws_forward needs when sums != NULL (0 on bad arguments). */
size_t ssdk_pws_stats_workspace_bytes(int B, int K, int M, int HW);

/* y[b] = a x[b] (+ bias): x [B][K][HW] with images x_image_stride apart, y [B][M][HW] with images y_image_stride apart, a [M][lda]
 * row-major in the tensors' dtype (lda % 8 == 0, lda >= K, 16-byte aligned; what the columns K .. lda - 1 hold does not matter),
 * bias [M] fp32 or NULL.  K, M >= 8 are any values.  Channels >= K of x are never read and rows >= M of y never written, pixels
 * >= HW of a plane neither.
 * sums (optional) [M][2] fp32: per output channel (sum y, sum y^2) over all images and pixels, of the fp32 accumulators before the
 * store's rounding, reduced in a fixed order through `workspace` (16-byte aligned, ssdk_pws_stats_workspace_bytes) -- the meaning
 * of ssdk_pw_forward_stats.  With sums == NULL the workspace is not used (it may be NULL).
 * The forward of a slice: x = X + Cb HW, x_image_stride = 2 Cb HW.  The input gradient written INTO a slice: x = dy, a = wt16 of
 * ssdk_pws_prepare (lda = Mp), y = GX + Cb HW, y_image_stride = 2 Cb HW. */
int ssdk_pws_forward(const void* x, size_t x_image_stride, const void* a, int lda, const float* bias, void* y, size_t y_image_stride,
                     float* sums, void* workspace, size_t workspace_bytes, int B, int K, int M, int HW, int dtype, void* stream);

/* Bytes of workspace ssdk_pws_wgrad needs (0 on bad arguments). */
size_t ssdk_pws_wgrad_workspace_bytes(int B, int Cout, int Cin, int HW);

/* dw [Cout][Cin] fp32 = sum_b dy[b] x[b]^T: dy [B][Cout][HW] contiguous, x [B][Cin][HW] with images x_image_stride apart.
 * Cout, Cin >= 1.  fp32 partial sums per pixel range, added in index order. */
int ssdk_pws_wgrad(const void* dy, const void* x, size_t x_image_stride, float* dw, void* workspace, size_t workspace_bytes, int B,
                   int Cout, int Cin, int HW, int dtype, void* stream);

/* The join of a ShuffleNetV2 unit, channel_shuffle(cat((left, right), 1), 2):  y[n][2i] = left[n][i], y[n][2i + 1] = right[n][i].
 * y [N][2 Cb][HW] and right [N][Cb][HW] are contiguous; left [N][Cb][HW] has images left_image_stride apart (Cb HW: the contiguous
 * output of branch1; 2 Cb HW: the first half of the unit's input).  A copy: every output carries the bits of an input element.
 * One launch.  N, Cb, HW >= 1. */
int ssdk_shuffle_join_fwd(const void* left, size_t left_image_stride, const void* right, void* y, int N, int Cb, int HW, int dtype,
                          void* stream);

/* Its backward: gleft[n][i] = gy[n][2i] (images gleft_image_stride apart), gright[n][i] = gy[n][2i + 1] (contiguous).  gleft may be
 * NULL (not computed; its stride is then ignored).  One launch. */
int ssdk_shuffle_join_bwd(const void* gy, void* gleft, size_t gleft_image_stride, void* gright, int N, int Cb, int HW, int dtype,
                          void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SSDK_SHUFFLETRAIN_H_ */
