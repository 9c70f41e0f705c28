/*
 * ssdk_densetrain.h -- C-ABI of the DenseNet dense-block TRAINING step (csrc/ssdk_densetrain.hip), part of libssdk.so.  A dense block
 * trains on ONE feature buffer F [N][Ctot][HW] and ONE gradient buffer G of the same shape: layer j reads the channel prefix
 * [0, K_j) of F where it lies and writes its new channels behind it, so there is no concatenation, and relu(norm1(x)) is never
 * stored -- the first 1x1 of a layer applies the BatchNorm's coefficients while it stages its operand.
 *
 * A header of its own next to ssdk.h, like ssdk_shuffletrain.h: the entry points of ssdk.h are a closed list under SSDK_VERSION 245, and
 * this addition changes neither.  Conventions (pointers, streams, return values, ssdk_last_error) are those of ssdk.h, and those of
 * ssdk_shuffletrain.h for tensors: NCHW of dtype SSDK_BF16 | SSDK_F16, HW = H * W, fp32 accumulation; a tensor with an "image stride" is
 * a channel slice of a wider tensor (the channel offset folded into the pointer, the distance in ELEMENTS between two images passed;
 * >= channels * HW of the slice).  Tensor pointers need 2-byte alignment, fp32 vectors 4 bytes, weight matrices, coef and workspaces
 * 16 bytes.  No allocation, no synchronisation, no atomics, hipGraph-capturable; sums are in a fixed order: bit-reproducible.  Every
 * argument is checked before any launch: null pointers, K or M < 8, a bad lda, an image stride smaller than the slice, a dtype that
 * is not 16 bit, a tensor of 2^32 elements or more (counted over the image strides) are SSDK_E_BADARG with a message, a small
 * workspace is SSDK_E_WORKSPACE.
 *
 * coef [K][4] fp32 = (a, b, ., .) per channel as ssdk_bn_act_train_stats writes it.  The operand transform of the two GEMM entries is
 *     op(x)_c = round_dtype(max(fmaf(a_c, x_c, b_c), 0))
 * -- one fused multiply-add in fp32, the ReLU, ONE rounding to the tensors' dtype; the ReLU's gradient mask of the two bn1 entries is
 * fmaf(a_c, x_c, b_c) > 0 (strict, on the fp32 value).
 */
#ifndef SSDK_DENSETRAIN_H_
#define SSDK_DENSETRAIN_H_

#include "ssdk.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of workspace ssdk_dense_train_place needs (0 on bad arguments). */
size_t ssdk_dense_train_place_workspace_bytes(int N, int C, int HW);

/* y[n][c] = t[n][c], bit for bit: t [N][C][HW] contiguous, y a C-channel slice with images y_image_stride apart (the block's input
 * features, or a layer's new channels, on their place in F).  sums [C][2] fp32 = per channel (sum, sum of squares) of the STORED
 * values over N * HW, in a fixed order through `workspace` (16-byte aligned): the batch statistics of every later layer's norm1 for
 * this channel.  Nothing outside the slice is written.  Two launches (copy + partial sums, finalize).  N, C, HW >= 1. */
int ssdk_dense_train_place(const void* t, void* y, size_t y_image_stride, float* sums, void* workspace, size_t workspace_bytes, int N,
                           int C, int HW, int dtype, void* stream);

/* m[b] = a op(x[b]): x [B][K][HW] with images x_image_stride apart (the prefix of F), coef [K][4], a [M][lda] row-major in the tensors'
 * dtype (w16 of ssdk_pws_prepare: lda % 8 == 0, lda >= K, 16-byte aligned), m [B][M][HW] contiguous.  K, M >= 8 are any values.
 * Channels >= K of x are never read.  sums (optional) [M][2] fp32 as in ssdk_pws_forward, with `workspace` of
 * ssdk_pws_stats_workspace_bytes(B, K, M, HW) (same launch geometry); with sums == NULL the workspace is not used.  One launch
 * (+ the fixed-order reduction of the sums). */
int ssdk_dense_train_pw_forward(const void* x, size_t x_image_stride, const float* coef, const void* a, int lda, void* m, float* sums,
                                void* workspace, size_t workspace_bytes, int B, int K, int M, int HW, int dtype, void* stream);

/* dw [M][K] fp32 = sum_b dm[b] op(x[b])^T: dm [B][M][HW] contiguous, x and coef as above.  The plan, the workspace rule
 * (ssdk_pws_wgrad_workspace_bytes(B, M, K, HW)) and the summation order of ssdk_pws_wgrad.  M, K >= 8. */
int ssdk_dense_train_pw_wgrad(const void* dm, const void* x, size_t x_image_stride, const float* coef, float* dw, void* workspace,
                              size_t workspace_bytes, int B, int M, int K, int HW, int dtype, void* stream);

/* Bytes of workspace ssdk_dense_train_bn1_reduce needs (0 on bad arguments). */
size_t ssdk_dense_train_bn1_workspace_bytes(int N, int K, int HW);

/* The reduction of norm1's backward: red [K][2] fp32 = (sum g, sum g xhat) over N * HW per channel, g = s [fmaf(a, x, b) > 0],
 * xhat = (x - save_mean) save_invstd.  s [N][K][HW] contiguous is the raw input gradient W1^T dm (ssdk_pws_forward on wt16), x the
 * prefix of F.  red[c][0] is the gradient of norm1's bias, red[c][1] that of its weight.  Fixed order through `workspace` (16-byte
 * aligned).  Two launches.  K >= 1. */
int ssdk_dense_train_bn1_reduce(const void* s, const void* x, size_t x_image_stride, const float* coef, const float* save_mean,
                                const float* save_invstd, float* red, void* workspace, size_t workspace_bytes, int N, int K, int HW,
                                int dtype, void* stream);

/* g[n][c] = round_dtype(g[n][c] + weight_c invstd_c (gm - red[c][0] / n - xhat red[c][1] / n)), n = N * HW, gm the masked s as above:
 * norm1's input gradient ADDED to the prefix [0, K) of the block's gradient buffer (images g_image_stride apart).  The sum is formed
 * in fp32 and rounded once.  Channels >= K of g are neither read nor written.  One launch. */
int ssdk_dense_train_bn1_apply(const void* s, const void* x, size_t x_image_stride, const float* coef, const float* save_mean,
                               const float* save_invstd, const float* weight, const float* red, void* g, size_t g_image_stride, int N,
                               int K, int HW, int dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SSDK_DENSETRAIN_H_ */
