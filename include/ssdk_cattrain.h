/*
 * ssdk_cattrain.h -- C-ABI of the channel concatenation and the SPP block of the YOLO TRAINING step, forward and backward
 * (csrc/ssdk_cattrain.hip), part of libssdk.so.
 *
 * A header of its own next to ssdk.h, like ssdk_cat.h and ssdk_convt.h: the entry points of ssdk.h are a closed list under
 * SSDK_VERSION 245, and this addition changes neither.  Conventions (pointers, streams, return values, ssdk_last_error) are those
 * of ssdk.h.
 *
 * All tensors are contiguous NCHW of dtype SSDK_BF16 | SSDK_F16 (ssdk_cat.h is the NHWC, forward-only form the recorded plan
 * runs).  Every call is ONE launch: no allocation, no workspace, no synchronisation, no atomics, hipGraph-capturable.  Every output
 * element is written exactly once, sums are fp32 in a fixed order with one rounding, and the results are bit-reproducible.  Any
 * N, C, C1, C2, H, W >= 1 with fewer than 2^31 elements per tensor is accepted, planes whose start is not 16-byte aligned (5 x 7)
 * included; pointers need the 2-byte alignment of an element.  Anything else is SSDK_E_BADARG with a message before any launch.
 */
#ifndef SSDK_CATTRAIN_H_
#define SSDK_CATTRAIN_H_

#include "ssdk.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Channel concatenation (ssds/yolo.py: torch.cat((a, F.interpolate(b, scale_factor=2)), 1) and torch.cat((a, b), 1)):
 *   y [N][C1 + C2][H][W] = a [N][C1][H][W]  ||  R(b)
 *   mode  SSDK_FUSE_SAME  b is [N][C2][H][W]
 *         SSDK_FUSE_UP2   b is [N][C2][H/2][W/2], y[n][C1 + c][oy][ox] = b[n][c][oy/2][ox/2] (nearest); H and W even.
 *                         The upsampled tensor is never written.
 * Every output carries the bits of an input element. */
int ssdk_cat_train_fwd(const void* a, const void* b, void* y, int N, int C1, int C2, int H, int W, int mode, int dtype, void* stream);

/* Its backward: gy [N][C1 + C2][H][W] -> ga [N][C1][H][W], the contiguous copy of gy[:, :C1], and gb: under SSDK_FUSE_SAME the
 * copy of gy[:, C1:], under SSDK_FUSE_UP2 [N][C2][H/2][W/2] with gb[..][y][x] = ((g00 + g01) + g10) + g11 over the 2 x 2 block of
 * gy in row-major order, in fp32, rounded once (the rule of ssdk_neck_fuse_bwd).  Either of ga, gb may be NULL (not computed). */
int ssdk_cat_train_bwd(const void* gy, void* ga, void* gb, int N, int C1, int C2, int H, int W, int mode, int dtype, void* stream);

/* The largest plane side the SPP kernels stage in LDS: H <= 64 and W <= 64 (36 KiB of LDS per workgroup in the backward at 64 x 64,
 * 2.25 KiB at the 16 x 16 map of yolov4_resnet18_512, so several workgroups share a CU).  A larger H or W is SSDK_E_BADARG. */
#define SSDK_SPP_TRAIN_MAX_SIDE 64

/* The SPP block (ssds/yolo.py SPPModule(3), max-pool): torch.cat([x] + [F.max_pool2d(x, k, 1, k // 2) for k in (5, 9, 13)], 1):
 *   y [N][4 C][H][W]: channels [0, C) are x, [C, 2C) / [2C, 3C) / [3C, 4C) the stride-1 maxima over windows 5 / 9 / 13.
 * The padding never wins: a maximum runs over the pixels of the window that lie inside the map.  The three pools come from ONE
 * staging of the plane, in the separable form.  Comparison is numeric (-0 == +0: either zero may be returned); a window that holds
 * a NaN gives a NaN. */
int ssdk_spp_train_fwd(const void* x, void* y, int N, int C, int H, int W, int dtype, void* stream);

/* Its backward: x [N][C][H][W], gy [N][4 C][H][W] -> gx [N][C][H][W].  No index tensor exists: the arg-max of every window is
 * recomputed from x by torch's rule -- the FIRST maximum in row-major order of the clipped window under NUMERIC comparison, so
 * -0 == +0 (the packed-key order of ssdk_spp, -0 < +0, would route differently), and a NaN is a maximum: a window holding one
 * sends its gradient to a NaN element of the window.  It is a gather: gx[p] is the fp32 sum, rounded once, of gy_0[p] and then, for
 * k = 5, 9, 13 in that order, gy_k[q] over the output positions q in row-major order whose window's arg-max is p. */
int ssdk_spp_train_bwd(const void* x, const void* gy, void* gx, int N, int C, int H, int W, int dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SSDK_CATTRAIN_H_ */
