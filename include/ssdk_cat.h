/*
 * ssdk_cat.h -- C-ABI of the channel concatenation and the SPP block of the YOLO necks (csrc/ssdk_cat.hip), part of libssdk.so.
 *
 * A header of its own next to ssdk.h, like ssdk_convt.h: the entry points of ssdk.h and the layout of ssdk_op are a closed list
 * under SSDK_VERSION 245, and this addition changes neither.  Conventions (pointers, streams, return values, zero-initialised
 * descriptors, ssdk_last_error) are those of ssdk.h.
 *
 * Both operations are pure data movement and comparison on NHWC tensors of dtype SSDK_BF16 | SSDK_F16: every output element
 * is a copy of one input element, so the results carry the bits of the torch expressions they replace.  Each is ONE launch: no
 * allocation, no atomics, no synchronisation, hipGraph-capturable.  Anything outside the accepted set is SSDK_E_BADARG with a
 * message before any launch.  Neither descriptor is part of ssdk_struct_size(): ssdk_cat_desc_bytes() / ssdk_spp_desc_bytes()
 * report their sizes.  Inside a recorded plan the same calls are executor ops SSDK_OP_CAT / SSDK_OP_SPP, described by the op's
 * ssdk_conv_desc member (include/ssdk.h).
 */
#ifndef SSDK_CAT_H_
#define SSDK_CAT_H_

#include "ssdk.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Channel concatenation of a map with a second one at the same size or at half the size (ssds/yolo.py: YOLOv3 / PAN top-down
 * torch.cat((a, F.interpolate(b, scale_factor=2)), 1); PAN bottom-up torch.cat((a, b), 1)):
 *   y [N][H][W][C1 + C2] = a [N][H][W][C1]  ||  R(b)
 *   mode  SSDK_FUSE_SAME  b is [N][H][W][C2]
 *         SSDK_FUSE_UP2   b is [N][H/2][W/2][C2] and y[..][oy][ox][C1 + c] = b[..][oy/2][ox/2][c] (nearest); H and W even.
 *                         The upsampled tensor is never written.
 * Accepted: C1, C2 multiples of 8 (a lane moves 16 bytes), N, H, W >= 1, N H W < 2^31; a, b, y 16-byte aligned, none NULL. */
typedef struct ssdk_cat_desc {
  const void* a;
  const void* b;
  void* y;
  int32_t N, H, W, C1, C2, mode, dtype, pad;
} ssdk_cat_desc;
int ssdk_cat2(const ssdk_cat_desc* desc, void* stream);
size_t ssdk_cat_desc_bytes(void);

/* The SPP block (ssds/yolo.py SPPModule(3), max-pool): torch.cat([x] + [F.max_pool2d(x, k, 1, k // 2) for k in (5, 9, 13)], 1):
 *   y [N][H][W][4 C]: channels [0, C) are x, [C, 2C) / [2C, 3C) / [3C, 4C) the stride-1 maxima over windows 5 / 9 / 13.
 * The padding never wins: a maximum runs over the pixels of the window that lie inside the map, so any H, W >= 1 is accepted,
 * maps smaller than every window included.  The three pools come from ONE staging of x in LDS, in the separable form (maxima
 * along a row, then along a column -- exact for max on the clipped domain).  Values are ordered as numbers with -0 < +0; a
 * window that holds a NaN gives a NaN (of positive sign, whatever the sign and payload of the one torch would return).
 * Accepted: C a multiple of 8, N, H, W >= 1, N H W < 2^31; x, y 16-byte aligned, neither NULL. */
typedef struct ssdk_spp_desc {
  const void* x;
  void* y;
  int32_t N, H, W, C, dtype, pad;
} ssdk_spp_desc;
int ssdk_spp(const ssdk_spp_desc* desc, void* stream);
size_t ssdk_spp_desc_bytes(void);

#ifdef __cplusplus
}
#endif
#endif /* SSDK_CAT_H_ */
