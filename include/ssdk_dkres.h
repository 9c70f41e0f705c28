/*
 * ssdk_dkres.h -- C-ABI of the DarkNet residual block as ONE launch (csrc/ssdk_dkres.hip), part of libssdk.so.
 *
 * A header of its own next to ssdk.h, like ssdk_convt.h and ssdk_cat.h: the entry points of ssdk.h and the layout of ssdk_op are a
 * closed list under SSDK_VERSION 245, and this addition changes neither.  Conventions (pointers, streams, return values,
 * zero-initialised descriptors, ssdk_last_error) are those of ssdk.h.
 *
 * The block (ssds/modeling/nets/darknet.py Residual: x + act(BN(conv3x3(act(BN(conv1x1(x))))))), C -> C/2 -> C, on NHWC tensors of
 * dtype SSDK_BF16 | SSDK_F16 with the BatchNorms folded into fp32 (scale, bias) pairs:
 *   m = round16( act1( conv1x1(x, w1) * scale1 + bias1 ) )                 [N][H][W][C/2], lives in LDS, never written to memory
 *   y = round16( act2( conv3x3(pad0(m), w2) * scale2 + bias2 ) + x )       [N][H][W][C]
 * fp32 accumulation on v_mfma_f32_16x16x32_{bf16,f16}; m is rounded to the tensor dtype as a stored tensor would be; the add is done in
 * fp32 and y is rounded ONCE.  The 3x3 pads m with ZEROS: a position outside the image contributes nothing, whatever bias1 is.
 * One launch: no workspace, no allocation, no atomics, no synchronisation, hipGraph-capturable, bit-reproducible.
 *
 * A workgroup owns a tile of SSDK_DKRES_TILE_H x SSDK_DKRES_TILE_W output pixels and reads x on the tile and a one-pixel halo, so
 * the operation cannot run in place: y must not overlap x.
 *
 * Inside a recorded plan the same call is executor op SSDK_OP_DKRES, described by the op's ssdk_xpair_desc member (include/ssdk.h).
 */
#ifndef SSDK_DKRES_H_
#define SSDK_DKRES_H_

#include "ssdk.h"

#ifdef __cplusplus
extern "C" {
#endif

/* output tile of a workgroup (tests choose their ragged shapes from it) */
#define SSDK_DKRES_TILE_H 8
#define SSDK_DKRES_TILE_W 16

/* w1 KRSC [C/2][C], w2 KRSC [C][3][3][C/2], tensor dtype; scale1 / bias1 fp32 [C/2], scale2 / bias2 fp32 [C]; act1 / act2
 * SSDK_ACT_NONE | SSDK_ACT_RELU | SSDK_ACT_RELU6.  w1_frag / w2_frag: optional fragment-major images of w1 [C/2][C] and
 * w2 [C][9 C/2] (ssdk_weight_frag_bytes), both or neither.  Every pointer 16-byte aligned.
 * Accepted: what ssdk_dkres_supported(C, H, W, dtype) accepts, N >= 1, N * tiles < 2^31, y not overlapping x; anything else is
 * SSDK_E_BADARG with a message before any launch. */
typedef struct ssdk_dkres_desc {
  const void* x;
  void* y;
  const void* w1;
  const float* scale1;
  const float* bias1;
  const void* w2;
  const float* scale2;
  const float* bias2;
  const void* w1_frag;
  const void* w2_frag;
  int32_t N, H, W, C, act1, act2, dtype, pad;
} ssdk_dkres_desc;
int ssdk_dkres(const ssdk_dkres_desc* desc, void* stream);
size_t ssdk_dkres_desc_bytes(void);
/* 1 when ssdk_dkres takes a block of width C on an H x W map in dtype, else 0: C 64 | 128 | 256 (a tile of m plus its halo fits
 * LDS several times over, so three workgroups share a CU; at C = 512 one tile takes 99 KiB and at C = 1024 it does not fit),
 * 1 <= H, W <= 32768, dtype SSDK_BF16 | SSDK_F16.  Host only, touches no device: the single source of the rule. */
int ssdk_dkres_supported(int C, int H, int W, int dtype);

#ifdef __cplusplus
}
#endif
#endif /* SSDK_DKRES_H_ */
