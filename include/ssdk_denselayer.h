/*
 * ssdk_denselayer.h -- C-ABI of the DenseNet dense layer as ONE launch, and of the two small kernels a dense block needs around it
 * (csrc/ssdk_denselayer.hip), part of libssdk.so.
 *
 * A header of its own next to ssdk.h, like ssdk_dkres.h: the entry points of ssdk.h and the layout of ssdk_op are a closed list under
 * SSDK_VERSION 245, and this addition changes neither.  Conventions (pointers, streams, return values, zero-initialised descriptors,
 * ssdk_last_error) are those of ssdk.h.
 *
 * A dense block owns ONE buffer [N][H][W][ld] (NHWC with pixel stride ld channels, dtype SSDK_BF16 | SSDK_F16).  A dense layer
 * (ssds/modeling/nets/densenet.py _DenseLayer: conv3x3(ReLU(BN(conv1x1(ReLU(BN(cat(features)))))))) reads channels [0, Cin) of it
 * and writes its 32 new channels behind them, so the concatenation never exists as an operation.  With norm1 folded into the fp32
 * pair (a, b) and norm2 into (scale1, bias1):
 *   xa = round16( max(0, a[c] * x[..., c] + b[c]) )            c < Cin; applied on the way into the MFMA operand, never stored
 *   m  = round16( max(0, conv1x1(xa, w1) * scale1 + bias1) )   [N][H][W][128], lives in LDS, never written to memory
 *   y  = round16( conv3x3(pad0(m), w2) )                       32 channels, pixel stride ld; no BatchNorm, no activation
 * fp32 accumulation on v_mfma_f32_16x16x32_{bf16,f16}; the affines are done in fp32 (multiply, then add) and rounded once, as a stored
 * 16-bit tensor would be.  The 3x3 pads m with ZEROS: a position outside the image contributes nothing, whatever b and bias1 are.
 * One launch: no workspace, no allocation, no atomics, no synchronisation, hipGraph-capturable, bit-reproducible.
 *
 * x and y are pixel-0 pointers of two channel windows with the SAME pixel stride: x of the Cin channels read, y of the 32 channels
 * written.  Inside a block y == x + Cin elements.  Channels >= Cin of an x pixel are never read (in a plan they are uninitialised),
 * and nothing but the 32 channels of y is written.  y may live in the buffer x lives in as long as no written channel is a read one.
 *
 * Inside a recorded plan the three calls are executor ops SSDK_OP_DENSE / SSDK_OP_DENSEPOOL / SSDK_OP_DENSEPLACE, described by
 * existing members of ssdk_op (include/ssdk.h).
 */
#ifndef SSDK_DENSELAYER_H_
#define SSDK_DENSELAYER_H_

#include "ssdk.h"

#ifdef __cplusplus
extern "C" {
#endif

/* output tile of a workgroup (tests choose their ragged shapes from it) */
#define SSDK_DENSE_TILE_H 8
#define SSDK_DENSE_TILE_W 16
/* the only widths the registered DenseNets have: bn_size * growth middle channels, growth output channels */
#define SSDK_DENSE_CMID 128
#define SSDK_DENSE_COUT 32

/* w1 KRSC [128][Cin], w2 KRSC [32][3][3][128], tensor dtype; a / b fp32 [Cin], scale1 / bias1 fp32 [128].  w1_frag / w2_frag:
 * optional fragment-major images of w1 [128][Cin] and w2 [32][9 * 128] (ssdk_weight_frag_bytes), both or neither.  Every pointer
 * 16-byte aligned.  Accepted: what ssdk_dense_layer_supported(Cin, H, W, ld, dtype) accepts, N >= 1, N * tiles < 2^31, y's channels
 * disjoint from x's; anything else is SSDK_E_BADARG with a message before any launch. */
typedef struct ssdk_dense_layer_desc {
  const void* x;
  void* y;
  const void* w1;
  const float* a;
  const float* b;
  const float* scale1;
  const float* bias1;
  const void* w2;
  const void* w1_frag;
  const void* w2_frag;
  int32_t N, H, W, Cin, ld, dtype;
} ssdk_dense_layer_desc;
int ssdk_dense_layer(const ssdk_dense_layer_desc* desc, void* stream);
size_t ssdk_dense_layer_desc_bytes(void);
/* 1 when ssdk_dense_layer takes a layer of Cin input channels on an H x W map in a buffer of pixel stride ld, else 0:
 * Cin % 32 == 0, 32 <= Cin <= 2048, ld % 8 == 0, ld >= Cin + 32, 1 <= H, W <= 32768, dtype SSDK_BF16 | SSDK_F16.  Host only, touches
 * no device: the single source of the rule. */
int ssdk_dense_layer_supported(int Cin, int H, int W, int ld, int dtype);

/* Front of a transition (_Transition: norm, relu, conv 1x1, avgpool 2x2): p = round16( mean over the 2x2 window of
 * max(0, a[c] * x[..., c] + b[c]) ), x [N][H][W] with pixel stride ld, channels [0, C); y dense [N][H/2][W/2][C] (floor, like
 * AvgPool2d(2, 2)).  The transition's 1x1 is linear and has no bias, so it commutes with the average and runs BEHIND this kernel on a
 * quarter of the pixels.  C % 8 == 0, 8 <= C <= ld, ld % 8 == 0, 2 <= H, W <= 32768, N >= 1; pointers 16-byte aligned; y must not overlap
 * the buffer.  Anything else: SSDK_E_BADARG. */
typedef struct ssdk_dense_pool_desc {
  const void* x;
  void* y;
  const float* a;
  const float* b;
  int32_t N, H, W, C, ld, dtype;
} ssdk_dense_pool_desc;
int ssdk_dense_pool(const ssdk_dense_pool_desc* desc, void* stream);
size_t ssdk_dense_pool_desc_bytes(void);

/* Copies a dense x [N][H][W][C] into channels [0, C) of y, a buffer [N][H][W] of pixel stride ld (16 bytes per lane); the other
 * channels of y are not touched.  C % 8 == 0, 8 <= C <= ld, ld % 8 == 0, 1 <= H, W <= 32768, N >= 1; pointers 16-byte aligned; x must
 * not overlap the buffer.  Anything else: SSDK_E_BADARG. */
typedef struct ssdk_dense_place_desc {
  const void* x;
  void* y;
  int32_t N, H, W, C, ld, dtype;
} ssdk_dense_place_desc;
int ssdk_dense_place(const ssdk_dense_place_desc* desc, void* stream);
size_t ssdk_dense_place_desc_bytes(void);

#ifdef __cplusplus
}
#endif
#endif /* SSDK_DENSELAYER_H_ */
