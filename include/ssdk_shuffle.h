/*
 * ssdk_shuffle.h -- C-ABI of the ShuffleNetV2 unit as ONE launch (csrc/ssdk_shuffle.hip), part of libssdk.so.
 *
 * A header of its own next to ssdk.h, like ssdk_denselayer.h: the entry points of ssdk.h and the layout of ssdk_op are a closed list
 * under SSDK_VERSION 245, and this addition changes neither.  Conventions (pointers, streams, return values, zero-initialised
 * descriptors, ssdk_last_error) are those of ssdk.h.
 *
 * Tensors.  Dense NHWC, dtype SSDK_BF16 | SSDK_F16.  A tensor of C real channels has Cp = 8 * ceil(C / 8) channels per pixel.
 * A kernel READS only channels [0, C) of its input -- never the padding, whatever it holds -- and WRITES all
 * Cp channels of its output, zeros in [C, Cp): padding channels of a produced tensor are defined zeros, never garbage.
 *
 * The unit (ssds/modeling/nets/shufflenet.py InvertedResidual), with Cb = oup / 2 and C = 2 Cb output channels:
 *   stride 1 (ssdk_shuffle_unit)   left = x[..., :Cb]          right = branch2(x[..., Cb : 2 Cb])
 *   stride 2 (ssdk_shuffle_down)   left = branch1(x[..., :Cin])  right = branch2(x[..., :Cin])        Ho = (H - 1) / 2 + 1
 *   y[..., 2 i] = left[i], y[..., 2 i + 1] = right[i]           (channel_shuffle(cat(left, right), 2): one 32-bit word per pair)
 *   branch2:  m = round16( max(0, conv1x1(x, w1) * scale1 + bias1) )         lives in LDS on the tile plus a one-pixel halo
 *             d = round16( dw3x3/s(pad0(m), wd) * scale2 + bias2 )           no activation; lives in registers (an MFMA operand)
 *             r = round16( max(0, conv1x1(d, w3) * scale3 + bias3) )
 *   branch1:  e = round16( dw3x3/2(pad0(x), b1_wd) * b1_scale1 + b1_bias1 )  no activation
 *             l = round16( max(0, conv1x1(e, b1_w2) * b1_scale2 + b1_bias2) )
 * Rounding contract: every sum is accumulated in fp32 (v_mfma_f32_16x16x32_{bf16,f16} for the 1x1s, fp32 multiply-adds for the
 * depthwise); every folded BatchNorm affine is applied in fp32 (multiply, then add); each of the three stage outputs of branch2 (two of
 * branch1) is rounded ONCE to the tensor dtype, as a stored 16-bit tensor would be.  The depthwise pads its INPUT MAP with zeros: a
 * position of m outside the image is 0, not max(0, bias1).  The pass-through half of a stride-1 unit is copied bit for bit, in the
 * same store that writes the computed half.  No chunk, concatenation or shuffle exists as an operation.
 * One launch: no workspace, no allocation, no atomics, hipGraph-capturable, bit-reproducible.  y must not overlap x.
 *
 * Weights come zero-padded from the host (ssds/modeling/layers/fused_conv.py ShuffleUnitPack / ShuffleDownPack), so that the
 * kernels need no channel bound checks on them: with P = SSDK_SHUFFLE_CHUNK * ceil(Cb / SSDK_SHUFFLE_CHUNK) and KP = 32 * ceil(Cin / 32),
 *   1x1 weights  fragment-major images (ssdk_weight_frag_bytes) of the zero-padded matrix [P rows][P | KP columns], tensor dtype
 *   depthwise    [9 taps][P | KP] in the tensor dtype, tap = 3 ky + kx
 *   scale, bias  fp32 [P | KP], zeros in the padding (so a padding channel computes max(0, 0) = 0 at every stage)
 * Channel counts need NOT be multiples of 8, 16 or 32 (58, 116, 232; 122, 244, 488): middle channels are walked in chunks of 64 that
 * are self-contained for the depthwise, and the second 1x1 accumulates over the chunks in registers.
 *
 * Inside a recorded plan the two calls are executor ops SSDK_OP_SHUFFLE / SSDK_OP_SHUFFLEDOWN, described by existing members of
 * ssdk_op (include/ssdk.h).
 */
#ifndef SSDK_SHUFFLE_H_
#define SSDK_SHUFFLE_H_

#include "ssdk.h"

#ifdef __cplusplus
extern "C" {
#endif

/* output tile of a workgroup of ssdk_shuffle_unit (tests choose their ragged shapes from it) */
#define SSDK_SHUFFLE_TILE_H 4
#define SSDK_SHUFFLE_TILE_W 16
/* output tile of a workgroup of ssdk_shuffle_down (one MFMA pixel fragment; input channel counts above 512: half of it) */
#define SSDK_SHUFFLE_DOWN_TILE_H 4
#define SSDK_SHUFFLE_DOWN_TILE_W 4
/* middle channels per chunk: the weight images and vectors of a branch of Cb channels are zero-padded to P = CHUNK * ceil(Cb / CHUNK) */
#define SSDK_SHUFFLE_CHUNK 64

/* Stride-1 unit.  x, y [N][H][W][Cp], Cp = 8 * ceil(2 Cb / 8).  w1, w3: images of [P][P]; wd [9][P]; scale / bias fp32 [P].
 * Every pointer 16-byte aligned.  Accepted: what ssdk_shuffle_unit_supported accepts, N >= 1, N * tiles < 2^31, y disjoint from x;
 * anything else is SSDK_E_BADARG with a message before any launch. */
typedef struct ssdk_shuffle_unit_desc {
  const void* x;
  void* y;
  const void* w1;
  const float* scale1;
  const float* bias1;
  const void* wd;
  const float* scale2;
  const float* bias2;
  const void* w3;
  const float* scale3;
  const float* bias3;
  int32_t N, H, W, Cb, dtype;
} ssdk_shuffle_unit_desc;
int ssdk_shuffle_unit(const ssdk_shuffle_unit_desc* desc, void* stream);
size_t ssdk_shuffle_unit_desc_bytes(void);
/* 1 when ssdk_shuffle_unit takes a unit of Cb channels per branch on an H x W map, else 0: Cb even, 8 <= Cb <= 512,
 * 1 <= H, W <= 32768, dtype SSDK_BF16 | SSDK_F16.  Host only, touches no device: the single source of the rule. */
int ssdk_shuffle_unit_supported(int Cb, int H, int W, int dtype);

/* Stride-2 unit.  x [N][H][W][ld_in] of which channels [0, Cin) are read (ld_in = 0: 8 * ceil(Cin / 8); otherwise a multiple of
 * 8 that is >= Cin: the pixel stride of a wider tensor); y [N][Ho][Wo][8 * ceil(2 Cb / 8)].  Both branches are computed from ONE
 * staging of the input tile in LDS.  b1_wd [9][KP], b1_scale1 / b1_bias1 fp32 [KP], b1_w2 image of [P][KP], b1_scale2 / b1_bias2
 * fp32 [P]; w1 image of [P][KP]; wd, w3 and the other vectors as in ssdk_shuffle_unit_desc.  Every pointer 16-byte aligned. */
typedef struct ssdk_shuffle_down_desc {
  const void* x;
  void* y;
  const void* b1_wd;
  const float* b1_scale1;
  const float* b1_bias1;
  const void* b1_w2;
  const float* b1_scale2;
  const float* b1_bias2;
  const void* w1;
  const float* scale1;
  const float* bias1;
  const void* wd;
  const float* scale2;
  const float* bias2;
  const void* w3;
  const float* scale3;
  const float* bias3;
  int32_t N, H, W, Cin, ld_in, Cb, dtype;
} ssdk_shuffle_down_desc;
int ssdk_shuffle_down(const ssdk_shuffle_down_desc* desc, void* stream);
size_t ssdk_shuffle_down_desc_bytes(void);
/* 1 when ssdk_shuffle_down takes Cin input and Cb branch channels on an H x W input map, else 0: Cin even, 8 <= Cin <= 1024, Cb even,
 * 8 <= Cb <= 512, 1 <= H, W <= 32768, dtype SSDK_BF16 | SSDK_F16.  Host only: the single source of the rule. */
int ssdk_shuffle_down_supported(int Cin, int Cb, int H, int W, int dtype);

#ifdef __cplusplus
}
#endif
#endif /* SSDK_SHUFFLE_H_ */
