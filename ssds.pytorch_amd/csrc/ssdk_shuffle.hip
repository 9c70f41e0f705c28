// ssdk_shuffle.hip -- one ShuffleNetV2 unit (nets/shufflenet.py InvertedResidual) as ONE launch on gfx950 (include/ssdk_shuffle.h):
//   stride 1  y[2i] = x[i],             y[2i + 1] = branch2(x[Cb:])[i]      shuffle_unit_kernel
//   stride 2  y[2i] = branch1(x)[i],    y[2i + 1] = branch2(x)[i]           shuffle_down_kernel
// branch2 = 1x1 + BN + ReLU, depthwise 3x3 + BN, 1x1 + BN + ReLU; branch1 = depthwise 3x3 / 2 + BN, 1x1 + BN + ReLU.
//
// Why: on library kernels the unit is chunk, three convolutions with a BatchNorm pass each, cat and a five-dimensional transpose: six
// or more passes over a tensor whose arithmetic is almost nothing.  Here x is read once and y written once; the interleave of the
// channel shuffle is the ADDRESS of the store (one 32-bit word per channel pair), and the pass-through half rides in that store.
//
// Channel counts are not multiples of 8, 16 or 32 (Cb = 58, 116, 232; 122, 244, 488).  The host zero-pads every weight image and
// vector to P = 64 ceil(Cb / 64), so only the loads of x need a bound: sh_load8 never touches a channel pair at or past the limit.
// Middle channels are walked in chunks of 64 (the scheme of ssdk_mbk.hip: the depthwise is per channel, so a chunk is
// self-contained): per chunk
//   phase 1  m[hp][64] = relu(bn1(W1[chunk] . x[hp])) on the output tile plus its one-pixel halo, MFMA 16x16x32 -> LDS (row stride
//            144 B).  A halo position OUTSIDE THE IMAGE gets ZEROS, not relu(bias1): the depthwise pads m, not x.
//   phase 2  d = bn2(dw3x3(m)): each lane computes 8 channels of ONE output pixel from LDS in fp32 -- exactly the B operand fragment
//            of the second 1x1, so d never leaves registers
//   phase 3  acc[co] += W3[co][chunk] . d, accumulated over the chunks in registers
// Stride 1: tile 4 x 16 (halo 6 x 18 = 108 -> 7 fragments of 16 pixels); wave w owns halo fragments w, w + 4 in phase 1 and the 16
// output pixels of tile row w with ALL output channels in phases 2 / 3 (P / 16 accumulator fragments: the kernel is
// instantiated for 4, 8, 16 and 32).  LDS 112 x 144 B = 15.75 KiB.
// Stride 2: tile 4 x 4 = one pixel fragment (input halo 9 x 9 = 81 -> 6 fragments), the input tile staged ONCE in LDS
// ([96][KP + 8] elements) and read from there by branch1's depthwise and branch2's first 1x1; wave w owns output-channel fragments
// w, w + 4, ... of both branches (8 + 8 accumulator fragments at most).  Input channel counts above 512: tile 2 x 4, so that the
// staged tile stays below 112 KiB.
#include "ssdk_conv_common.h"
#include "../../include/ssdk_shuffle.h"

namespace ssdk {

constexpr int kShThreads = 256;
constexpr int kShCH = SSDK_SHUFFLE_CHUNK;  // middle channels per chunk
constexpr int kShMS = kShCH * 2 + 16;      // LDS row stride of the middle chunk (bytes)
constexpr int kShTH = SSDK_SHUFFLE_TILE_H, kShTW = SSDK_SHUFFLE_TILE_W;
constexpr int kShHW = kShTW + 2;                  // width of the halo tile
constexpr int kShHP = (kShTH + 2) * (kShTW + 2);  // 108 halo pixels
constexpr int kShNF = (kShHP + 15) / 16;          // 7 pixel fragments
constexpr size_t kShLds = (size_t)kShNF * 16 * kShMS;
static_assert(kShCH == 64 && kShTH == 4 && kShTW == 16 && kShNF <= 8, "tile: one wave per output row, one lane group per pixel");

// 8 channels [k, k + 8) of a pixel (px32: its channel 0, as 32-bit words; k even) whose real channels end at lim (even): a pair at or
// past lim reads as zero and its memory is never touched.  The pixel need only be 4-byte aligned (Cb = 58: byte offset 116).
__device__ __forceinline__ u32x4 sh_load8(const u32* px32, int k, int lim) {
  u32x4 v = {0u, 0u, 0u, 0u};
  const u32* s = px32 + (k >> 1);
  if (k + 8 <= lim) {
    __builtin_memcpy(&v, s, 16);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (k + 2 * j < lim) v[j] = s[j];
  }
  return v;
}

// depthwise 3x3 + BN on an LDS map, 8 channels of one output position: tap0 = this lane's 8 channels at tap (0, 0), rowB / pixB the
// byte strides of a map row / pixel; wd = the 8 channels' weights of tap 0 ([9][ldw]); sc / bi the 8 channels' affine.  fp32, rounded once.
template <int DT>
__device__ __forceinline__ u32x4 sh_dw8(const unsigned char* tap0, int rowB, int pixB, const u16* wd, int ldw, const float* sc,
                                        const float* bi) {
  float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int t = 0; t < 9; ++t) {
    const u32x4 m = *reinterpret_cast<const u32x4*>(tap0 + (t / 3) * rowB + (t % 3) * pixB);
    const u32x4 w = *reinterpret_cast<const u32x4*>(wd + (size_t)t * ldw);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      s[2 * j] += bits16_to_f32<DT>(m[j] & 0xffffu) * bits16_to_f32<DT>(w[j] & 0xffffu);
      s[2 * j + 1] += bits16_to_f32<DT>(m[j] >> 16) * bits16_to_f32<DT>(w[j] >> 16);
    }
  }
  const f32x4 s0 = *reinterpret_cast<const f32x4*>(sc), s1 = *reinterpret_cast<const f32x4*>(sc + 4);
  const f32x4 b0 = *reinterpret_cast<const f32x4*>(bi), b1 = *reinterpret_cast<const f32x4*>(bi + 4);
  u32x4 o;
  o[0] = pack2_16<DT>(s[0] * s0[0] + b0[0], s[1] * s0[1] + b0[1]);
  o[1] = pack2_16<DT>(s[2] * s0[2] + b0[2], s[3] * s0[3] + b0[3]);
  o[2] = pack2_16<DT>(s[4] * s1[0] + b1[0], s[5] * s1[1] + b1[1]);
  o[3] = pack2_16<DT>(s[6] * s1[2] + b1[2], s[7] * s1[3] + b1[3]);
  return o;
}

// the interleaved store of 4 channel pairs (left[co + r], right[co + r]), r < 4, at y[2 co ...]: right = relu(acc * sc + bi) rounded
// once; pairs at or past Cb are the zeros of the padding channels [2 Cb, Cp)
template <int DT>
__device__ __forceinline__ void sh_store4(u16* ypix, int co, int Cb, const f32x4 acc, const float* sc, const float* bi, uint2 left) {
  const f32x4 s = *reinterpret_cast<const f32x4*>(sc + co), b = *reinterpret_cast<const f32x4*>(bi + co);
  u32x4 o;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const u32 rt = f32_to_bits16<DT>(__builtin_fmaxf(acc[r] * s[r] + b[r], 0.f)) & 0xffffu;
    const u32 lf = ((r < 2 ? left.x : left.y) >> (16 * (r & 1))) & 0xffffu;
    o[r] = co + r < Cb ? (lf | (rt << 16)) : 0u;
  }
  *reinterpret_cast<u32x4*>(ypix + 2 * co) = o;
}

struct ShUnitParams {
  const u16* x;
  u16* y;
  const u16* w1;
  const float* s1;
  const float* b1;
  const u16* wd;
  const float* s2;
  const float* b2;
  const u16* w3;
  const float* s3;
  const float* b3;
  int H, W, tiles_y, tiles_x, Cb, Cp, P;
};

// NCO: accumulator fragments (16 output channels each) a wave holds, P <= 16 NCO
template <int DT, int NCO>
__global__ __launch_bounds__(kShThreads, NCO <= 16 ? 2 : 1) void shuffle_unit_kernel(const ShUnitParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const u32 tid = threadIdx.x, lane = tid & 63u, wave = (u32)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
  const u32 fr = lane & 15u, fg = lane >> 4;
  int blk = (int)blockIdx.x;
  const int tx0 = (blk % p.tiles_x) * kShTW;
  blk /= p.tiles_x;
  const int ty0 = (blk % p.tiles_y) * kShTH;
  const int n = blk / p.tiles_y;
  const int H = p.H, W = p.W, Cb = p.Cb, Cp = p.Cp, P = p.P;
  const int K1 = (Cb + 31) >> 5;  // k-steps of the first 1x1 that hold a real input channel
  const int KP = P >> 5;          // k-steps per row fragment of the weight images
  const int nco = P >> 4, nchunks = P / kShCH;
  const size_t img = (size_t)n * H * W * Cp;

  // phase 1: this wave's halo fragments wave and wave + 4 (the second one: waves 0..2)
  const bool have1 = wave + 4 < (u32)kShNF;  // (wave-uniform)
  const u32* xa[2];
  u32 row[2];
  bool inside[2];
#pragma unroll
  for (int m = 0; m < 2; ++m) {
    const int hp = ((int)wave + 4 * m) * 16 + (int)fr;
    const int hy = hp / kShHW, hx = hp - hy * kShHW;
    int iy = ty0 - 1 + hy, ix = tx0 - 1 + hx;
    inside[m] = hp < kShHP && (unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W;
    if (!inside[m]) iy = ty0, ix = tx0;  // computed on a pixel of the image, stored as zeros
    xa[m] = reinterpret_cast<const u32*>(p.x + img + ((size_t)iy * W + ix) * Cp + Cb);  // the right half: channels [Cb, 2 Cb)
    row[m] = (u32)hp * kShMS;
  }
  // phases 2 / 3: output pixel fr of fragment wave = tile row wave
  const int py = (int)wave, px = (int)fr;
  const unsigned char* tap0 = smem + (py * kShHW + px) * kShMS + fg * 16u;

  f32x4 acc[NCO];
#pragma unroll
  for (int a = 0; a < NCO; ++a) acc[a] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int chunk = 0; chunk < nchunks; ++chunk) {
    {
      f32x4 a1[4][2];
#pragma unroll
      for (int a = 0; a < 4; ++a) a1[a][0] = a1[a][1] = f32x4{0.f, 0.f, 0.f, 0.f};
      const u16* wa = p.w1 + (size_t)(chunk * 4) * KP * 512 + lane * 8;
      for (int ks = 0; ks < K1; ++ks) {
        const int k = ks * 32 + (int)fg * 8;
        const u32x4 xb0 = sh_load8(xa[0], k, Cb);
        u32x4 xb1 = {0u, 0u, 0u, 0u};
        if (have1) xb1 = sh_load8(xa[1], k, Cb);
#pragma unroll
        for (int a = 0; a < 4; ++a) {
          const u32x4 rw = *reinterpret_cast<const u32x4*>(wa + ((size_t)a * KP + ks) * 512);
          a1[a][0] = mfma16<DT>(rw, xb0, a1[a][0]);  // D[cm = 4fg + r][px = fr]
          if (have1) a1[a][1] = mfma16<DT>(rw, xb1, a1[a][1]);
        }
      }
#pragma unroll
      for (int a = 0; a < 4; ++a) {
        const int cl = a * 16 + (int)fg * 4, cm = chunk * kShCH + cl;
        const f32x4 sc = *reinterpret_cast<const f32x4*>(p.s1 + cm), bi = *reinterpret_cast<const f32x4*>(p.b1 + cm);
#pragma unroll
        for (int m = 0; m < 2; ++m) {
          if (m == 1 && !have1) continue;
          float v[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) v[r] = inside[m] ? __builtin_fmaxf(a1[a][m][r] * sc[r] + bi[r], 0.f) : 0.f;
          *reinterpret_cast<uint2*>(smem + row[m] + cl * 2) = make_uint2(pack2_16<DT>(v[0], v[1]), pack2_16<DT>(v[2], v[3]));
        }
      }
    }
    __syncthreads();  // the middle chunk is complete
#pragma unroll
    for (int ks2 = 0; ks2 < 2; ++ks2) {
      const int c = chunk * kShCH + ks2 * 32 + (int)fg * 8;
      const u32x4 d = sh_dw8<DT>(tap0 + ks2 * 64, kShHW * kShMS, kShMS, p.wd + c, P, p.s2 + c, p.b2 + c);
      const u16* wb = p.w3 + (size_t)(chunk * 2 + ks2) * 512 + lane * 8;
#pragma unroll
      for (int a = 0; a < NCO; ++a) {
        if (a < nco) {  // (uniform)
          const u32x4 rw = *reinterpret_cast<const u32x4*>(wb + (size_t)a * KP * 512);
          acc[a] = mfma16<DT>(rw, d, acc[a]);  // D[co = 4fg + r][px = fr]
        }
      }
    }
    __syncthreads();  // every wave has read the chunk: the next one may overwrite it
  }

  const int oy = ty0 + py, ox = tx0 + px;
  if (oy < H && ox < W) {
    const size_t off = img + ((size_t)oy * W + ox) * Cp;
    const u16* xpix = p.x + off;
    u16* ypix = p.y + off;
#pragma unroll
    for (int a = 0; a < NCO; ++a) {
      const int co = a * 16 + (int)fg * 4;
      if (a < nco && 2 * co < Cp) {
        uint2 left = make_uint2(0u, 0u);
        if (co < Cb) left = *reinterpret_cast<const uint2*>(xpix + co);  // channels co .. co + 3 < 2 Cb: the pass-through half
        sh_store4<DT>(ypix, co, Cb, acc[a], p.s3, p.b3, left);
      }
    }
  }
}

struct ShDownParams {
  const u16* x;
  u16* y;
  const u16* b1_wd;
  const float* b1_s1;
  const float* b1_b1;
  const u16* b1_w2;
  const float* b1_s2;
  const float* b1_b2;
  const u16* w1;
  const float* s1;
  const float* b1;
  const u16* wd;
  const float* s2;
  const float* b2;
  const u16* w3;
  const float* s3;
  const float* b3;
  int H, W, Ho, Wo, tiles_y, tiles_x, Cin, ld, KP, Cb, Cp, P;
};

constexpr int kShDnAcc = 8;  // accumulator fragments per wave and branch: P <= 512 = 4 waves x 8 x 16

template <int TH, int TW>
struct ShDownTile {
  static constexpr int HH = 2 * TH + 1, HW = 2 * TW + 1, HP = HH * HW, NF = (HP + 15) / 16, ROWS = NF * 16;
};
static size_t sh_down_lds(int rows, int KP) { return (size_t)rows * ((size_t)KP * 2 + 16 + kShMS); }

template <int DT, int TH, int TW>
__global__ __launch_bounds__(kShThreads) void shuffle_down_kernel(const ShDownParams p) {
  typedef ShDownTile<TH, TW> T;
  static_assert(TH * TW <= 16, "one pixel fragment");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const u32 tid = threadIdx.x, lane = tid & 63u, wave = (u32)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
  const u32 fr = lane & 15u, fg = lane >> 4;
  int blk = (int)blockIdx.x;
  const int tx0 = (blk % p.tiles_x) * TW;
  blk /= p.tiles_x;
  const int ty0 = (blk % p.tiles_y) * TH;
  const int n = blk / p.tiles_y;
  const int H = p.H, W = p.W, Cin = p.Cin, KP = p.KP, Cb = p.Cb, Cp = p.Cp, P = p.P;
  const int KS = KP >> 5, KPP = P >> 5, nco = P >> 4, nchunks = P / kShCH;
  const int XS = KP * 2 + 16;  // LDS row stride of the staged input tile (bytes)
  unsigned char* xs = smem;
  unsigned char* ms = smem + (size_t)T::ROWS * XS;
  const size_t ximg = (size_t)n * H * W * p.ld;
  const int iy0 = 2 * ty0 - 1, ix0 = 2 * tx0 - 1;

  // ---- the ONE staging of the input tile: channels [0, Cin) of the halo pixels, zeros outside the image and in [Cin, KP) ----------
  {
    const int G = KP >> 3;  // 16-byte groups per pixel
    for (int i = (int)tid; i < T::ROWS * G; i += kShThreads) {
      const int hp = i / G, g = i - hp * G;
      const int hy = hp / T::HW, hx = hp - hy * T::HW;
      const int iy = iy0 + hy, ix = ix0 + hx;
      u32x4 v = {0u, 0u, 0u, 0u};
      if (hp < T::HP && (unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W && g * 8 < Cin)
        v = sh_load8(reinterpret_cast<const u32*>(p.x + ximg + ((size_t)iy * W + ix) * p.ld), g * 8, Cin);
      *reinterpret_cast<u32x4*>(xs + (size_t)hp * XS + g * 16) = v;
    }
  }
  __syncthreads();

  // output pixel fr of the tile (lanes past TH * TW compute pixel 0 again and store nothing)
  const bool pvalid = fr < (u32)(TH * TW);
  const int ty = pvalid ? (int)fr / TW : 0, tx = pvalid ? (int)fr % TW : 0;
  const int tapi = (2 * ty) * T::HW + 2 * tx;  // halo index of tap (0, 0)

  // ---- branch 1: e = bn(dw3x3/2(x)) from the staged tile, left = relu(bn(W . e)); this wave's fragments wave, wave + 4, ... ----------
  f32x4 acc1[kShDnAcc], acc2[kShDnAcc];
#pragma unroll
  for (int a = 0; a < kShDnAcc; ++a) acc1[a] = acc2[a] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int ks = 0; ks < KS; ++ks) {
    const int c = ks * 32 + (int)fg * 8;
    const u32x4 e = sh_dw8<DT>(xs + (size_t)tapi * XS + c * 2, T::HW * XS, XS, p.b1_wd + c, KP, p.b1_s1 + c, p.b1_b1 + c);
    const u16* wb = p.b1_w2 + (size_t)ks * 512 + lane * 8;
#pragma unroll
    for (int a = 0; a < kShDnAcc; ++a) {
      const int af = (int)wave + 4 * a;
      if (af < nco) {  // (uniform)
        const u32x4 rw = *reinterpret_cast<const u32x4*>(wb + (size_t)af * KS * 512);
        acc1[a] = mfma16<DT>(rw, e, acc1[a]);
      }
    }
  }
  uint2 left[kShDnAcc];
#pragma unroll
  for (int a = 0; a < kShDnAcc; ++a) {
    const int af = (int)wave + 4 * a;
    left[a] = make_uint2(0u, 0u);
    if (af < nco) {
      const int co = af * 16 + (int)fg * 4;
      const f32x4 s = *reinterpret_cast<const f32x4*>(p.b1_s2 + co), b = *reinterpret_cast<const f32x4*>(p.b1_b2 + co);
      float v[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] = __builtin_fmaxf(acc1[a][r] * s[r] + b[r], 0.f);
      left[a] = make_uint2(pack2_16<DT>(v[0], v[1]), pack2_16<DT>(v[2], v[3]));
    }
  }

  // ---- branch 2, middle channels in chunks of 64 ----------------------------------------------------------------------------------
  for (int chunk = 0; chunk < nchunks; ++chunk) {
    {  // phase 1: this wave's 16 middle channels of the chunk on every halo fragment, x from the staged tile
      f32x4 a1[T::NF];
#pragma unroll
      for (int f = 0; f < T::NF; ++f) a1[f] = f32x4{0.f, 0.f, 0.f, 0.f};
      const int cmf = chunk * 4 + (int)wave;
      const u16* wa = p.w1 + (size_t)cmf * KS * 512 + lane * 8;
      const unsigned char* xb = xs + (size_t)fr * XS + fg * 16u;
      for (int ks = 0; ks < KS; ++ks) {
        const u32x4 rw = *reinterpret_cast<const u32x4*>(wa + (size_t)ks * 512);
#pragma unroll
        for (int f = 0; f < T::NF; ++f) {
          const u32x4 b = *reinterpret_cast<const u32x4*>(xb + (size_t)(f * 16) * XS + ks * 64);
          a1[f] = mfma16<DT>(rw, b, a1[f]);  // D[cm = 4fg + r][px = fr]
        }
      }
      const int cl = (int)wave * 16 + (int)fg * 4, cm = chunk * kShCH + cl;
      const f32x4 sc = *reinterpret_cast<const f32x4*>(p.s1 + cm), bi = *reinterpret_cast<const f32x4*>(p.b1 + cm);
#pragma unroll
      for (int f = 0; f < T::NF; ++f) {
        const int hp = f * 16 + (int)fr;
        const int hy = hp / T::HW, hx = hp - hy * T::HW;
        const bool in = hp < T::HP && (unsigned)(iy0 + hy) < (unsigned)H && (unsigned)(ix0 + hx) < (unsigned)W;
        float v[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = in ? __builtin_fmaxf(a1[f][r] * sc[r] + bi[r], 0.f) : 0.f;  // ZEROS outside the image
        *reinterpret_cast<uint2*>(ms + (size_t)hp * kShMS + cl * 2) = make_uint2(pack2_16<DT>(v[0], v[1]), pack2_16<DT>(v[2], v[3]));
      }
    }
    __syncthreads();  // the middle chunk is complete
#pragma unroll
    for (int ks2 = 0; ks2 < 2; ++ks2) {
      const int c = chunk * kShCH + ks2 * 32 + (int)fg * 8;
      const u32x4 d = sh_dw8<DT>(ms + (size_t)tapi * kShMS + ks2 * 64 + fg * 16u, T::HW * kShMS, kShMS, p.wd + c, P, p.s2 + c, p.b2 + c);
      const u16* wb = p.w3 + (size_t)(chunk * 2 + ks2) * 512 + lane * 8;
#pragma unroll
      for (int a = 0; a < kShDnAcc; ++a) {
        const int af = (int)wave + 4 * a;
        if (af < nco) {  // (uniform)
          const u32x4 rw = *reinterpret_cast<const u32x4*>(wb + (size_t)af * KPP * 512);
          acc2[a] = mfma16<DT>(rw, d, acc2[a]);
        }
      }
    }
    __syncthreads();  // every wave has read the chunk: the next one may overwrite it
  }

  const int oy = ty0 + ty, ox = tx0 + tx;
  if (pvalid && oy < p.Ho && ox < p.Wo) {
    u16* ypix = p.y + (((size_t)n * p.Ho + oy) * p.Wo + ox) * Cp;
#pragma unroll
    for (int a = 0; a < kShDnAcc; ++a) {
      const int af = (int)wave + 4 * a, co = af * 16 + (int)fg * 4;
      if (af < nco && 2 * co < Cp) sh_store4<DT>(ypix, co, Cb, acc2[a], p.s3, p.b3, left[a]);
    }
  }
}

static bool sh_ranges_overlap(uintptr_t a, size_t na, uintptr_t b, size_t nb) { return a < b + nb && b < a + na; }
static bool sh_dtype_ok(int dtype) { return dtype == SSDK_BF16 || dtype == SSDK_F16; }

}  // namespace ssdk

using namespace ssdk;

extern "C" size_t ssdk_shuffle_unit_desc_bytes(void) { return sizeof(ssdk_shuffle_unit_desc); }
extern "C" size_t ssdk_shuffle_down_desc_bytes(void) { return sizeof(ssdk_shuffle_down_desc); }

extern "C" int ssdk_shuffle_unit_supported(int Cb, int H, int W, int dtype) {
  return Cb % 2 == 0 && Cb >= 8 && Cb <= 512 && H >= 1 && W >= 1 && H <= 32768 && W <= 32768 && sh_dtype_ok(dtype);
}

extern "C" int ssdk_shuffle_down_supported(int Cin, int Cb, int H, int W, int dtype) {
  return Cin % 2 == 0 && Cin >= 8 && Cin <= 1024 && Cb % 2 == 0 && Cb >= 8 && Cb <= 512 && H >= 1 && W >= 1 && H <= 32768 &&
         W <= 32768 && sh_dtype_ok(dtype);
}

extern "C" int ssdk_shuffle_unit(const ssdk_shuffle_unit_desc* d, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!d) {
    set_error("shuffle_unit: null descriptor");
    return SSDK_E_BADARG;
  }
  if (!ssdk_shuffle_unit_supported(d->Cb, d->H, d->W, d->dtype)) {
    set_error("shuffle_unit: unsupported unit Cb=%d H=%d W=%d dtype=%d (Cb even, 8 <= Cb <= 512, 1 <= H, W <= 32768, bf16 | f16)", d->Cb,
              d->H, d->W, d->dtype);
    return SSDK_E_BADARG;
  }
  const int tiles_y = (d->H + kShTH - 1) / kShTH, tiles_x = (d->W + kShTW - 1) / kShTW;
  const long long blocks = (long long)d->N * tiles_y * tiles_x;
  if (d->N < 1 || blocks > 0x7fffffffLL) {
    set_error("shuffle_unit: N=%d with %d x %d tiles (N >= 1, fewer than 2^31 workgroups)", d->N, tiles_y, tiles_x);
    return SSDK_E_BADARG;
  }
  if (!d->x || !d->y || !d->w1 || !d->scale1 || !d->bias1 || !d->wd || !d->scale2 || !d->bias2 || !d->w3 || !d->scale3 || !d->bias3) {
    set_error("shuffle_unit: null pointer (x, y, the three weights and their scale / bias vectors are required)");
    return SSDK_E_BADARG;
  }
  if (((uintptr_t)d->x | (uintptr_t)d->y | (uintptr_t)d->w1 | (uintptr_t)d->scale1 | (uintptr_t)d->bias1 | (uintptr_t)d->wd |
       (uintptr_t)d->scale2 | (uintptr_t)d->bias2 | (uintptr_t)d->w3 | (uintptr_t)d->scale3 | (uintptr_t)d->bias3) & 15) {
    set_error("shuffle_unit: every pointer must be 16-byte aligned");
    return SSDK_E_BADARG;
  }
  const int Cp = (2 * d->Cb + 7) / 8 * 8, P = (d->Cb + kShCH - 1) / kShCH * kShCH;
  const size_t bytes = (size_t)d->N * d->H * d->W * Cp * 2;
  if (sh_ranges_overlap((uintptr_t)d->x, bytes, (uintptr_t)d->y, bytes)) {
    set_error("shuffle_unit: y overlaps x (other workgroups read x's halo while this one writes y)");
    return SSDK_E_BADARG;
  }
  ShUnitParams p;
  p.x = (const u16*)d->x, p.y = (u16*)d->y;
  p.w1 = (const u16*)d->w1, p.s1 = d->scale1, p.b1 = d->bias1;
  p.wd = (const u16*)d->wd, p.s2 = d->scale2, p.b2 = d->bias2;
  p.w3 = (const u16*)d->w3, p.s3 = d->scale3, p.b3 = d->bias3;
  p.H = d->H, p.W = d->W, p.tiles_y = tiles_y, p.tiles_x = tiles_x, p.Cb = d->Cb, p.Cp = Cp, p.P = P;
  const int nco = P / 16;
#define SSDK_SH(DT, NCO_) hipLaunchKernelGGL((shuffle_unit_kernel<DT, NCO_>), dim3((unsigned)blocks), dim3(kShThreads), kShLds, stream, p)
#define SSDK_SHN(DT)            \
  do {                          \
    if (nco <= 4) SSDK_SH(DT, 4);        \
    else if (nco <= 8) SSDK_SH(DT, 8);   \
    else if (nco <= 16) SSDK_SH(DT, 16); \
    else SSDK_SH(DT, 32);                \
  } while (0)
  if (d->dtype == SSDK_BF16) SSDK_SHN(SSDK_BF16);
  else SSDK_SHN(SSDK_F16);
#undef SSDK_SHN
#undef SSDK_SH
  return check_launch("shuffle_unit_kernel");
}

extern "C" int ssdk_shuffle_down(const ssdk_shuffle_down_desc* d, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!d) {
    set_error("shuffle_down: null descriptor");
    return SSDK_E_BADARG;
  }
  if (!ssdk_shuffle_down_supported(d->Cin, d->Cb, d->H, d->W, d->dtype)) {
    set_error("shuffle_down: unsupported unit Cin=%d Cb=%d H=%d W=%d dtype=%d (Cin even, 8 <= Cin <= 1024, Cb even, 8 <= Cb <= 512, "
              "1 <= H, W <= 32768, bf16 | f16)", d->Cin, d->Cb, d->H, d->W, d->dtype);
    return SSDK_E_BADARG;
  }
  const int ld = d->ld_in ? d->ld_in : (d->Cin + 7) / 8 * 8;
  if (ld % 8 || ld < d->Cin) {
    set_error("shuffle_down: ld_in=%d with Cin=%d (0, or a multiple of 8 that is >= Cin)", d->ld_in, d->Cin);
    return SSDK_E_BADARG;
  }
  const bool small = d->Cin > 512;  // half the tile: the staged input stays below 112 KiB
  const int TH = small ? SSDK_SHUFFLE_DOWN_TILE_H / 2 : SSDK_SHUFFLE_DOWN_TILE_H, TW = SSDK_SHUFFLE_DOWN_TILE_W;
  const int Ho = (d->H - 1) / 2 + 1, Wo = (d->W - 1) / 2 + 1;
  const int tiles_y = (Ho + TH - 1) / TH, tiles_x = (Wo + TW - 1) / TW;
  const long long blocks = (long long)d->N * tiles_y * tiles_x;
  if (d->N < 1 || blocks > 0x7fffffffLL) {
    set_error("shuffle_down: N=%d with %d x %d tiles (N >= 1, fewer than 2^31 workgroups)", d->N, tiles_y, tiles_x);
    return SSDK_E_BADARG;
  }
  const void* ptrs[] = {d->x, d->y, d->b1_wd, d->b1_scale1, d->b1_bias1, d->b1_w2, d->b1_scale2, d->b1_bias2, d->w1, d->scale1,
                        d->bias1, d->wd, d->scale2, d->bias2, d->w3, d->scale3, d->bias3};
  uintptr_t bits = 0;
  for (const void* q : ptrs) {
    if (!q) {
      set_error("shuffle_down: null pointer (x, y, the five weights and their scale / bias vectors are required)");
      return SSDK_E_BADARG;
    }
    bits |= (uintptr_t)q;
  }
  if (bits & 15) {
    set_error("shuffle_down: every pointer must be 16-byte aligned");
    return SSDK_E_BADARG;
  }
  const int Cp = (2 * d->Cb + 7) / 8 * 8, P = (d->Cb + kShCH - 1) / kShCH * kShCH, KP = (d->Cin + 31) / 32 * 32;
  if (sh_ranges_overlap((uintptr_t)d->x, (size_t)d->N * d->H * d->W * ld * 2, (uintptr_t)d->y, (size_t)d->N * Ho * Wo * Cp * 2)) {
    set_error("shuffle_down: y overlaps x");
    return SSDK_E_BADARG;
  }
  ShDownParams p;
  p.x = (const u16*)d->x, p.y = (u16*)d->y;
  p.b1_wd = (const u16*)d->b1_wd, p.b1_s1 = d->b1_scale1, p.b1_b1 = d->b1_bias1;
  p.b1_w2 = (const u16*)d->b1_w2, p.b1_s2 = d->b1_scale2, p.b1_b2 = d->b1_bias2;
  p.w1 = (const u16*)d->w1, p.s1 = d->scale1, p.b1 = d->bias1;
  p.wd = (const u16*)d->wd, p.s2 = d->scale2, p.b2 = d->bias2;
  p.w3 = (const u16*)d->w3, p.s3 = d->scale3, p.b3 = d->bias3;
  p.H = d->H, p.W = d->W, p.Ho = Ho, p.Wo = Wo, p.tiles_y = tiles_y, p.tiles_x = tiles_x;
  p.Cin = d->Cin, p.ld = ld, p.KP = KP, p.Cb = d->Cb, p.Cp = Cp, p.P = P;
  const size_t lds = sh_down_lds(small ? ShDownTile<2, 4>::ROWS : ShDownTile<4, 4>::ROWS, KP);
#define SSDK_SD(DT, TH_)                                                                                                         \
  do {                                                                                                                           \
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&shuffle_down_kernel<DT, TH_, 4>),                                  \
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);                                             \
    hipLaunchKernelGGL((shuffle_down_kernel<DT, TH_, 4>), dim3((unsigned)blocks), dim3(kShThreads), lds, stream, p);            \
  } while (0)
  if (d->dtype == SSDK_BF16) {
    if (small) SSDK_SD(SSDK_BF16, 2);
    else SSDK_SD(SSDK_BF16, 4);
  } else {
    if (small) SSDK_SD(SSDK_F16, 2);
    else SSDK_SD(SSDK_F16, 4);
  }
#undef SSDK_SD
  return check_launch("shuffle_down_kernel");
}
