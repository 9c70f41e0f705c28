// ssdk_conv3train.hip -- the DENSE 3x3 convolution of the TRAINING step on gfx950: forward (+ bias), input gradient, weight gradient.
//
// Reference: the towers, smoothing and head convolutions of SSDFPN / SSDBiFPN (ssds/modeling/ssds/fpn.py, bifpn.py), the 3x3 of the
// ResNet bottlenecks (nets/resnet.py) and the extras, inside the DDP step.  pad 1, stride 1 | 2, Cin a multiple of 16 (16 .. 4096),
// Cout a multiple of 4 (4 .. 4096), independent of each other.  Tensors are bf16 | fp16, NCHW contiguous in and out (the layout of the
// 1x1, grouped 3x3 and BatchNorm kernels around the layer), fp32 accumulation on mfma16<DT>.  No BatchNorm fold, no activation.
// The one-group case ssdk_gconvtrain.hip cannot reach (gw <= 256, Cin == Cout there).
//
//   prepare   conv3_train_prepare_kernel: the fp32 master weight [Cout, Cin, 3, 3] -> two 16-bit dense images (include/ssdk.h, "dense
//             3x3 image"): the forward image and the input-gradient image (transposed, taps flipped).  Replaces autocast's cast.
//   forward / input gradient   conv3_train_conv_kernel<DT, S, T>: an implicit GEMM.  A workgroup (4 waves) owns a patch of 2 FT
//             fragments of 16 output pixels (a fragment is 16 / TW rows x TW columns, TW = 16 | 8 | 4 by the map's width, so that
//             narrow maps put several rows into one fragment) x 64 output channels, and loops over the input channels in chunks of 32.
//             The halo of a chunk lives in LDS as four planes [8-channel group][pixel][8 channels] (a lane's A operand is one
//             ds_read_b128; the plane pitch is a multiple of 256 B, + 16 B at stride 2, which keeps the four lane groups of the read
//             on different banks), double-buffered: the next chunk's global loads are in flight while the matrix cores work on this
//             one, one barrier per chunk.  The accumulators persist over the whole K = 9 Cin.  Operand roles as
//             gconv_train_conv_kernel: A = pixels, B = weights streamed from the image, so a lane's four accumulator values are four
//             consecutive pixels of ONE channel, an 8-byte store along W.  The bias is added in fp32 before the single rounding.
//             A wave is (FT fragments) x (2 blocks of 16 channels); FT = 4 at stride 1, 2 at stride 2.  (Four blocks per wave, a
//             128-channel tile, compile to 84 + 96 registers, 2 waves per SIMD, and halve the LDS reads per MFMA: to be tried
//             once the kernel can be timed.)
//             The last chunk of a Cin that is no multiple of 32 (912), and the channels that pad Cout to 16 in the input-gradient
//             image (36, 720), are zeros in LDS and masked weight loads.
//             T (input gradient at stride 2) is a real transposed convolution by input-pixel parity: an input pixel (2a + py, 2b + px)
//             sees the (1 + py)(1 + px) taps whose output pixel exists, 9 taps per 2 x 2 pixels, no zero-dilated dy.  A wave keeps the
//             four parity classes of its fragments and interleaves the two column parities into one 16-byte store.
//             Stride-1 input gradient = the forward kernel on the input-gradient image with Cin and Cout swapped.
//             The halo is staged with 2-byte loads (64 lanes on 64 consecutive pixels of a channel row), eight channels packed in
//             registers into one ds_write_b128; the 16-byte row loads + register transpose of ssdk_pwtrain.hip are not used yet.
//   weight gradient   conv3_train_wgrad_kernel<DT, S, CKL>: dW[co][ci][tap] = sum over pixels dy[co][p] x[ci][p + tap] contracts over
//             pixels, contiguous along W in both operands.  A workgroup owns a 64 x 64 (co, ci) tile, all nine taps, and a range of
//             output rows; a wave a 32 x 32 quarter (36 accumulators).  A k-step is 32 pixels (4 >> CKL rows x (1 << CKL) groups of
//             eight): the dy rows and the three x rows behind them are copied into LDS as they lie in memory (no transpose), shared
//             by the four waves; the three kx shifts come from one row window (v_alignbit at stride 1, v_perm even / odd pick at
//             stride 2).  The next step's global loads are issued before the MFMAs of this one.  The fp32 partial tiles go to
//             caller-owned workspace [split][tile][9][64][64]; conv3_train_wgrad_reduce_kernel adds them in split order: no float
//             atomics, bit-reproducible.
//
// Compiler figures for gfx950 (-Rpass-analysis=kernel-resource-usage; bf16 / fp16 within 3 VGPRs; no scratch in any instance; the LDS
// of the conv kernel is dynamic, 2 buffers x 4 planes; VGPRs + AGPRs, LDS per workgroup, waves per SIMD):
//   conv, forward / stride-1 input gradient  <S = 1>  70 + 48, 24.0 KiB (26.0 at TW = 4), 4
//   conv, forward stride 2                   <S = 2>  80 + 24, 38.1 KiB, 4
//   conv, stride-2 input gradient            <T>      84 + 68, 12.0 KiB, 3
//   wgrad stride 1, CKL = 2 / 1 / 0: 130 / 141 / 162 + 144, 18.8 / 20.3 / 23.3 KiB, 1 wave per SIMD
//   wgrad stride 2, CKL = 2 / 1 / 0: 207 / 234 / 237 + 144, 30.8 / 32.3 / 35.3 KiB, 1 wave per SIMD
//   prepare 12, reduce 12 VGPRs, no LDS, 8
#include "ssdk_conv_common.h"

namespace ssdk {

static inline int c3_up(int v, int m) { return (v + m - 1) / m * m; }

static bool c3_shape_ok(int Cin, int Cout) {
  return Cin >= 16 && Cin <= 4096 && (Cin % 16) == 0 && Cout >= 4 && Cout <= 4096 && (Cout % 4) == 0;
}

// ---- prepare ------------------------------------------------------------------------------------------------------------------------
struct C3PrepParams {
  const float* w;  // [Cout][Cin][3][3]
  u16* img[2];     // forward | input-gradient image, either may be NULL
  int Ci, Co;
  int KS[2], Cp[2];  // k-steps and channel pitch of each image
  u32 total[2];      // elements of each image
};

template <int DT>
__global__ __launch_bounds__(256) void conv3_train_prepare_kernel(const C3PrepParams p) {
  const u32 idx = blockIdx.x * 256u + threadIdx.x;
  const int which = (int)blockIdx.y;
  u16* out = p.img[which];
  if (!out || idx >= p.total[which]) return;
  // image element [row block][k-step][k % 32 / 8][row % 16][k % 8], k = tap * Cp + channel
  const int e8 = (int)(idx & 7u), r16 = (int)((idx >> 3) & 15u), c4 = (int)((idx >> 7) & 3u);
  const int blk = (int)(idx >> 9), KS = p.KS[which], Cp = p.Cp[which];
  const int ks = blk % KS, rb = blk / KS;
  const int row = rb * 16 + r16, k = ks * 32 + c4 * 8 + e8, tap = k / Cp, c = k - tap * Cp;
  float v = 0.f;
  if (which == 0) {  // rows: output channels, channels: input channels
    if (row < p.Co && tap < 9 && c < p.Ci) v = p.w[((size_t)row * p.Ci + c) * 9 + tap];
  } else {  // rows: input channels, channels: output channels, taps flipped
    if (row < p.Ci && tap < 9 && c < p.Co) v = p.w[((size_t)c * p.Ci + row) * 9 + (8 - tap)];
  }
  out[idx] = (u16)f32_to_bits16<DT>(v);
}

// ---- forward / input gradient ---------------------------------------------------------------------------------------------------------
struct C3ConvParams {
  const u16* x;       // [N, Ci, H, W]
  const u16* wf;      // dense image [RB][KS][4][16][8]
  const float* bias;  // [Co] or NULL
  u16* y;             // [N, Co, Ho, Wo]
  int N, Ci, Cp, Co, H, W, Ho, Wo;
  int Pa, Pb;  // the grid the patches tile: the output map, or (T) the half-resolution grid of one parity class
  int RB, KS, nchunks, cblocks, tiles_x, tiles_y, tw_log2, IH, IW, iw_inv, npx, plane;
};

template <int S, bool T> struct C3Cfg {
  static constexpr int FT = (!T && S == 1) ? 4 : 2;       // fragments per wave; a patch is 2 FT fragments
  static constexpr int NIT = T ? 2 : (S == 1 ? 4 : 5);    // staged (pixel, 8-channel group) items per thread and chunk
  static constexpr int NPAR = T ? 4 : 1;
};

template <int DT, int S, bool T>
__global__ __launch_bounds__(256) void conv3_train_conv_kernel(const C3ConvParams p) {
  constexpr int RBT = 2;  // blocks of 16 output channels per wave
  extern __shared__ __attribute__((aligned(16))) unsigned char csm[];
  constexpr int FT = C3Cfg<S, T>::FT, NIT = C3Cfg<S, T>::NIT, NPAR = C3Cfg<S, T>::NPAR;
  const u32 tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const u32 fr = lane & 15u, fg = lane >> 4;
  const int wp = (int)(wave & 1u), wc = (int)(wave >> 1);
  u32 b = blockIdx.x;
  const u32 cb = b % (u32)p.cblocks;
  b /= (u32)p.cblocks;
  const u32 tx = b % (u32)p.tiles_x;
  b /= (u32)p.tiles_x;
  const u32 ty = b % (u32)p.tiles_y;
  const u32 n = b / (u32)p.tiles_y;
  const int IW = p.IW, npx = p.npx, plane = p.plane;
  const int TW = 1 << p.tw_log2, RPF = 16 >> p.tw_log2;  // fragment: RPF rows x TW columns of the patch grid
  const int a0 = (int)ty * (2 * FT) * RPF, b0 = (int)tx * TW;
  const int iy0 = T ? a0 : a0 * S - 1, ix0 = T ? b0 : b0 * S - 1;
  const size_t plane_in = (size_t)p.H * p.W;
  const u32 bufsz = 4u * (u32)plane;

  // ---- staging items of this thread: halo pixel q of 8-channel group c8 (the same for every chunk)
  int goff[NIT];   // pixel offset inside a channel plane, -1: outside the image (zeros) or no item
  u32 soff[NIT];   // byte offset inside a buffer, ~0u: no item
#pragma unroll
  for (int j = 0; j < NIT; ++j) {
    const int i = (int)tid + 256 * j;
    const int c8 = (i >= npx) + (i >= 2 * npx) + (i >= 3 * npx);
    const int q = i - c8 * npx;
    const bool item = i < 4 * npx;
    const int row = (q * p.iw_inv) >> 16, col = q - row * IW;
    const int iy = iy0 + row, ix = ix0 + col;
    const bool ok = item && (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W;
    goff[j] = ok ? iy * p.W + ix : -1;
    soff[j] = item ? (u32)(c8 * plane + q * 16) : ~0u;
  }
  const u16* xin = p.x + (size_t)n * p.Ci * plane_in;
  u32x4 stg[NIT];
  auto stage_load = [&](int chunk) {
#pragma unroll
    for (int j = 0; j < NIT; ++j) {
      u32 d[4] = {0u, 0u, 0u, 0u};
      if (goff[j] >= 0) {
        const int i = (int)tid + 256 * j;
        const int c8 = (i >= npx) + (i >= 2 * npx) + (i >= 3 * npx);
        const int ch0 = chunk * 32 + c8 * 8;
        const u16* src = xin + (size_t)ch0 * plane_in + goff[j];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          u32 v = 0u;
          if (ch0 + e < p.Ci) v = src[(size_t)e * plane_in];
          d[e >> 1] |= v << (16 * (e & 1));
        }
      }
      stg[j] = u32x4{d[0], d[1], d[2], d[3]};
    }
  };
  auto stage_store = [&](int buf) {
#pragma unroll
    for (int j = 0; j < NIT; ++j)
      if (soff[j] != ~0u) *reinterpret_cast<u32x4*>(csm + (u32)buf * bufsz + soff[j]) = stg[j];
  };

  // A operand: this lane's pixel fr of a fragment, 8-channel group fg of the chunk
  const int oyf = (int)(fr >> p.tw_log2), oxf = (int)(fr & (u32)(TW - 1));
  const int SH = T ? 1 : S;
  const u32 xlane = fg * (u32)plane + (u32)((oyf * SH * IW + oxf * SH + wp * FT * RPF * SH * IW) * 16);
  const u32 fstr = (u32)(RPF * SH * IW * 16);
  // B operand: the wave's two blocks of 16 output channels
  const int rb0 = ((int)cb * 2 + wc) * RBT;
  const int cp8 = p.Cp >> 3;
  const u16* wlane = p.wf + (size_t)rb0 * p.KS * 512 + fr * 8u;

  f32x4 acc[NPAR][RBT][FT];
#pragma unroll
  for (int h = 0; h < NPAR; ++h)
#pragma unroll
    for (int r = 0; r < RBT; ++r)
#pragma unroll
      for (int f = 0; f < FT; ++f) acc[h][r][f] = f32x4{0.f, 0.f, 0.f, 0.f};

  auto kstep = [&](int par, u32 xo, int itap, int chunk, u32 bufbase) {  // one tap of one chunk: 32 channels
    const bool kin = chunk * 32 + (int)fg * 8 < p.Cp;
    const int a8g = itap * cp8 + chunk * 4 + (int)fg;  // the 8-channel group's place in the image row
    const u32 wo = (u32)((a8g >> 2) * 512 + (a8g & 3) * 128);
    u32x4 w[RBT];
#pragma unroll
    for (int r = 0; r < RBT; ++r) {
      w[r] = u32x4{0u, 0u, 0u, 0u};
      if (kin && rb0 + r < p.RB) w[r] = *reinterpret_cast<const u32x4*>(wlane + (size_t)r * p.KS * 512 + wo);
    }
#pragma unroll
    for (int f = 0; f < FT; ++f) {
      const u32x4 xv = *reinterpret_cast<const u32x4*>(csm + bufbase + xlane + xo + (u32)f * fstr);
#pragma unroll
      for (int r = 0; r < RBT; ++r) acc[par][r][f] = mfma16<DT>(xv, w[r], acc[par][r][f]);  // D[pixel 4 fg + e][channel fr]
    }
  };

  stage_load(0);
  stage_store(0);
  __syncthreads();
  for (int chunk = 0; chunk < p.nchunks; ++chunk) {  // uniform
    const bool more = chunk + 1 < p.nchunks;
    if (more) stage_load(chunk + 1);
    const u32 bufbase = (u32)(chunk & 1) * bufsz;
    if constexpr (!T) {
#pragma unroll
      for (int tap = 0; tap < 9; ++tap) kstep(0, (u32)(((tap / 3) * IW + (tap % 3)) * 16), tap, chunk, bufbase);
    } else {
      // the class's taps in (row, column) order of the output pixels (a + tyk, b + txk); in the input-gradient image the tap of
      // output row a + tyk is ky' = 2 tyk (odd input rows) or 1 (even input rows), columns alike
#pragma unroll
      for (int py = 0; py < 2; ++py)
#pragma unroll
        for (int px = 0; px < 2; ++px)
#pragma unroll
          for (int tap = 0; tap < (1 + py) * (1 + px); ++tap) {
            const int tyk = px ? (tap >> 1) : tap, txk = px ? (tap & 1) : 0;
            const int itap = 3 * (py ? 2 * tyk : 1) + (px ? 2 * txk : 1);
            kstep(py * 2 + px, (u32)((tyk * IW + txk) * 16), itap, chunk, bufbase);
          }
    }
    if (more) stage_store((chunk + 1) & 1);
    __syncthreads();
  }

  // D: this lane's four pixels 4 fg .. 4 fg + 3 of a fragment (one row of it, consecutive columns)
  const int oyd = (int)((fg * 4u) >> p.tw_log2), oxd = (int)((fg * 4u) & (u32)(TW - 1));
  const size_t plane_out = (size_t)p.Ho * p.Wo;
#pragma unroll
  for (int r = 0; r < RBT; ++r) {
    const int co = (rb0 + r) * 16 + (int)fr;
    if (co >= p.Co) continue;  // row padding
    const float bi = p.bias ? p.bias[co] : 0.f;
    u16* yc = p.y + ((size_t)n * p.Co + co) * plane_out;
#pragma unroll
    for (int f = 0; f < FT; ++f) {
      const int a = a0 + (wp * FT + f) * RPF + oyd, bq = b0 + oxd;
      if constexpr (!T) {
        if (a < p.Ho && bq < p.Wo) {
          u16* dst = yc + (size_t)a * p.Wo + bq;
          f32x4 v = acc[0][r][f];
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] += bi;
          if ((p.Wo & 3) == 0 && (((uintptr_t)p.y) & 7u) == 0) {  // uniform: the four pixels exist and are 8-byte aligned
            *reinterpret_cast<uint2*>(dst) = make_uint2(pack2_16<DT>(v[0], v[1]), pack2_16<DT>(v[2], v[3]));
          } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
              if (bq + e < p.Wo) dst[e] = (u16)f32_to_bits16<DT>(v[e]);
          }
        }
      } else {
#pragma unroll
        for (int py = 0; py < 2; ++py) {
          const int iy = 2 * a + py, ix = 2 * bq;
          if (iy < p.Ho && ix < p.Wo) {
            u16* dst = yc + (size_t)iy * p.Wo + ix;
            const f32x4 v0 = acc[(py * 2) % NPAR][r][f], v1 = acc[(py * 2 + 1) % NPAR][r][f];
            if ((p.Wo & 7) == 0 && (((uintptr_t)p.y) & 15u) == 0) {  // uniform
              *reinterpret_cast<u32x4*>(dst) = u32x4{pack2_16<DT>(v0[0], v1[0]), pack2_16<DT>(v0[1], v1[1]),
                                                     pack2_16<DT>(v0[2], v1[2]), pack2_16<DT>(v0[3], v1[3])};
            } else {
#pragma unroll
              for (int e = 0; e < 4; ++e) {
                if (ix + 2 * e < p.Wo) dst[2 * e] = (u16)f32_to_bits16<DT>(v0[e]);
                if (ix + 2 * e + 1 < p.Wo) dst[2 * e + 1] = (u16)f32_to_bits16<DT>(v1[e]);
              }
            }
          }
        }
      }
    }
  }
}

template <int DT, int S, bool T>
static void c3_conv_launch(const C3ConvParams& p, long grid, size_t lds, hipStream_t stream) {
  hipLaunchKernelGGL((conv3_train_conv_kernel<DT, S, T>), dim3((unsigned)grid), dim3(256), lds, stream, p);
}

// x [N, Ci, H, W] -> y [N, Co, Ho, Wo]; transposed: x is the output gradient of a stride-2 layer, y its input gradient
static int c3_conv(const char* what, const void* x, const void* wf, const float* bias, void* y, int N, int Ci, int Co, int H, int W, int Ho,
                   int Wo, int stride, bool transposed, int dtype, hipStream_t stream) {
  C3ConvParams p;
  memset(&p, 0, sizeof(p));
  p.x = (const u16*)x;
  p.wf = (const u16*)wf;
  p.bias = bias;
  p.y = (u16*)y;
  p.N = N;
  p.Ci = Ci;
  p.Cp = c3_up(Ci, 16);
  p.Co = Co;
  p.H = H;
  p.W = W;
  p.Ho = Ho;
  p.Wo = Wo;
  p.Pa = transposed ? (Ho + 1) / 2 : Ho;
  p.Pb = transposed ? (Wo + 1) / 2 : Wo;
  p.RB = (Co + 15) / 16;
  p.KS = (9 * p.Cp + 31) / 32;
  p.nchunks = (p.Cp + 31) / 32;
  p.cblocks = (p.RB + 3) / 4;
  const int S = transposed ? 1 : stride;
  const int FT = (!transposed && S == 1) ? 4 : 2, NIT = transposed ? 2 : (S == 1 ? 4 : 5);
  p.tw_log2 = p.Pb > 8 ? 4 : (p.Pb > 4 ? 3 : 2);
  const int TW = 1 << p.tw_log2, RPF = 16 / TW, rows = 2 * FT * RPF;
  p.IW = transposed ? TW + 1 : (TW - 1) * S + 3;
  p.IH = transposed ? rows + 1 : (rows - 1) * S + 3;
  p.iw_inv = (65536 + p.IW - 1) / p.IW;
  p.npx = p.IH * p.IW;
  p.plane = c3_up(p.npx * 16, 256) + ((S == 2 && !transposed) ? 16 : 0);
  const size_t lds = (size_t)8 * p.plane;
  if (4 * p.npx > NIT * 256 || lds > 64u * 1024u) {
    set_error("%s: halo of %d pixels does not fit the staging", what, p.npx);
    return SSDK_E_BADARG;
  }
  p.tiles_y = (p.Pa + rows - 1) / rows;
  p.tiles_x = (p.Pb + TW - 1) / TW;
  const long grid = (long)N * p.tiles_y * p.tiles_x * p.cblocks;
  if (grid >= (1l << 31) || grid < 1) {
    set_error("%s: grid too large", what);
    return SSDK_E_BADARG;
  }
  if (dtype == SSDK_BF16) {
    if (transposed) c3_conv_launch<SSDK_BF16, 1, true>(p, grid, lds, stream);
    else if (S == 1) c3_conv_launch<SSDK_BF16, 1, false>(p, grid, lds, stream);
    else c3_conv_launch<SSDK_BF16, 2, false>(p, grid, lds, stream);
  } else {
    if (transposed) c3_conv_launch<SSDK_F16, 1, true>(p, grid, lds, stream);
    else if (S == 1) c3_conv_launch<SSDK_F16, 1, false>(p, grid, lds, stream);
    else c3_conv_launch<SSDK_F16, 2, false>(p, grid, lds, stream);
  }
  return SSDK_OK;
}

// ---- weight gradient ------------------------------------------------------------------------------------------------------------------
struct C3WgradParams {
  const u16* x;   // [N, Ci, H, W]
  const u16* dy;  // [N, Co, Ho, Wo]
  float* part;    // [splits][ntiles][9][64][64]
  float* dw;      // [Co][Ci][3][3]
  int N, Ci, Co, H, W, Ho, Wo;
  int tci, ntiles, splits, rows_per_split, ck_log2;
};

// d: dwords of one x row behind eight output pixels ox .. ox + 7: d[0] = columns (S ox - 2, S ox - 1), d[1] = (S ox, S ox + 1), ...
// -> the eight elements of column shift kx as four dwords (kx compile-time after unrolling)
template <int S>
__device__ __forceinline__ u32x4 c3_window_pick(const u32 (&d)[10], int kx) {
  u32x4 out;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if constexpr (S == 1) {
      out[j] = kx == 1 ? d[1 + j] : (kx == 0 ? __builtin_amdgcn_alignbit(d[j + 1], d[j], 16) : __builtin_amdgcn_alignbit(d[j + 2], d[j + 1], 16));
    } else {
      // kx = 0: high halves of (d[2j], d[2j + 1]); kx = 1: low halves of (d[2j + 1], d[2j + 2]); kx = 2: their high halves
      const u32 lo = kx == 0 ? d[2 * j] : d[1 + 2 * j], hi = kx == 0 ? d[1 + 2 * j] : d[2 + 2 * j];
      out[j] = kx == 1 ? __builtin_amdgcn_perm(hi, lo, 0x05040100u) : __builtin_amdgcn_perm(hi, lo, 0x07060302u);
    }
  }
  return out;
}

template <int DT, int S, int CKL>
__global__ __launch_bounds__(256) void conv3_train_wgrad_kernel(const C3WgradParams p) {
  constexpr int CKG = 1 << CKL, RK = 4 >> CKL;  // a k-step: RK output rows x CKG groups of 8 pixels
  constexpr int XLD = (S * 8 * CKG + 4) / 2;    // dwords of one staged x row: columns S ox0 - 2 .. S (ox0 + 8 CKG) + 1
  constexpr int NR = 3 * RK;                    // x rows per channel and step
  constexpr int XPER = NR * XLD, XCS = XPER | 1;  // dwords per channel; odd pitch
  constexpr int DYS = 20;                       // dwords per dy channel row (32 pixels + pad: 80 B keeps ds_read_b128 aligned)
  constexpr int NIX = (64 * XPER + 255) / 256, NIY = 4;
  constexpr int ND = S == 1 ? 6 : 9;
  __shared__ __attribute__((aligned(16))) u32 dyS[64 * DYS];
  __shared__ __attribute__((aligned(16))) u32 xS[64 * XCS];
  const u32 tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const int fr = (int)(lane & 15u), fg = (int)(lane >> 4);
  const int wa = (int)(wave & 1u), wb = (int)(wave >> 1);
  const int tile = (int)blockIdx.x, split = (int)blockIdx.y;
  const int co0 = (tile / p.tci) * 64, ci0 = (tile % p.tci) * 64;
  const int total_rows = p.N * p.Ho;
  const int R0 = split * p.rows_per_split, R1 = R0 + p.rows_per_split < total_rows ? R0 + p.rows_per_split : total_rows;
  const int nox = (p.Wo + 8 * CKG - 1) / (8 * CKG);
  const int nsteps = ((R1 - R0 + RK - 1) / RK) * nox;
  const size_t plane_x = (size_t)p.H * p.W, plane_y = (size_t)p.Ho * p.Wo;

  u32 sy[NIY], sx[NIX];
  auto stage_load = [&](int s) {
    const int R = R0 + (s / nox) * RK, ox0 = (s % nox) * 8 * CKG;
    int nn[RK], oyy[RK];
#pragma unroll
    for (int q = 0; q < RK; ++q) {
      const int Rr = R + q;
      nn[q] = Rr < R1 ? Rr / p.Ho : -1;
      oyy[q] = Rr - (Rr / p.Ho) * p.Ho;
    }
#pragma unroll
    for (int j = 0; j < NIY; ++j) {  // dy: 64 channels x 16 pixel pairs
      const int i = (int)tid + 256 * j;
      const int cl = i >> 4, slot = (i & 15) * 2, fgi = slot >> 3;
      const int rr = fgi >> CKL, col = ox0 + 8 * (fgi & (CKG - 1)) + (slot & 7);
      int n_ = nn[0], oy_ = oyy[0];
#pragma unroll
      for (int q = 1; q < RK; ++q)
        if (rr == q) n_ = nn[q], oy_ = oyy[q];
      u32 v = 0u;
      if (n_ >= 0 && co0 + cl < p.Co && col < p.Wo) {
        const u16* src = p.dy + ((size_t)n_ * p.Co + co0 + cl) * plane_y + (size_t)oy_ * p.Wo + col;
        v = src[0];
        if (col + 1 < p.Wo) v |= (u32)src[1] << 16;
      }
      sy[j] = v;
    }
#pragma unroll
    for (int j = 0; j < NIX; ++j) {  // x: 64 channels x NR rows x XLD column pairs
      const int i = (int)tid + 256 * j;
      const int cl = i / XPER, rem = i - cl * XPER, r = rem / XLD, d = rem - r * XLD;
      const int rr = r / 3, ky = r - 3 * rr;
      int n_ = nn[0], oy_ = oyy[0];
#pragma unroll
      for (int q = 1; q < RK; ++q)
        if (rr == q) n_ = nn[q], oy_ = oyy[q];
      const int iy = oy_ * S + ky - 1, c0 = S * ox0 - 2 + 2 * d;
      u32 v = 0u;
      if (cl < 64 && n_ >= 0 && ci0 + cl < p.Ci && (unsigned)iy < (unsigned)p.H && c0 + 1 >= 0 && c0 < p.W) {
        const u16* src = p.x + ((size_t)n_ * p.Ci + ci0 + cl) * plane_x + (size_t)iy * p.W;
        if (c0 >= 0) v = src[c0];
        if (c0 + 1 < p.W) v |= (u32)src[c0 + 1] << 16;
      }
      sx[j] = v;
    }
  };
  auto stage_store = [&]() {
#pragma unroll
    for (int j = 0; j < NIY; ++j) {
      const int i = (int)tid + 256 * j;
      dyS[(i >> 4) * DYS + (i & 15)] = sy[j];
    }
#pragma unroll
    for (int j = 0; j < NIX; ++j) {
      const int i = (int)tid + 256 * j;
      const int cl = i / XPER, rem = i - cl * XPER;
      if (cl < 64) xS[cl * XCS + rem] = sx[j];
    }
  };

  f32x4 acc[2][2][9];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int bb = 0; bb < 2; ++bb)
#pragma unroll
      for (int t = 0; t < 9; ++t) acc[a][bb][t] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int rrl = fg >> CKL, gl = fg & (CKG - 1);
  if (nsteps > 0) stage_load(0);
  for (int s = 0; s < nsteps; ++s) {  // uniform
    stage_store();
    __syncthreads();
    if (s + 1 < nsteps) stage_load(s + 1);
    u32x4 A[2];
#pragma unroll
    for (int a = 0; a < 2; ++a) A[a] = *reinterpret_cast<const u32x4*>(&dyS[(wa * 32 + a * 16 + fr) * DYS + fg * 4]);
#pragma unroll
    for (int bb = 0; bb < 2; ++bb) {
      const u32* xr = &xS[(wb * 32 + bb * 16 + fr) * XCS + rrl * 3 * XLD + gl * 4 * S];
#pragma unroll
      for (int ky = 0; ky < 3; ++ky) {
        u32 D[10];
#pragma unroll
        for (int k = 0; k < 10; ++k) D[k] = k < ND ? xr[ky * XLD + k] : 0u;
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
          const u32x4 B = c3_window_pick<S>(D, kx);
#pragma unroll
          for (int a = 0; a < 2; ++a) acc[a][bb][ky * 3 + kx] = mfma16<DT>(A[a], B, acc[a][bb][ky * 3 + kx]);
        }
      }
    }
    __syncthreads();
  }
  // D[m = 4 fg + j][n = fr] of tap t = dW[co0 + 32 wa + 16 a + m][ci0 + 32 wb + 16 b + n][t]
  float* out = p.part + ((size_t)split * p.ntiles + tile) * (9 * 4096);
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int bb = 0; bb < 2; ++bb)
#pragma unroll
      for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int j = 0; j < 4; ++j) out[t * 4096 + (wa * 32 + a * 16 + fg * 4 + j) * 64 + wb * 32 + bb * 16 + fr] = acc[a][bb][t][j];
}

// dw = the partial tiles added in split order; one thread per tile element
__global__ __launch_bounds__(256) void conv3_train_wgrad_reduce_kernel(const C3WgradParams p) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t per = (size_t)p.ntiles * (9 * 4096);
  if (i >= per) return;
  float s = 0.f;
  for (int q = 0; q < p.splits; ++q) s += p.part[(size_t)q * per + i];
  const int tile = (int)(i / (9 * 4096)), r = (int)(i % (9 * 4096));
  const int t = r >> 12, m = (r >> 6) & 63, nn = r & 63;
  const int co = (tile / p.tci) * 64 + m, ci = (tile % p.tci) * 64 + nn;
  if (co >= p.Co || ci >= p.Ci) return;
  p.dw[((size_t)co * p.Ci + ci) * 9 + t] = s;
}

static void c3_wgrad_plan(int N, int Ci, int Co, int Ho, int Wo, C3WgradParams* p) {
  p->tci = (Ci + 63) / 64;
  p->ntiles = ((Co + 63) / 64) * p->tci;
  p->ck_log2 = Wo > 16 ? 2 : (Wo > 8 ? 1 : 0);
  const int RK = 4 >> p->ck_log2;
  const long rows = (long)N * Ho;
  long target = 512 / p->ntiles;  // ~512 workgroups, two per CU
  if (target > 256) target = 256;
  if (target < 1) target = 1;
  long rps = (rows + target - 1) / target;
  rps = (rps + RK - 1) / RK * RK;
  p->rows_per_split = (int)rps;
  p->splits = (int)((rows + rps - 1) / rps);
}

static int c3_check(const char* what, int N, int Cin, int Cout, int H, int W, int stride, int dtype) {
  if (N < 1 || H < 1 || W < 1 || (stride != 1 && stride != 2) || (dtype != SSDK_BF16 && dtype != SSDK_F16) || !c3_shape_ok(Cin, Cout)) {
    set_error("%s: built for dense 3x3, pad 1, stride 1|2, Cin a multiple of 16 in 16..4096, Cout a multiple of 4 in 4..4096, bf16|f16 "
              "NCHW tensors (N=%d Cin=%d Cout=%d H=%d W=%d stride=%d dtype=%d)", what, N, Cin, Cout, H, W, stride, dtype);
    return SSDK_E_BADARG;
  }
  const size_t cmax = Cin > Cout ? Cin : Cout;
  if ((size_t)H * W >= (1ull << 30) || (size_t)N * cmax * H * W >= (1ull << 40) || (size_t)N * H >= (1ull << 30)) {
    set_error("%s: tensor too large", what);
    return SSDK_E_BADARG;
  }
  return SSDK_OK;
}

}  // namespace ssdk

using namespace ssdk;

extern "C" int ssdk_conv3x3_train_prepare(const float* w32, void* w_fwd, void* w_dgrad, int Cin, int Cout, int dtype, void* stream) {
  if (int rc = c3_check("conv3x3_train_prepare", 1, Cin, Cout, 1, 1, 1, dtype)) return rc;
  if (!w32 || (!w_fwd && !w_dgrad) || (((uintptr_t)w_fwd | (uintptr_t)w_dgrad) & 15u) || ((uintptr_t)w32 & 3u)) {
    set_error("conv3x3_train_prepare: null weights, no image asked for, or an image that is not 16-byte aligned");
    return SSDK_E_BADARG;
  }
  C3PrepParams p;
  p.w = w32;
  p.img[0] = (u16*)w_fwd;
  p.img[1] = (u16*)w_dgrad;
  p.Ci = Cin;
  p.Co = Cout;
  p.Cp[0] = Cin;
  p.Cp[1] = c3_up(Cout, 16);
  p.KS[0] = (9 * p.Cp[0] + 31) / 32;
  p.KS[1] = (9 * p.Cp[1] + 31) / 32;
  const size_t t0 = (size_t)((Cout + 15) / 16) * p.KS[0] * 512, t1 = (size_t)(Cin / 16) * p.KS[1] * 512;
  p.total[0] = (u32)t0;
  p.total[1] = (u32)t1;
  const size_t total = t0 > t1 ? t0 : t1;
  const dim3 grid((unsigned)((total + 255) / 256), 2);
  if (dtype == SSDK_BF16) hipLaunchKernelGGL((conv3_train_prepare_kernel<SSDK_BF16>), grid, dim3(256), 0, (hipStream_t)stream, p);
  else hipLaunchKernelGGL((conv3_train_prepare_kernel<SSDK_F16>), grid, dim3(256), 0, (hipStream_t)stream, p);
  return check_launch("conv3_train_prepare_kernel");
}

extern "C" int ssdk_conv3x3_train_forward(const void* x, const void* w_fwd, const float* bias, void* y, int N, int Cin, int Cout, int H, int W,
                                          int stride, int dtype, void* stream) {
  if (int rc = c3_check("conv3x3_train_forward", N, Cin, Cout, H, W, stride, dtype)) return rc;
  if (!x || !w_fwd || !y || ((uintptr_t)w_fwd & 15u) || (((uintptr_t)x | (uintptr_t)y) & 1u) || ((uintptr_t)bias & 3u)) {
    set_error("conv3x3_train_forward: null pointer, an image that is not 16-byte aligned, or a misaligned tensor / bias");
    return SSDK_E_BADARG;
  }
  const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
  if (int rc = c3_conv("conv3x3_train_forward", x, w_fwd, bias, y, N, Cin, Cout, H, W, Ho, Wo, stride, false, dtype, (hipStream_t)stream))
    return rc;
  return check_launch("conv3_train_fwd_kernel");
}

extern "C" int ssdk_conv3x3_train_dgrad(const void* dy, const void* w_dgrad, void* dx, int N, int Cin, int Cout, int H, int W, int stride,
                                        int dtype, void* stream) {
  if (int rc = c3_check("conv3x3_train_dgrad", N, Cin, Cout, H, W, stride, dtype)) return rc;
  if (!dy || !w_dgrad || !dx || ((uintptr_t)w_dgrad & 15u) || (((uintptr_t)dy | (uintptr_t)dx) & 1u)) {
    set_error("conv3x3_train_dgrad: null pointer, an image that is not 16-byte aligned, or a misaligned tensor");
    return SSDK_E_BADARG;
  }
  const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
  hipStream_t st = (hipStream_t)stream;
  int rc;
  if (stride == 1) rc = c3_conv("conv3x3_train_dgrad", dy, w_dgrad, nullptr, dx, N, Cout, Cin, H, W, H, W, 1, false, dtype, st);
  else rc = c3_conv("conv3x3_train_dgrad", dy, w_dgrad, nullptr, dx, N, Cout, Cin, Ho, Wo, H, W, 2, true, dtype, st);
  if (rc) return rc;
  return check_launch(stride == 1 ? "conv3_train_dgrad_kernel" : "conv3_train_dgrad_s2_kernel");
}

extern "C" size_t ssdk_conv3x3_train_wgrad_workspace_bytes(int N, int Cin, int Cout, int H, int W, int stride) {
  if (N < 1 || H < 1 || W < 1 || (stride != 1 && stride != 2) || !c3_shape_ok(Cin, Cout)) return 0;
  C3WgradParams p;
  c3_wgrad_plan(N, Cin, Cout, (H - 1) / stride + 1, (W - 1) / stride + 1, &p);
  return (size_t)p.splits * p.ntiles * (9 * 4096) * sizeof(float);
}

extern "C" int ssdk_conv3x3_train_wgrad(const void* x, const void* dy, float* dw, void* workspace, size_t workspace_bytes, int N, int Cin,
                                        int Cout, int H, int W, int stride, int dtype, void* stream) {
  if (int rc = c3_check("conv3x3_train_wgrad", N, Cin, Cout, H, W, stride, dtype)) return rc;
  const size_t need = ssdk_conv3x3_train_wgrad_workspace_bytes(N, Cin, Cout, H, W, stride);
  if (!x || !dy || !dw || !workspace || ((uintptr_t)workspace & 15u) || (((uintptr_t)x | (uintptr_t)dy) & 1u) || ((uintptr_t)dw & 3u) ||
      workspace_bytes < need) {
    set_error("conv3x3_train_wgrad: null pointer, or workspace too small / misaligned (%zu bytes given, %zu needed)", workspace_bytes, need);
    return SSDK_E_BADARG;
  }
  C3WgradParams p;
  memset(&p, 0, sizeof(p));
  p.x = (const u16*)x;
  p.dy = (const u16*)dy;
  p.dw = dw;
  p.part = (float*)workspace;
  p.N = N;
  p.Ci = Cin;
  p.Co = Cout;
  p.H = H;
  p.W = W;
  p.Ho = (H - 1) / stride + 1;
  p.Wo = (W - 1) / stride + 1;
  c3_wgrad_plan(N, Cin, Cout, p.Ho, p.Wo, &p);
  if (p.splits > 65535) {
    set_error("conv3x3_train_wgrad: too many pixel ranges (%d)", p.splits);
    return SSDK_E_BADARG;
  }
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)p.ntiles, (unsigned)p.splits);
#define SSDK_C3_W(DT, S)                                                                                    \
  do {                                                                                                      \
    if (p.ck_log2 == 2) hipLaunchKernelGGL((conv3_train_wgrad_kernel<DT, S, 2>), grid, dim3(256), 0, st, p); \
    else if (p.ck_log2 == 1) hipLaunchKernelGGL((conv3_train_wgrad_kernel<DT, S, 1>), grid, dim3(256), 0, st, p); \
    else hipLaunchKernelGGL((conv3_train_wgrad_kernel<DT, S, 0>), grid, dim3(256), 0, st, p);               \
  } while (0)
  if (dtype == SSDK_BF16) {
    if (stride == 1) SSDK_C3_W(SSDK_BF16, 1);
    else SSDK_C3_W(SSDK_BF16, 2);
  } else {
    if (stride == 1) SSDK_C3_W(SSDK_F16, 1);
    else SSDK_C3_W(SSDK_F16, 2);
  }
#undef SSDK_C3_W
  const size_t per = (size_t)p.ntiles * (9 * 4096);
  hipLaunchKernelGGL(conv3_train_wgrad_reduce_kernel, dim3((unsigned)((per + 255) / 256)), dim3(256), 0, st, p);
  return check_launch("conv3_train_wgrad_kernel");
}
