// ssdk_conv3train_kernels.h -- device templates and launch plans of the dense 3x3 training kernels, shared by ssdk_conv3train.hip
// (convolution) and ssdk_convttrain.hip (its adjoint, the transposed 3x3 / stride 2 of the Shelf decoder).  The kernel designs are
// described at the top of ssdk_conv3train.hip.
#pragma once
#include "ssdk_conv_common.h"

namespace ssdk {

static inline int c3_up(int v, int m) { return (v + m - 1) / m * m; }

static inline bool c3_shape_ok(int Cin, int Cout) {
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

// ---- forward / input gradient ---------------------------------------------------------------------------------------------------------
struct C3ConvParams {
  const u16* x;       // [N, Ci, H, W]
  const u16* wf;      // dense image [RB][KS][4][16][8]
  const float* bias;  // [Co] or NULL
  u16* y;             // [N, Co, Ho, Wo]
  int N, Ci, Cp, Co, H, W, Ho, Wo;
  int Pa, Pb;  // the grid the patches tile: the output map, or (T) the half-resolution grid of one parity class
  int RB, KS, nchunks, cblocks, tiles_x, tiles_y, tw_log2, IH, IW, iw_inv, npx, plane;
  const u16* skip;  // EPI only: [N, Co, Ho, Wo] added to the output in fp32 before the single rounding, or NULL
};

template <int S, bool T> struct C3Cfg {
  static constexpr int FT = (!T && S == 1) ? 4 : 2;       // fragments per wave; a patch is 2 FT fragments
  static constexpr int NIT = T ? 2 : (S == 1 ? 4 : 5);    // staged (pixel, 8-channel group) items per thread and chunk
  static constexpr int NPAR = T ? 4 : 1;
};

// EPI (T only): the transposed convolution as a layer of its own (ssdk_convttrain.hip) -- bias and skip map added in fp32 to the
// accumulators of the four parity classes, one rounding.  Without EPI the instances are those the dense 3x3 has always had.
template <int DT, int S, bool T, bool EPI = false>
__global__ __launch_bounds__(256) void conv3_train_conv_kernel(const C3ConvParams p) {
  static_assert(T || !EPI, "the epilogue belongs to the transposed form");
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
            if constexpr (EPI) {
              // the map sides are odd (2 H - 1): rows start at any 2-byte address, so elements are read and written one by one;
              // a lane covers eight consecutive pixels of one row, the wave's four lane groups 32
              const u16* sk = p.skip ? p.skip + (dst - p.y) : nullptr;
#pragma unroll
              for (int e = 0; e < 8; ++e) {
                if (ix + e < p.Wo) {
                  float v = ((e & 1) ? v1[e >> 1] : v0[e >> 1]) + bi;
                  if (sk) v += bits16_to_f32<DT>((u32)sk[e]);
                  dst[e] = (u16)f32_to_bits16<DT>(v);
                }
              }
            } else if ((p.Wo & 7) == 0 && (((uintptr_t)p.y) & 15u) == 0) {  // uniform
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

// The launch plan of conv3_train_conv_kernel: x [N, Ci, H, W] -> y [N, Co, Ho, Wo]; transposed: x is the output gradient of a stride-2
// layer, y its input gradient.  Fills p, the grid and the dynamic LDS; SSDK_E_BADARG with a message when the shape does not fit.
static inline int c3_conv_plan(const char* what, const void* x, const void* wf, const float* bias, void* y, int N, int Ci, int Co, int H,
                               int W, int Ho, int Wo, int stride, bool transposed, C3ConvParams* pp, long* pgrid, size_t* plds) {
  C3ConvParams& p = *pp;
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
  *pgrid = grid;
  *plds = lds;
  return SSDK_OK;
}

// Every kernel instance is launched from ONE translation unit.  These live in ssdk_conv3train.hip; ssdk_convttrain.hip calls them
// for the parts of the transposed layer that ARE the dense convolution's (its images, its stride-2 forward, the sum of the
// weight-gradient partials) and instantiates only its own epilogue forward and bias-gradient weight pass.
int c3_prepare(const float* w32, void* w_fwd, void* w_dgrad, int Cin, int Cout, int dtype, hipStream_t stream);
int c3_conv(const char* what, const void* x, const void* wf, const float* bias, void* y, int N, int Ci, int Co, int H, int W, int Ho,
            int Wo, int stride, bool transposed, int dtype, hipStream_t stream);
struct C3WgradParams;
void c3_wgrad_reduce(const C3WgradParams& p, hipStream_t stream);

// ---- weight gradient ------------------------------------------------------------------------------------------------------------------
struct C3WgradParams {
  const u16* x;   // [N, Ci, H, W]
  const u16* dy;  // [N, Co, Ho, Wo]
  float* part;    // [splits][ntiles][9][64][64]
  float* dw;      // [Co][Ci][3][3]
  int N, Ci, Co, H, W, Ho, Wo;
  int tci, ntiles, splits, rows_per_split, ck_log2;
  float* gbpart;  // GB only: [splits][64 tci] per-channel sums of x over each split's rows, or NULL
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

// GB (stride 2, H = 2 Ho - 1, W = 2 Wo - 1: x is the output gradient of a transposed layer): the workgroups of the first row of
// tiles also add up every x element they stage, per channel -- the bias gradient of that layer, on the pass over x the weight
// gradient makes anyway.  An output pixel (oy, ox) OWNS the x pixels (2 oy - 1 | 2 oy, 2 ox - 1 | 2 ox), so each element of the map
// is counted exactly once although rows and columns of neighbouring windows overlap.  A thread sums the items it stages over the
// steps, the items of a channel are added in index order at the end: a fixed order, no atomics.
template <int DT, int S, int CKL, bool GB = false>
__global__ __launch_bounds__(256) void conv3_train_wgrad_kernel(const C3WgradParams p) {
  static_assert(S == 2 || !GB, "the bias sum counts by stride-2 ownership");
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
  const bool do_gb = GB && p.gbpart && co0 == 0;  // uniform
  float gbacc[GB ? NIX : 1];
#pragma unroll
  for (int j = 0; j < (GB ? NIX : 1); ++j) gbacc[j] = 0.f;
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
      if constexpr (GB) {
        if (do_gb) {  // rows ky = 0, 1 and columns 2 ox0 - 1 .. 2 (ox0 + 8 CKG) - 2 of the window are this step's own
          const bool own = ky < 2 && cl < 64;
          const float lo = (own && d >= 1 && d <= 8 * CKG) ? bits16_to_f32<DT>(v & 0xffffu) : 0.f;
          const float hi = (own && d < 8 * CKG) ? bits16_to_f32<DT>(v >> 16) : 0.f;
          gbacc[j] += lo + hi;
        }
      }
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
  if constexpr (GB) {
    if (do_gb) {  // xS is free after the last step's barrier
      float* red = reinterpret_cast<float*>(xS);
#pragma unroll
      for (int j = 0; j < NIX; ++j) {
        const int i = (int)tid + 256 * j;
        const int cl = i / XPER, rem = i - cl * XPER;
        if (cl < 64) red[cl * XCS + rem] = gbacc[j];
      }
      __syncthreads();
      if (tid < 64u) {
        float sum = 0.f;
        for (int q = 0; q < XPER; ++q) sum += red[(int)tid * XCS + q];
        p.gbpart[(size_t)split * (64 * p.tci) + ci0 + (int)tid] = sum;
      }
    }
  }
}

static inline void c3_wgrad_plan(int N, int Ci, int Co, int Ho, int Wo, C3WgradParams* p) {
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

static inline int c3_check(const char* what, int N, int Cin, int Cout, int H, int W, int stride, int dtype) {
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
