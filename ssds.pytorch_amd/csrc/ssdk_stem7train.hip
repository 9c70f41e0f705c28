// ssdk_stem7train.hip -- the 7x7 / stride 2 / pad 3 image-side convolution of the ResNet / ResNeXt backbones inside the training
// step (nets/resnet.py: conv1, nn.Conv2d(3, 64, 7, 2, 3, bias=False)): Cin <= 3 image channels (49 * Cin <= 147 taps) to
// Cout <= 64 channels.  Forward and weight gradient; an image has no input gradient.  16-bit NCHW tensors as autograd hands them
// over, fp32 master weights.  The same character as the 3x3 stem (ssdk_stemtrain.hip): a STREAM -- at batch 32 / 640 x 640,
// 78.6 MB of image in and 419 MB out (forward), the same two tensors in (weight gradient).
//
//   forward      stem7_train_fwd_kernel: the layer as a GEMM on the matrix cores with k = 8 r + j -- r = 7 ci + ky one of the
//                <= 21 (channel, kernel row) pairs, j the eight image columns 2 ox - 4 .. 2 ox + 3 of which j = 0 carries a zero
//                weight and j = 1 .. 7 are kx = 0 .. 6 -- so that a lane's eight consecutive k are 16 contiguous bytes of one image
//                row at a 4-byte aligned address: no gather, no LDS.  K = 168 padded to 192, six k-steps (two / four for one / two
//                channels).  The weights, rounded to the tensor dtype here (what autocast's cast of the parameter did), are the
//                loop-invariant A operand in registers.
//   weight grad  stem7_train_wgrad_kernel: dW[co][tap] = sum over pixels dy[co][p] patch[tap][p] contracts over PIXELS, which are
//                contiguous in dy and stride-2 in x: v_mfma_f32_16x16x32 with A = dy (16 channels x 32 pixels: one 16-byte load
//                per lane) and B = patch (16 taps x 32 pixels: the 16 image columns that hold the lane's eight stride-2 columns,
//                their even or odd halves picked with v_perm_b32).  M = 4 channel fragments, N = 10 tap fragments: 40
//                accumulator fragments, split over the two tap halves of a workgroup's wave pairs (20 fragments = 80 registers a
//                wave).  Waves 0 / 1 and 2 / 3 walk different output rows; the pair 2 / 3 hands its sums over through LDS and
//                waves 0 / 1 add them (wave order), workgroup partials go to the workspace and stem7_train_wgrad_reduce_kernel adds
//                them in index order: no float atomics, bit-reproducible.
// Every load is unconditional on a clamped address and masked afterwards; offsets are size_t.
#include "ssdk_conv_common.h"

namespace ssdk {

struct Stem7TrainParams {
  const u16* x;     // [N, Cin, H, W]
  const float* w;   // forward: [Cout, Cin, 7, 7] fp32 master weights
  u16* y;           // forward: [N, Cout, Ho, Wo]
  const u16* dy;    // weight gradient: [N, Cout, Ho, Wo]
  float* part;      // weight gradient: [partials][64 * 160]
  float* dw;        // weight gradient: [Cout, Cin, 7, 7]
  int N, Cin, H, W, Cout, Ho, Wo;
  int rows_per_wave;  // output rows (n, oy) per wave
  int partials;
};

constexpr int kStem7Taps = 160;              // 147 taps padded to ten 16-tap fragments
constexpr int kStem7Tile = 64 * kStem7Taps;  // one partial: [64 channels][160 taps] fp32

typedef u32 u32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));  // a 16-byte load at a 4-byte aligned address

// o[i] = q[i + s] (zero outside the array) for s = -2 .. 1, all zero for any other s: moves a run of dwords that was loaded from
// a clamped column back to where the window wanted it
template <int NQ>
__device__ __forceinline__ void stem7_shift(u32 (&q)[NQ], int s) {
  u32 o[NQ];
#pragma unroll
  for (int i = 0; i < NQ; ++i) {
    const u32 up = i + 1 < NQ ? q[i + 1] : 0u, dn1 = i >= 1 ? q[i - 1] : 0u, dn2 = i >= 2 ? q[i - 2] : 0u;
    o[i] = s == 0 ? q[i] : (s == 1 ? up : (s == -1 ? dn1 : (s == -2 ? dn2 : 0u)));
  }
#pragma unroll
  for (int i = 0; i < NQ; ++i) q[i] = o[i];
}

// ---- forward ---------------------------------------------------------------------------------------------------------------
// columns c0 .. c0 + 7 (c0 even) of one image row as four dwords, zero outside the row.  FAST (W even and >= 8, 4-byte aligned
// tensor): one 16-byte load inside the row; `edge` (wave-uniform) says that some lane's window leaves the row.
template <bool FAST>
__device__ __forceinline__ u32x4 stem7_window(const u16* row, int c0, int W, bool edge) {
  u32 q[4];
  if constexpr (FAST) {
    const int cs = c0 < 0 ? 0 : (c0 > W - 8 ? W - 8 : c0);
    const u32x4 v = *reinterpret_cast<const u32x4_a4*>(row + cs);
#pragma unroll
    for (int i = 0; i < 4; ++i) q[i] = v[i];
    if (edge) stem7_shift<4>(q, (c0 - cs) >> 1);
  } else {
    const int last = W - 1;
    u32 e[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int c = c0 + i;
      const u32 t = row[c < 0 ? 0 : (c < last ? c : last)];
      e[i] = (c >= 0 && c < W) ? t : 0u;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) q[i] = e[2 * i] | (e[2 * i + 1] << 16);
  }
  return u32x4{q[0], q[1], q[2], q[3]};
}

// y[co][px] = sum_k A[co][k] B[k][px].  The B operand of v_mfma_f32_16x16x32 wants eight consecutive k of one pixel per lane: in
// k-step ks lane group fg holds (channel, kernel row) pair r = 4 ks + fg.  A wave iteration is 32 neighbouring pixels of one
// output row as two tiles of the EVEN / ODD pixels, so a lane ends up with two neighbouring pixels of four channels per channel
// fragment: one 4-byte store per channel, 64 contiguous bytes per 16 lanes.  Channels >= Cout (padding lanes) store nothing.
template <int DT, bool FAST>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(FAST ? 2 : 1))) void stem7_train_fwd_kernel(const Stem7TrainParams p) {
  const u32 tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const int fr = (int)(lane & 15u), fg = (int)(lane >> 4);
  const int rows = 7 * p.Cin, taps = 49 * p.Cin;
  const int nks = (rows + 3) >> 2;  // uniform: k-steps that hold a row
  // the weights as A fragments [channel fragment][k-step][lane][8], rounded to the tensor dtype (what autocast's cast of the
  // parameter did), zero in the padding: built once per workgroup in LDS, then 24 16-byte reads per lane
  __shared__ __attribute__((aligned(16))) u16 sw[24 * 64 * 8];
  for (u32 i = tid; i < 24u * 64u * 8u; i += 256u) {
    const int e = (int)(i & 7u), ln = (int)((i >> 3) & 63u), f = (int)(i >> 9);
    const int co = 16 * (f / 6) + (ln & 15), r = 4 * (f % 6) + (ln >> 4);
    const bool ok = e > 0 && r < rows && co < p.Cout;
    const float wv = p.w[ok ? (size_t)co * taps + r * 7 + (e - 1) : 0];
    sw[i] = ok ? (u16)f32_to_bits16<DT>(wv) : (u16)0;
  }
  __syncthreads();
  u32x4 Aw[4][6];
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int ks = 0; ks < 6; ++ks) Aw[t][ks] = *reinterpret_cast<const u32x4*>(sw + ((t * 6 + ks) * 64 + (int)lane) * 8);
  const size_t plane = (size_t)p.Ho * p.Wo;
  const int total_rows = p.N * p.Ho;
  const int wid = (int)(blockIdx.x * 4u + wave);
  const int r0 = wid * p.rows_per_wave, r1 = r0 + p.rows_per_wave < total_rows ? r0 + p.rows_per_wave : total_rows;
  const bool pack = (p.Wo & 1) == 0 && (((uintptr_t)p.y) & 3u) == 0;  // uniform: 4-byte stores of pixel pairs
  for (int r = r0; r < r1; ++r) {  // wave-uniform
    const int n = r / p.Ho, oy = r - n * p.Ho;
    const u16* xrow[6];
    bool xok[6];
#pragma unroll
    for (int ks = 0; ks < 6; ++ks) {
      const int rr = 4 * ks + fg, ci = rr / 7, ky = rr - 7 * ci, iy = 2 * oy + ky - 3;
      xok[ks] = rr < rows && (unsigned)iy < (unsigned)p.H;
      xrow[ks] = p.x + (((size_t)n * p.Cin + (xok[ks] ? ci : 0)) * p.H + (xok[ks] ? iy : 0)) * p.W;
    }
    u16* yrow = p.y + (size_t)n * p.Cout * plane + (size_t)oy * p.Wo;
    // the loads of a tile (T = 0 / 1: the even / odd pixels of a 32-pixel chunk), one per k-step; the NEXT tile is requested before
    // this one is multiplied
    auto load_tile = [&](int ox0, int T, u32x4 (&raw)[6]) {
      const int c0 = 2 * (ox0 + 2 * fr + T) - 4;             // first column of the pixel's window
      const bool edge = ox0 == 0 || 2 * ox0 + 58 > p.W - 8;  // (uniform) a window of this chunk leaves the row
#pragma unroll
      for (int ks = 0; ks < 6; ++ks) {
        if (ks < nks) raw[ks] = stem7_window<FAST>(xrow[ks], c0, p.W, edge);
        else raw[ks] = u32x4{0u, 0u, 0u, 0u};
      }
    };
    auto multiply = [&](const u32x4 (&raw)[6], f32x4 (&acc)[4]) {
#pragma unroll
      for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < 6; ++ks) {
        if (ks < nks) {  // uniform
          u32x4 B = raw[ks];
          B[0] &= 0xffff0000u;  // j = 0: the column in front of the window (its weight is zero; keep a non-finite pixel out)
#pragma unroll
          for (int q = 0; q < 4; ++q) B[q] = xok[ks] ? B[q] : 0u;
#pragma unroll
          for (int t = 0; t < 4; ++t) acc[t] = mfma16<DT>(Aw[t][ks], B, acc[t]);
        }
      }
    };
    u32x4 even[6], odd[6];
    load_tile(0, 0, even);
    for (int ox0 = 0; ox0 < p.Wo; ox0 += 32) {
      f32x4 acc[2][4];  // [tile][channel fragment]
      load_tile(ox0, 1, odd);
      multiply(even, acc[0]);
      if (ox0 + 32 < p.Wo) load_tile(ox0 + 32, 0, even);  // (uniform)
      multiply(odd, acc[1]);
      // D[m = 4 fg + i][n = fr] of (tile T, channel fragment t) = y[co = 16 t + 4 fg + i][pixel ox0 + 2 fr + T]
      const int ox = ox0 + 2 * fr;
      const u32 yoff = (u32)(4 * fg) * (u32)plane + (u32)ox;  // (stem7_check: 64 planes are below 2^31 elements)
      if (ox < p.Wo) {
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int co = 16 * t + 4 * fg + i;
            if (co < p.Cout) {
              u16* dst = yrow + (size_t)(16 * t + i) * plane + yoff;  // (a uniform address and a 32-bit lane offset)
              if (pack) {
                *reinterpret_cast<u32*>(dst) = pack2_16<DT>(acc[0][t][i], acc[1][t][i]);
              } else {
                dst[0] = (u16)f32_to_bits16<DT>(acc[0][t][i]);
                if (ox + 1 < p.Wo) dst[1] = (u16)f32_to_bits16<DT>(acc[1][t][i]);
              }
            }
          }
      }
    }
  }
}

// ---- weight gradient ---------------------------------------------------------------------------------------------------------
// B fragment of one k-step: the lane's tap (ci, ky, kx) at the eight output pixels ox .. ox + 7 of row oy = the columns
// 2 (ox + j) + kx - 3 of image row 2 oy + ky - 3: the even (kx odd) or odd (kx even) halves of the eight dwords that start at the
// even column ce = 2 ox + 2 floor((kx - 3) / 2).
// FAST (W a multiple of 16, x 4-byte and dy 16-byte aligned): an eight-pixel group lies inside the row or completely outside it,
// and the 16 columns are two 16-byte loads inside the row; `edge` (wave-uniform) says that some lane's columns leave the row.
template <bool FAST>
__device__ __forceinline__ u32x4 stem7_patch(const u16* row, int ox, int kx, int W, int Wo, bool edge, bool ok) {
  u32x4 out;
  if constexpr (FAST) {
    const int ce = 2 * ox + 2 * ((kx - 3) >> 1);
    const int cs = ce < 0 ? 0 : (ce > W - 16 ? W - 16 : ce);
    const u32x4 v0 = *reinterpret_cast<const u32x4_a4*>(row + cs), v1 = *reinterpret_cast<const u32x4_a4*>(row + cs + 8);
    u32 d[8] = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
    if (edge) stem7_shift<8>(d, (ce - cs) >> 1);
    const u32 sel = (kx & 1) ? 0x05040100u : 0x07060302u;  // low halves (even columns) / high halves
#pragma unroll
    for (int j = 0; j < 4; ++j) out[j] = ok ? __builtin_amdgcn_perm(d[2 * j + 1], d[2 * j], sel) : 0u;
  } else {
    const int last = W - 1;
    u32 e[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int c = 2 * (ox + j) + kx - 3;
      const u32 t = row[c < 0 ? 0 : (c < last ? c : last)];
      e[j] = (ok && c >= 0 && c < W && ox + j < Wo) ? t : 0u;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) out[j] = e[2 * j] | (e[2 * j + 1] << 16);
  }
  return out;
}

template <bool FAST>
__device__ __forceinline__ u32x4 stem7_dy_load(const u16* row, int ox, int Wo) {  // eight pixels ox .. ox + 7 of one channel row
  u32x4 out;
  if constexpr (FAST) {
    out = *reinterpret_cast<const u32x4*>(row + (ox < Wo ? ox : Wo - 8));
  } else {
    const int last = Wo - 1;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int c = ox + 2 * i;
      const u32 e0 = row[c < last ? c : last], e1 = row[c + 1 < last ? c + 1 : last];
      out[i] = (c < Wo ? e0 : 0u) | ((c + 1 < Wo ? e1 : 0u) << 16);
    }
  }
  return out;
}

template <int DT, bool FAST>
__global__ __launch_bounds__(256) void stem7_train_wgrad_kernel(const Stem7TrainParams p) {
  __shared__ float red[kStem7Tile];
  const u32 tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const int fr = (int)(lane & 15u), fg = (int)(lane >> 4);
  const int th = (int)(wave & 1u), ph = (int)(wave >> 1);  // tap half (fragments 5 th .. 5 th + 4), row half of the workgroup
  const int taps = p.Cin * 49;
  // this lane's five taps (B fragments) and four channels (A fragments)
  int t_ci[5], t_ky[5], t_kx[5];
  bool t_ok[5];
#pragma unroll
  for (int f = 0; f < 5; ++f) {
    const int tap = (5 * th + f) * 16 + fr;
    t_ok[f] = tap < taps;
    const int tt = t_ok[f] ? tap : 0;
    t_ci[f] = tt / 49;
    t_ky[f] = (tt % 49) / 7;
    t_kx[f] = tt % 7;
  }
  bool c_ok[4];
#pragma unroll
  for (int a = 0; a < 4; ++a) c_ok[a] = 16 * a + fr < p.Cout;
  f32x4 acc[4][5];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int f = 0; f < 5; ++f) acc[a][f] = f32x4{0.f, 0.f, 0.f, 0.f};
  const size_t plane = (size_t)p.Ho * p.Wo;
  const int total_rows = p.N * p.Ho;
  const long rb = ((long)blockIdx.x * 2 + ph) * p.rows_per_wave;
  const int r0 = rb < total_rows ? (int)rb : total_rows;
  const int r1 = r0 + p.rows_per_wave < total_rows ? r0 + p.rows_per_wave : total_rows;
  for (int r = r0; r < r1; ++r) {  // wave-uniform
    const int n = r / p.Ho, oy = r - n * p.Ho;
    const u16* xrow[5];
    bool xok[5];
#pragma unroll
    for (int f = 0; f < 5; ++f) {
      const int iy = 2 * oy + t_ky[f] - 3;
      xok[f] = t_ok[f] && (unsigned)iy < (unsigned)p.H;
      xrow[f] = p.x + (((size_t)n * p.Cin + t_ci[f]) * p.H + (xok[f] ? iy : 0)) * p.W;
    }
    const u16* grow[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) grow[a] = p.dy + ((size_t)n * p.Cout + (c_ok[a] ? 16 * a + fr : 0)) * plane + (size_t)oy * p.Wo;
    // a k-step = 32 output pixels: lane group fg holds pixels ox0 + 8 fg .. + 7
    for (int ox0 = 0; ox0 < p.Wo; ox0 += 32) {
      const int ox = ox0 + 8 * fg;
      const bool in = ox < p.Wo;
      const bool edge = ox0 == 0 || 2 * ox0 + 50 > p.W - 16;  // (uniform) a lane's 16 columns (from 2 ox0 - 4 .. 2 ox0 + 50) leave the row
      const int oxc = FAST ? (in ? ox : p.Wo - 8) : ox;
      u32x4 A[4], B[5];
#pragma unroll
      for (int a = 0; a < 4; ++a) A[a] = stem7_dy_load<FAST>(grow[a], ox, p.Wo);
#pragma unroll
      for (int f = 0; f < 5; ++f) B[f] = stem7_patch<FAST>(xrow[f], oxc, t_kx[f], p.W, p.Wo, edge, xok[f] && in);
#pragma unroll
      for (int a = 0; a < 4; ++a) {
#pragma unroll
        for (int i = 0; i < 4; ++i) A[a][i] = (c_ok[a] && in) ? A[a][i] : 0u;
#pragma unroll
        for (int f = 0; f < 5; ++f) acc[a][f] = mfma16<DT>(A[a], B[f], acc[a][f]);
      }
    }
  }
  // D[m = 4 fg + j][n = fr] of fragment (a, f) = dW[co = 16 a + 4 fg + j][tap = 16 (5 th + f) + fr]
  if (ph == 1) {
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int f = 0; f < 5; ++f)
#pragma unroll
        for (int j = 0; j < 4; ++j) red[(16 * a + 4 * fg + j) * kStem7Taps + (5 * th + f) * 16 + fr] = acc[a][f][j];
  }
  __syncthreads();
  if (ph == 0) {
    float* part = p.part + (size_t)blockIdx.x * kStem7Tile;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int f = 0; f < 5; ++f)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int i = (16 * a + 4 * fg + j) * kStem7Taps + (5 * th + f) * 16 + fr;
          part[i] = acc[a][f][j] + red[i];
        }
  }
}

// dw[co][tap] = sum of the workgroup partials in index order: 64 row groups x 16 elements per workgroup, each group adds its
// partials g, g + 64, ... in order, the groups are added in order
__global__ __launch_bounds__(1024) void stem7_train_wgrad_reduce_kernel(const Stem7TrainParams p) {
  __shared__ float red[64][16];
  const u32 el = threadIdx.x & 15u, g = threadIdx.x >> 4;
  const u32 i = blockIdx.x * 16u + el;  // element of the 64 x 160 tile
  float s = 0.f;
  for (int q = (int)g; q < p.partials; q += 64) s += p.part[(size_t)q * kStem7Tile + i];
  red[g][el] = s;
  __syncthreads();
  if (g == 0) {
    float t = red[0][el];
    for (int k = 1; k < 64; ++k) t += red[k][el];
    const int co = (int)(i / (u32)kStem7Taps), tap = (int)(i % (u32)kStem7Taps), taps = p.Cin * 49;
    if (co < p.Cout && tap < taps) p.dw[(size_t)co * taps + tap] = t;
  }
}

static int stem7_check(const char* what, const void* x, int N, int Cin, int H, int W, int Cout, int dtype) {
  if (!x || N < 1 || Cin < 1 || Cin > 3 || H < 1 || W < 1 || Cout < 1 || Cout > 64 || (dtype != SSDK_BF16 && dtype != SSDK_F16)) {
    set_error("%s: bad arguments (N=%d Cin=%d H=%d W=%d Cout=%d dtype=%d; Cin <= 3, Cout <= 64, 16-bit tensors)", what, N, Cin, H, W, Cout,
              dtype);
    return SSDK_E_BADARG;
  }
  const size_t Ho = ((size_t)H - 1) / 2 + 1, Wo = ((size_t)W - 1) / 2 + 1;
  if ((size_t)N * 64 * Ho * Wo >= (1ull << 40) || (size_t)N * Ho >= (1ull << 30) || Ho * Wo >= (1ull << 24) || W >= (1 << 28)) {
    set_error("%s: tensor too large", what);
    return SSDK_E_BADARG;
  }
  return SSDK_OK;
}

// output rows (n, oy) per wave so that ~2048 waves share the work (two workgroups of four waves on each of 256 compute units, the
// occupancy the kernels' registers allow); -> rows
static long stem7_rows_per_wave(int N, int Ho) {
  const long rows = (long)N * Ho;
  const long rpw = (rows + 2048 - 1) / 2048;
  return rpw < 1 ? 1 : rpw;
}
static int stem7_fwd_blocks(int N, int Ho, int* rows_per_wave) {  // four waves, each its own rows
  const long rpw = stem7_rows_per_wave(N, Ho);
  *rows_per_wave = (int)rpw;
  return (int)(((long)N * Ho + rpw * 4 - 1) / (rpw * 4));
}
static int stem7_wgrad_blocks(int N, int Ho, int* rows_per_wave) {  // two wave pairs, each pair its own rows
  const long rpw = stem7_rows_per_wave(N, Ho);
  *rows_per_wave = (int)rpw;
  return (int)(((long)N * Ho + rpw * 2 - 1) / (rpw * 2));
}

static void stem7_fill(Stem7TrainParams* p, const void* x, int N, int Cin, int H, int W, int Cout) {
  memset(p, 0, sizeof(*p));
  p->x = (const u16*)x;
  p->N = N;
  p->Cin = Cin;
  p->H = H;
  p->W = W;
  p->Cout = Cout;
  p->Ho = (H - 1) / 2 + 1;
  p->Wo = (W - 1) / 2 + 1;
}

}  // namespace ssdk

using namespace ssdk;

extern "C" size_t ssdk_stem7x7s2_wgrad_workspace_bytes(int N, int H, int W, int Cout) {
  if (N < 1 || H < 1 || W < 1 || Cout < 1 || Cout > 64 || (size_t)N * (((size_t)H - 1) / 2 + 1) >= (1ull << 30)) return 0;
  int rpw = 1;
  return (size_t)stem7_wgrad_blocks(N, (H - 1) / 2 + 1, &rpw) * kStem7Tile * sizeof(float);  // the workgroup partials [partials][64 x 160] fp32
}

extern "C" int ssdk_stem7x7s2_fwd(const void* x, const float* w, void* y, int N, int Cin, int H, int W, int Cout, int dtype, void* stream) {
  if (int rc = stem7_check("stem7x7s2_fwd", x, N, Cin, H, W, Cout, dtype)) return rc;
  if (!w || !y) {
    set_error("stem7x7s2_fwd: null pointer");
    return SSDK_E_BADARG;
  }
  Stem7TrainParams p;
  stem7_fill(&p, x, N, Cin, H, W, Cout);
  p.w = w;
  p.y = (u16*)y;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)stem7_fwd_blocks(N, p.Ho, &p.rows_per_wave));
  const bool fast = (W & 1) == 0 && W >= 8 && (((uintptr_t)x) & 3u) == 0;
  if (dtype == SSDK_BF16) {
    if (fast) hipLaunchKernelGGL((stem7_train_fwd_kernel<SSDK_BF16, true>), grid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL((stem7_train_fwd_kernel<SSDK_BF16, false>), grid, dim3(256), 0, st, p);
  } else {
    if (fast) hipLaunchKernelGGL((stem7_train_fwd_kernel<SSDK_F16, true>), grid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL((stem7_train_fwd_kernel<SSDK_F16, false>), grid, dim3(256), 0, st, p);
  }
  return check_launch("stem7_train_fwd_kernel");
}

extern "C" int ssdk_stem7x7s2_wgrad(const void* x, const void* dy, float* dw, void* workspace, size_t workspace_bytes, int N, int Cin,
                                    int H, int W, int Cout, int dtype, void* stream) {
  if (int rc = stem7_check("stem7x7s2_wgrad", x, N, Cin, H, W, Cout, dtype)) return rc;
  if (!dy || !dw || !workspace || workspace_bytes < ssdk_stem7x7s2_wgrad_workspace_bytes(N, H, W, Cout) || ((uintptr_t)workspace & 15u)) {
    set_error("stem7x7s2_wgrad: null pointer, or workspace too small / misaligned");
    return SSDK_E_BADARG;
  }
  Stem7TrainParams p;
  stem7_fill(&p, x, N, Cin, H, W, Cout);
  p.dy = (const u16*)dy;
  p.dw = dw;
  p.part = (float*)workspace;
  p.partials = stem7_wgrad_blocks(N, p.Ho, &p.rows_per_wave);
  hipStream_t st = (hipStream_t)stream;
  const bool fast = (W & 15) == 0 && (((uintptr_t)x) & 3u) == 0 && (((uintptr_t)dy) & 15u) == 0;  // (then Wo = W / 2 is a multiple of 8)
  const dim3 grid((unsigned)p.partials);
  if (dtype == SSDK_BF16) {
    if (fast) hipLaunchKernelGGL((stem7_train_wgrad_kernel<SSDK_BF16, true>), grid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL((stem7_train_wgrad_kernel<SSDK_BF16, false>), grid, dim3(256), 0, st, p);
  } else {
    if (fast) hipLaunchKernelGGL((stem7_train_wgrad_kernel<SSDK_F16, true>), grid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL((stem7_train_wgrad_kernel<SSDK_F16, false>), grid, dim3(256), 0, st, p);
  }
  hipLaunchKernelGGL(stem7_train_wgrad_reduce_kernel, dim3(kStem7Tile / 16), dim3(1024), 0, st, p);
  return check_launch("stem7_train_wgrad_kernel");
}
