// ssdk_mbconvtrain.hip -- the EfficientNet MBConv layers of the TRAINING step that had no kernels: the 5x5 depthwise convolution
// (pad 2, stride 1 | 2, no bias) with both gradients, and SiLU + squeeze-excite as one function of the depthwise BatchNorm's
// output u:  z = silu(u) g,  g = sigmoid(W2 silu(W1 mean_hw(silu(u)) + b1) + b2).  NCHW, bf16 | f16, fp32 arithmetic, one rounding
// on every 16-bit store.  No allocation, no synchronisation, no atomics: every sum runs in a fixed order (two runs: same bits).
//
// Depthwise 5x5.  A workgroup of 256 threads owns a tile of TR output rows x TC = 8 TCu output columns of G planes (G > 1 only
// where a whole plane is one tile: the 32 x 32 / 16 x 16 / 8 x 8 maps).  The input window of the tile is staged in LDS as fp32 with
// its zero halo; a thread owns a UNIT of eight consecutive outputs of one row and walks the five input rows with a sliding window
// of 7 S + 5 staged values in registers (12 | 19), so the 25 taps cost 8 accumulators + one window row, not a 5 x 5 patch per
// output.  The 25 weights of a plane sit in LDS (uniform per plane, broadcast reads).
//   dw5_fwd_kernel<DT, S>    forward; with ``flip`` (the weights staged reversed) it IS the stride-1 input gradient
//   dw5_dgrad2_kernel<DT>    stride-2 input gradient by the parity of the dx pixel: rows / columns of even index take the taps
//                            {0, 2, 4}, odd ones {1, 3}; dy is staged as it is (no zero-inserted tensor)
//   dw5_wgrad_kernel<DT, S>  G images of ONE channel per workgroup; a thread adds the 8 products of its unit into 25 accumulators
//                            (fmaf chain of 8), the wave adds by the xor tree (6), the four waves in order (3) -> a workgroup
//                            partial in the workspace [C][25][parts]
//   dw5_wgrad_reduce_kernel  a wave per (channel, tap): lane l adds the partials l, l + 64, ... in order, then the xor tree
//
// SiLU + squeeze-excite.  silu(u) = u * rcp(1 + exp2(-log2(e) u)) on the hardware exp2 / rcp, in fp32 from the stored u.
//   se_sum_kernel<DT, WAVES, DOT>   per-plane reduction.  WAVES = 1: a wave per plane (HW < 1024); 4: a workgroup per plane, each
//                            wave a contiguous quarter.  Lane l owns the octets l, l + 64, ... of its range, ELEMENT e of every
//                            octet in accumulator e (8 chains), then acc 0..7 as a tree (3), the xor tree (6), the four waves in
//                            order (3).  DOT = false: pooled = sum silu(u) / HW; DOT = true: dgate_raw = sum dz silu(u).
//                            The order does not depend on the alignment (a 16-byte load where the address allows, 8 scalar loads
//                            otherwise: the same values in the same accumulators).
//   se_gate_kernel           a workgroup per image: FC1 (a wave per output, lanes stride over C, xor tree) + b1 -> hidden_pre,
//                            silu, FC2 (a lane per channel, Cr terms in index order) + b2, sigmoid -> gate.  fp32 parameters.
//   se_elem_kernel<DT, BWD>  flat octets over the whole tensor (a 16-byte access where the tensor bases allow, scalar otherwise), the
//                            plane's gate looked up per element, one rounding.  BWD = false: z = silu(u) gate[plane]; BWD = true:
//                            du = (dz g + dpool / HW) silu'(u), silu'(u) = s (1 + u (1 - s)), s = sigmoid(u)
//   se_gate_bwd_kernel       a workgroup per image: dv2 = dgate_raw g (1 - g), ds = W2^T dv2, dh = ds silu'(hidden_pre),
//                            dpool = W1^T dh; dv2, silu(hidden_pre), dh go to the workspace
//   se_param_grad_kernel     a thread per parameter element: the sum over the images in image order
#include "ssdk_conv_common.h"

namespace ssdk {

constexpr int kDw5Lds = 10240;   // floats of staged input per workgroup (40 KB)
constexpr int kDw5MaxG = 64;     // planes per workgroup (weights in LDS: 64 x 25)
constexpr int kSeMaxC = 4096;    // gate kernels: LDS vectors over C
constexpr int kSeMaxR = 1024;    // ... and over Cr
constexpr int kSeWgPlane = 1024; // planes of at least this many pixels get a workgroup each in se_sum_kernel

template <int DT> __device__ __forceinline__ u32 dw5_round16(float v) { return pack2_16<DT>(v, 0.f) & 0xffffu; }

__device__ __forceinline__ float se_sigmoid(float v) { return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.442695041f * v)); }
__device__ __forceinline__ float se_silu(float v) { return v * se_sigmoid(v); }
__device__ __forceinline__ float se_dsilu(float v) {
  const float s = se_sigmoid(v);
  return s * (1.0f + v * (1.0f - s));
}

// ---- depthwise 5x5 ----------------------------------------------------------------------------------------------------------------
struct Dw5Plan {
  int TR, TCu, bands, ctiles, G, IR, IC, groups;  // groups: of planes (forward, input gradient) or of images (weight gradient)
};

struct Dw5Params {
  const u16* src;   // the staged tensor: x (forward, weight gradient) or dy (input gradients)
  const u16* w;     // [C][25] 16 bit
  const u16* dy;    // weight gradient only
  u16* dst;         // y or dx
  float* ws;        // weight gradient partials [C][25][parts]
  float* dw;
  int N, C;
  int Hs, Ws;       // the staged tensor's plane
  int Hd, Wd;       // the plane the threads' units live in (y; dx; dy for the weight gradient)
  int flip;
  int parts;
  Dw5Plan pl;
};

// all 256 threads: G windows of IR x IC staged values starting at (ys0, xs0) of the planes plane0 + g * pstride, zero outside
template <int DT>
__device__ __forceinline__ void dw5_stage(float* tile, const Dw5Params& p, long plane0, long pstride, int nplanes_ok, int ys0, int xs0) {
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  const int rows = p.pl.G * p.pl.IR;
  for (int rr = wave; rr < rows; rr += 4) {
    const int g = rr / p.pl.IR, iy = rr - g * p.pl.IR;
    const int gy = ys0 + iy;
    const bool rok = g < nplanes_ok && (unsigned)gy < (unsigned)p.Hs;
    const u16* row = p.src + ((size_t)(plane0 + (long)g * pstride) * p.Hs + (rok ? gy : 0)) * (size_t)p.Ws;
    float* trow = tile + (size_t)rr * p.pl.IC;
    for (int ix = lane; ix < p.pl.IC; ix += 64) {
      const int gx = xs0 + ix;
      float v = 0.f;
      if (rok && (unsigned)gx < (unsigned)p.Ws) v = bits16_to_f32<DT>(row[gx]);
      trow[ix] = v;
    }
  }
}

// eight outputs of one row -> dst, a 16-byte store where the address allows and the unit is whole
template <int DT>
__device__ __forceinline__ void dw5_store8(u16* rowp, int ox, int W, const float (&acc)[8]) {
  u16* d = rowp + ox;
  if (ox + 8 <= W && ((uintptr_t)d & 15u) == 0) {
    u32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = pack2_16<DT>(acc[2 * e], acc[2 * e + 1]);
    *reinterpret_cast<u32x4*>(d) = o;
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (ox + j < W) d[j] = (u16)dw5_round16<DT>(acc[j]);
  }
}

struct Dw5Where {
  int grp, band, ct, g, r, seg;
  bool unit;
};
__device__ __forceinline__ Dw5Where dw5_where(const Dw5Plan& pl) {
  Dw5Where q;
  int b = (int)blockIdx.x;
  q.ct = b % pl.ctiles;
  b /= pl.ctiles;
  q.band = b % pl.bands;
  q.grp = b / pl.bands;
  const int upp = pl.TR * pl.TCu, u = (int)threadIdx.x;
  q.g = u / upp;
  const int v = u - q.g * upp;
  q.r = v / pl.TCu;
  q.seg = v - q.r * pl.TCu;
  q.unit = q.g < pl.G;
  return q;
}

template <int DT, int S>
__global__ __launch_bounds__(256) void dw5_fwd_kernel(const Dw5Params p) {
  __shared__ float tile[kDw5Lds];
  __shared__ float wl[kDw5MaxG * 25];
  const Dw5Plan& pl = p.pl;
  const Dw5Where q = dw5_where(pl);
  const long planes = (long)p.N * p.C;
  const long plane0 = (long)q.grp * pl.G;
  const int nok = (int)min((long)pl.G, planes - plane0);
  const int oy0 = q.band * pl.TR, ox0 = q.ct * pl.TCu * 8;
  for (int i = (int)threadIdx.x; i < pl.G * 25; i += 256) {
    const int g = i / 25, t = i - g * 25;
    float v = 0.f;
    if (g < nok) v = bits16_to_f32<DT>(p.w[(size_t)((plane0 + g) % p.C) * 25 + (p.flip ? 24 - t : t)]);
    wl[i] = v;
  }
  dw5_stage<DT>(tile, p, plane0, 1, nok, oy0 * S - 2, ox0 * S - 2);
  __syncthreads();
  const int oy = oy0 + q.r, ox = ox0 + q.seg * 8;
  if (!q.unit || q.g >= nok || oy >= p.Hd || ox >= p.Wd) return;
  constexpr int NW = 7 * S + 5;
  float acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = 0.f;
  const float* wp = wl + q.g * 25;
  const float* base = tile + ((size_t)q.g * pl.IR + q.r * S) * pl.IC + q.seg * 8 * S;
#pragma unroll
  for (int ky = 0; ky < 5; ++ky) {
    float win[NW];
#pragma unroll
    for (int i = 0; i < NW; ++i) win[i] = base[ky * pl.IC + i];
#pragma unroll
    for (int kx = 0; kx < 5; ++kx) {
      const float wv = wp[ky * 5 + kx];
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] = fmaf(win[j * S + kx], wv, acc[j]);
    }
  }
  dw5_store8<DT>(p.dst + ((size_t)(plane0 + q.g) * p.Hd + oy) * (size_t)p.Wd, ox, p.Wd, acc);
}

// stride-2 input gradient: the units live in dx (Hd x Wd), dy (Hs x Ws) is staged from (y0 / 2 - 1, x0 / 2 - 1); tile origins are even
template <int DT>
__global__ __launch_bounds__(256) void dw5_dgrad2_kernel(const Dw5Params p) {
  __shared__ float tile[kDw5Lds];
  __shared__ float wl[kDw5MaxG * 25];
  const Dw5Plan& pl = p.pl;
  const Dw5Where q = dw5_where(pl);
  const long planes = (long)p.N * p.C;
  const long plane0 = (long)q.grp * pl.G;
  const int nok = (int)min((long)pl.G, planes - plane0);
  const int y0 = q.band * pl.TR, x0 = q.ct * pl.TCu * 8;  // TR is even where there is more than one band
  for (int i = (int)threadIdx.x; i < pl.G * 25; i += 256) {
    const int g = i / 25, t = i - g * 25;
    float v = 0.f;
    if (g < nok) v = bits16_to_f32<DT>(p.w[(size_t)((plane0 + g) % p.C) * 25 + t]);
    wl[i] = v;
  }
  dw5_stage<DT>(tile, p, plane0, 1, nok, y0 / 2 - 1, x0 / 2 - 1);
  __syncthreads();
  const int iy = y0 + q.r, ix = x0 + q.seg * 8;
  if (!q.unit || q.g >= nok || iy >= p.Hd || ix >= p.Wd) return;
  float acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = 0.f;
  const float* wp = wl + q.g * 25;
  const int par = iy & 1;
#pragma unroll
  for (int t = 0; t < 3; ++t) {
    const int ky = par + 2 * t;
    if (ky < 5) {
      // dy row (iy + 2 - ky) / 2, relative to the staged origin y0 / 2 - 1
      const int dr = ((iy + 2 - ky) >> 1) - (y0 / 2 - 1);
      const float* row = tile + ((size_t)q.g * pl.IR + dr) * pl.IC + q.seg * 4;
      float win[6];
#pragma unroll
      for (int i = 0; i < 6; ++i) win[i] = row[i];
      const float* wr = wp + ky * 5;
      const float w0 = wr[0], w1 = wr[1], w2 = wr[2], w3 = wr[3], w4 = wr[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        // even column x0 + 2 j: taps 0, 2, 4 at staged columns j + 2, j + 1, j; odd column x0 + 2 j + 1: taps 1, 3 at j + 2, j + 1
        acc[2 * j] = fmaf(win[j + 2], w0, acc[2 * j]);
        acc[2 * j] = fmaf(win[j + 1], w2, acc[2 * j]);
        acc[2 * j] = fmaf(win[j], w4, acc[2 * j]);
        acc[2 * j + 1] = fmaf(win[j + 2], w1, acc[2 * j + 1]);
        acc[2 * j + 1] = fmaf(win[j + 1], w3, acc[2 * j + 1]);
      }
    }
  }
  dw5_store8<DT>(p.dst + ((size_t)(plane0 + q.g) * p.Hd + iy) * (size_t)p.Wd, ix, p.Wd, acc);
}

// weight gradient: blockIdx -> (channel, image group, band, column tile); the units live in dy (Hd x Wd), x (Hs x Ws) is staged
template <int DT, int S>
__global__ __launch_bounds__(256) void dw5_wgrad_kernel(const Dw5Params p) {
  __shared__ float tile[kDw5Lds];
  __shared__ float red[4][25];
  const Dw5Plan& pl = p.pl;
  const Dw5Where q = dw5_where(pl);
  const int c = q.grp / pl.groups, ng = q.grp - c * pl.groups;
  const int n0 = ng * pl.G;
  const int nok = min(pl.G, p.N - n0);
  const int oy0 = q.band * pl.TR, ox0 = q.ct * pl.TCu * 8;
  dw5_stage<DT>(tile, p, (long)n0 * p.C + c, p.C, nok, oy0 * S - 2, ox0 * S - 2);
  __syncthreads();
  float acc[25];
#pragma unroll
  for (int t = 0; t < 25; ++t) acc[t] = 0.f;
  const int oy = oy0 + q.r, ox = ox0 + q.seg * 8;
  if (q.unit && q.g < nok && oy < p.Hd && ox < p.Wd) {
    const u16* drow = p.dy + (((size_t)(n0 + q.g) * p.C + c) * p.Hd + oy) * (size_t)p.Wd + ox;
    float g8[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) g8[j] = ox + j < p.Wd ? bits16_to_f32<DT>(drow[j]) : 0.f;
    constexpr int NW = 7 * S + 5;
    const float* base = tile + ((size_t)q.g * pl.IR + q.r * S) * pl.IC + q.seg * 8 * S;
#pragma unroll
    for (int ky = 0; ky < 5; ++ky) {
      float win[NW];
#pragma unroll
      for (int i = 0; i < NW; ++i) win[i] = base[ky * pl.IC + i];
#pragma unroll
      for (int kx = 0; kx < 5; ++kx) {
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[ky * 5 + kx] = fmaf(g8[j], win[j * S + kx], acc[ky * 5 + kx]);
      }
    }
  }
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
#pragma unroll
  for (int t = 0; t < 25; ++t) {
    float v = acc[t];
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) v += __shfl_xor(v, d);
    if (lane == 0) red[wave][t] = v;
  }
  __syncthreads();
  if (threadIdx.x < 25) {
    const int t = (int)threadIdx.x;
    const int part = (ng * pl.bands + q.band) * pl.ctiles + q.ct;
    p.ws[((size_t)c * 25 + t) * p.parts + part] = ((red[0][t] + red[1][t]) + red[2][t]) + red[3][t];
  }
}

__global__ __launch_bounds__(256) void dw5_wgrad_reduce_kernel(const float* ws, float* dw, int rows, int parts) {
  const int lane = (int)threadIdx.x & 63;
  const int row = (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6);
  if (row >= rows) return;  // (wave-uniform, no barrier in this kernel)
  const float* src = ws + (size_t)row * parts;
  float s = 0.f;
  for (int i = lane; i < parts; i += 64) s += src[i];
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) s += __shfl_xor(s, d);
  if (lane == 0) dw[row] = s;
}

// ---- SiLU + squeeze-excite ------------------------------------------------------------------------------------------------------
// eight elements i0 .. i0 + 7 of a plane of HW elements (those below HW; the others read as zero)
template <int DT>
__device__ __forceinline__ void se_load8(const u16* plane, int i0, int HW, float (&v)[8]) {
  const u16* s = plane + i0;
  if (i0 + 8 <= HW && ((uintptr_t)s & 15u) == 0) {
    const u32x4 r = *reinterpret_cast<const u32x4*>(s);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      v[2 * e] = bits16_to_f32<DT>(r[e] & 0xffffu);
      v[2 * e + 1] = bits16_to_f32<DT>(r[e] >> 16);
    }
  } else {
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = i0 + e < HW ? bits16_to_f32<DT>(s[e]) : 0.f;
  }
}

struct SeSumParams {
  const u16* u;
  const u16* dz;
  float* out;  // [planes]
  long planes;
  int HW;
  int chunk;   // elements per wave (a multiple of 8)
  float inv;   // 1 / HW (pool) | unused
};

template <int DT, int WAVES, bool DOT>
__global__ __launch_bounds__(256) void se_sum_kernel(const SeSumParams p) {
  __shared__ float part[4];
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  const long plane = WAVES == 1 ? (long)blockIdx.x * 4 + wave : (long)blockIdx.x;
  float acc[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) acc[e] = 0.f;
  if (plane < p.planes) {
    const u16* up = p.u + (size_t)plane * p.HW;
    const u16* zp = DOT ? p.dz + (size_t)plane * p.HW : nullptr;
    const int lo = WAVES == 1 ? 0 : wave * p.chunk;
    const int hi = WAVES == 1 ? p.HW : min(p.HW, lo + p.chunk);
    for (int i0 = lo + lane * 8; i0 < hi; i0 += 512) {
      float v[8];
      se_load8<DT>(up, i0, p.HW, v);
      if (DOT) {
        float d[8];
        se_load8<DT>(zp, i0, p.HW, d);
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] = fmaf(d[e], se_silu(v[e]), acc[e]);
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] += se_silu(v[e]);  // (silu(0) = 0: the elements past the plane add nothing)
      }
    }
  }
  float s = ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]));
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) s += __shfl_xor(s, d);
  if (WAVES == 1) {
    if (lane == 0 && plane < p.planes) p.out[plane] = DOT ? s : s * p.inv;
  } else {
    if (lane == 0) part[wave] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
      const float t = ((part[0] + part[1]) + part[2]) + part[3];
      p.out[plane] = DOT ? t : t * p.inv;
    }
  }
}

struct SeGateParams {
  const float* pooled;  // [N][C]
  const float* w1;      // [Cr][C]
  const float* b1;
  const float* w2;      // [C][Cr]
  const float* b2;
  float* hidden_pre;    // [N][Cr]
  float* gate;          // [N][C]
  const float* dgate_raw;
  float* dpool;
  float* ws_dv2;        // [N][C]
  float* ws_s;          // [N][Cr]
  float* ws_dh;         // [N][Cr]
  float* dw1;
  float* db1;
  float* dw2;
  float* db2;
  int N, C, R;
};

__global__ __launch_bounds__(256) void se_gate_kernel(const SeGateParams p) {
  __shared__ float mean[kSeMaxC];
  __shared__ float sq[kSeMaxR];
  const int tid = (int)threadIdx.x, n = (int)blockIdx.x;
  const int q = tid >> 6, cl = tid & 63;
  for (int c = tid; c < p.C; c += 256) mean[c] = p.pooled[(size_t)n * p.C + c];
  __syncthreads();
  for (int r = q; r < p.R; r += 4) {
    const float* w = p.w1 + (size_t)r * p.C;
    float s = 0.f;
    for (int c = cl; c < p.C; c += 64) s = fmaf(w[c], mean[c], s);
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) s += __shfl_xor(s, d);
    if (cl == 0) {
      const float v = s + p.b1[r];
      p.hidden_pre[(size_t)n * p.R + r] = v;
      sq[r] = se_silu(v);
    }
  }
  __syncthreads();
  for (int c = tid; c < p.C; c += 256) {
    const float* w = p.w2 + (size_t)c * p.R;
    float s = 0.f;
    for (int r = 0; r < p.R; ++r) s = fmaf(w[r], sq[r], s);
    p.gate[(size_t)n * p.C + c] = se_sigmoid(s + p.b2[c]);
  }
}

__global__ __launch_bounds__(256) void se_gate_bwd_kernel(const SeGateParams p) {
  __shared__ float dv2[kSeMaxC];
  __shared__ float dh[kSeMaxR];
  const int tid = (int)threadIdx.x, n = (int)blockIdx.x;
  const int q = tid >> 6, cl = tid & 63;
  for (int c = tid; c < p.C; c += 256) {
    const float g = p.gate[(size_t)n * p.C + c];
    const float v = (p.dgate_raw[(size_t)n * p.C + c] * g) * (1.0f - g);
    dv2[c] = v;
    p.ws_dv2[(size_t)n * p.C + c] = v;
  }
  __syncthreads();
  for (int r = q; r < p.R; r += 4) {
    float s = 0.f;
    for (int c = cl; c < p.C; c += 64) s = fmaf(p.w2[(size_t)c * p.R + r], dv2[c], s);
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) s += __shfl_xor(s, d);
    if (cl == 0) {
      const float hp = p.hidden_pre[(size_t)n * p.R + r];
      const float v = s * se_dsilu(hp);
      dh[r] = v;
      p.ws_dh[(size_t)n * p.R + r] = v;
      p.ws_s[(size_t)n * p.R + r] = se_silu(hp);
    }
  }
  __syncthreads();
  for (int c = tid; c < p.C; c += 256) {
    float s = 0.f;
    for (int r = 0; r < p.R; ++r) s = fmaf(p.w1[(size_t)r * p.C + c], dh[r], s);
    p.dpool[(size_t)n * p.C + c] = s;
  }
}

// one thread per element of dW2 [C][R], dW1 [R][C], db2 [C], db1 [R] (in that order of the flat index); images in order
__global__ __launch_bounds__(256) void se_param_grad_kernel(const SeGateParams p) {
  const long cr = (long)p.C * p.R;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= 2 * cr + p.C + p.R) return;
  float s = 0.f;
  if (i < cr) {
    const int c = (int)(i / p.R), r = (int)(i - (long)c * p.R);
    for (int n = 0; n < p.N; ++n) s = fmaf(p.ws_dv2[(size_t)n * p.C + c], p.ws_s[(size_t)n * p.R + r], s);
    p.dw2[i] = s;
  } else if (i < 2 * cr) {
    const long k = i - cr;
    const int r = (int)(k / p.C), c = (int)(k - (long)r * p.C);
    for (int n = 0; n < p.N; ++n) s = fmaf(p.ws_dh[(size_t)n * p.R + r], p.pooled[(size_t)n * p.C + c], s);
    p.dw1[k] = s;
  } else if (i < 2 * cr + p.C) {
    const int c = (int)(i - 2 * cr);
    for (int n = 0; n < p.N; ++n) s += p.ws_dv2[(size_t)n * p.C + c];
    p.db2[c] = s;
  } else {
    const int r = (int)(i - 2 * cr - p.C);
    for (int n = 0; n < p.N; ++n) s += p.ws_dh[(size_t)n * p.R + r];
    p.db1[r] = s;
  }
}

struct SeElemParams {
  const u16* u;
  const u16* dz;
  const float* gate;   // [planes]
  const float* dpool;  // [planes]
  u16* out;
  size_t total;        // elements
  int HW;
  float inv;
};

// flat octets over the tensor; BWD = false: z = silu(u) g; true: du = (dz g + dpool / HW) silu'(u)
template <int DT, bool BWD>
__global__ __launch_bounds__(256) void se_elem_kernel(const SeElemParams p) {
  const size_t e0 = ((size_t)blockIdx.x * 256 + threadIdx.x) * 8;
  if (e0 >= p.total) return;
  const bool vec = e0 + 8 <= p.total && (((uintptr_t)p.u | (uintptr_t)p.out | (BWD ? (uintptr_t)p.dz : 0)) & 15u) == 0;
  float v[8], d[8];
  if (vec) {
    const u32x4 r = *reinterpret_cast<const u32x4*>(p.u + e0);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      v[2 * e] = bits16_to_f32<DT>(r[e] & 0xffffu);
      v[2 * e + 1] = bits16_to_f32<DT>(r[e] >> 16);
    }
    if (BWD) {
      const u32x4 s = *reinterpret_cast<const u32x4*>(p.dz + e0);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        d[2 * e] = bits16_to_f32<DT>(s[e] & 0xffffu);
        d[2 * e + 1] = bits16_to_f32<DT>(s[e] >> 16);
      }
    }
  } else {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const bool ok = e0 + e < p.total;
      v[e] = ok ? bits16_to_f32<DT>(p.u[e0 + e]) : 0.f;
      if (BWD) d[e] = ok ? bits16_to_f32<DT>(p.dz[e0 + e]) : 0.f;
    }
  }
  size_t plane = e0 / (size_t)p.HW;
  int rem = (int)(e0 - plane * (size_t)p.HW);
  float o[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    if (e0 + e < p.total) {
      const float g = p.gate[plane];
      if (BWD) o[e] = fmaf(d[e], g, p.dpool[plane] * p.inv) * se_dsilu(v[e]);
      else o[e] = se_silu(v[e]) * g;
    } else {
      o[e] = 0.f;
    }
    if (++rem == p.HW) {
      rem = 0;
      ++plane;
    }
  }
  if (vec) {
    u32x4 w;
#pragma unroll
    for (int e = 0; e < 4; ++e) w[e] = pack2_16<DT>(o[2 * e], o[2 * e + 1]);
    *reinterpret_cast<u32x4*>(p.out + e0) = w;
  } else {
#pragma unroll
    for (int e = 0; e < 8; ++e)
      if (e0 + e < p.total) p.out[e0 + e] = (u16)dw5_round16<DT>(o[e]);
  }
}

// ---- host -----------------------------------------------------------------------------------------------------------------------
static bool dw5_args(const char* what, int N, int C, int H, int W, int stride, int dtype, bool quiet = false) {
  const bool ok = N > 0 && C > 0 && H > 0 && W > 0 && (stride == 1 || stride == 2) && (dtype == SSDK_BF16 || dtype == SSDK_F16) &&
                  (long)N * C < (1L << 31) && (long)H * W < (1L << 30);
  if (!ok && !quiet)
    set_error("%s: N, C, H, W > 0, stride 1 | 2 and bf16 | f16 expected (got N=%d C=%d H=%d W=%d stride=%d dtype=%d)", what, N, C, H, W,
              stride, dtype);
  return ok;
}

// kind 0: forward / weight gradient (units in the OUTPUT plane oh x ow, stride S staging); 1: stride-2 input gradient (units in dx)
static Dw5Plan dw5_plan(int kind, int oh, int ow, int S, long planes) {
  Dw5Plan pl;
  const int upr = (ow + 7) / 8;
  pl.TCu = upr <= 32 ? upr : 32;
  pl.ctiles = (upr + pl.TCu - 1) / pl.TCu;
  pl.TR = 256 / pl.TCu;
  if (pl.TR > oh) pl.TR = oh;
  for (;;) {
    if (kind == 1 && pl.TR < oh && (pl.TR & 1)) --pl.TR;  // bands of the stride-2 input gradient start on even rows
    if (pl.TR < 1) pl.TR = 1;
    pl.IR = kind == 0 ? (pl.TR - 1) * S + 5 : (pl.TR + 1) / 2 + 2;
    pl.IC = kind == 0 ? (pl.TCu * 8 - 1) * S + 5 : pl.TCu * 4 + 2;
    if ((long)pl.IR * pl.IC <= kDw5Lds || pl.TR <= 2) break;
    --pl.TR;
  }
  pl.bands = (oh + pl.TR - 1) / pl.TR;
  pl.G = 1;
  if (pl.bands == 1 && pl.ctiles == 1) {
    long g = 256 / (pl.TR * pl.TCu);
    const long fit = kDw5Lds / ((long)pl.IR * pl.IC);
    if (g > fit) g = fit;
    if (g > kDw5MaxG) g = kDw5MaxG;
    if (g > planes) g = planes;
    if (g < 1) g = 1;
    pl.G = (int)g;
  }
  pl.groups = (int)((planes + pl.G - 1) / pl.G);
  return pl;
}

static bool dw5_grid_ok(const char* what, long blocks) {
  if (blocks <= 0 || blocks >= (1L << 31)) {
    set_error("%s: too many workgroups", what);
    return false;
  }
  return true;
}

static long dw5_wgrad_parts(int N, int H, int W, int stride, Dw5Plan* out) {
  const int ho = (H - 1) / stride + 1, wo = (W - 1) / stride + 1;
  const Dw5Plan pl = dw5_plan(0, ho, wo, stride, N);
  if (out) *out = pl;
  return (long)pl.groups * pl.bands * pl.ctiles;
}

}  // namespace ssdk

using namespace ssdk;

extern "C" size_t ssdk_dwconv5_bwd_weight_workspace_bytes(int N, int C, int H, int W, int stride) {
  if (!dw5_args("dwconv5_bwd_weight_workspace_bytes", N, C, H, W, stride, SSDK_BF16, true)) return 0;
  return (size_t)dw5_wgrad_parts(N, H, W, stride, nullptr) * 25 * (size_t)C * sizeof(float);
}

extern "C" int ssdk_dwconv5_fwd(const void* x, const void* w, void* y, int N, int C, int H, int W, int stride, int dtype, void* stream) {
  if (!dw5_args("dwconv5_fwd", N, C, H, W, stride, dtype)) return SSDK_E_BADARG;
  if (!x || !w || !y) {
    set_error("dwconv5_fwd: null pointer");
    return SSDK_E_BADARG;
  }
  Dw5Params p = {};
  p.src = (const u16*)x, p.w = (const u16*)w, p.dst = (u16*)y;
  p.N = N, p.C = C, p.Hs = H, p.Ws = W, p.Hd = (H - 1) / stride + 1, p.Wd = (W - 1) / stride + 1;
  p.pl = dw5_plan(0, p.Hd, p.Wd, stride, (long)N * C);
  const long blocks = (long)p.pl.groups * p.pl.bands * p.pl.ctiles;
  if (!dw5_grid_ok("dwconv5_fwd", blocks)) return SSDK_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)blocks);
  if (dtype == SSDK_BF16) {
    if (stride == 1) hipLaunchKernelGGL((dw5_fwd_kernel<SSDK_BF16, 1>), grid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL((dw5_fwd_kernel<SSDK_BF16, 2>), grid, dim3(256), 0, st, p);
  } else {
    if (stride == 1) hipLaunchKernelGGL((dw5_fwd_kernel<SSDK_F16, 1>), grid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL((dw5_fwd_kernel<SSDK_F16, 2>), grid, dim3(256), 0, st, p);
  }
  return check_launch("dw5_fwd_kernel");
}

extern "C" int ssdk_dwconv5_bwd_data(const void* dy, const void* w, void* dx, int N, int C, int H, int W, int stride, int dtype,
                                     void* stream) {
  if (!dw5_args("dwconv5_bwd_data", N, C, H, W, stride, dtype)) return SSDK_E_BADARG;
  if (!dy || !w || !dx) {
    set_error("dwconv5_bwd_data: null pointer");
    return SSDK_E_BADARG;
  }
  Dw5Params p = {};
  p.src = (const u16*)dy, p.w = (const u16*)w, p.dst = (u16*)dx;
  p.N = N, p.C = C, p.Hs = (H - 1) / stride + 1, p.Ws = (W - 1) / stride + 1, p.Hd = H, p.Wd = W;
  hipStream_t st = (hipStream_t)stream;
  if (stride == 1) {  // the forward kernel on dy with the window reversed
    p.flip = 1;
    p.pl = dw5_plan(0, H, W, 1, (long)N * C);
    const long blocks = (long)p.pl.groups * p.pl.bands * p.pl.ctiles;
    if (!dw5_grid_ok("dwconv5_bwd_data", blocks)) return SSDK_E_BADARG;
    if (dtype == SSDK_BF16) hipLaunchKernelGGL((dw5_fwd_kernel<SSDK_BF16, 1>), dim3((unsigned)blocks), dim3(256), 0, st, p);
    else hipLaunchKernelGGL((dw5_fwd_kernel<SSDK_F16, 1>), dim3((unsigned)blocks), dim3(256), 0, st, p);
    return check_launch("dw5_fwd_kernel");
  }
  p.pl = dw5_plan(1, H, W, 2, (long)N * C);
  const long blocks = (long)p.pl.groups * p.pl.bands * p.pl.ctiles;
  if (!dw5_grid_ok("dwconv5_bwd_data", blocks)) return SSDK_E_BADARG;
  if (dtype == SSDK_BF16) hipLaunchKernelGGL((dw5_dgrad2_kernel<SSDK_BF16>), dim3((unsigned)blocks), dim3(256), 0, st, p);
  else hipLaunchKernelGGL((dw5_dgrad2_kernel<SSDK_F16>), dim3((unsigned)blocks), dim3(256), 0, st, p);
  return check_launch("dw5_dgrad2_kernel");
}

extern "C" int ssdk_dwconv5_bwd_weight(const void* x, const void* dy, float* dw, void* workspace, size_t workspace_bytes, int N, int C,
                                       int H, int W, int stride, int dtype, void* stream) {
  if (!dw5_args("dwconv5_bwd_weight", N, C, H, W, stride, dtype)) return SSDK_E_BADARG;
  if (!x || !dy || !dw || !workspace || ((uintptr_t)workspace & 3u) ||
      workspace_bytes < ssdk_dwconv5_bwd_weight_workspace_bytes(N, C, H, W, stride)) {
    set_error("dwconv5_bwd_weight: null pointer, or workspace too small / misaligned");
    return SSDK_E_BADARG;
  }
  Dw5Params p = {};
  p.src = (const u16*)x, p.dy = (const u16*)dy, p.dw = dw, p.ws = (float*)workspace;
  p.N = N, p.C = C, p.Hs = H, p.Ws = W, p.Hd = (H - 1) / stride + 1, p.Wd = (W - 1) / stride + 1;
  p.parts = (int)dw5_wgrad_parts(N, H, W, stride, &p.pl);
  const long blocks = (long)C * p.parts;
  if (!dw5_grid_ok("dwconv5_bwd_weight", blocks)) return SSDK_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)blocks);
  if (dtype == SSDK_BF16) {
    if (stride == 1) hipLaunchKernelGGL((dw5_wgrad_kernel<SSDK_BF16, 1>), grid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL((dw5_wgrad_kernel<SSDK_BF16, 2>), grid, dim3(256), 0, st, p);
  } else {
    if (stride == 1) hipLaunchKernelGGL((dw5_wgrad_kernel<SSDK_F16, 1>), grid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL((dw5_wgrad_kernel<SSDK_F16, 2>), grid, dim3(256), 0, st, p);
  }
  const int rows = C * 25;
  hipLaunchKernelGGL(dw5_wgrad_reduce_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, (const float*)p.ws, dw, rows, p.parts);
  return check_launch("dw5_wgrad_kernel");
}

static bool se_args(const char* what, int N, int C, int H, int W, int dtype) {
  const bool ok = N > 0 && C > 0 && H > 0 && W > 0 && (dtype == SSDK_BF16 || dtype == SSDK_F16) && (long)N * C < (1L << 31) &&
                  (long)H * W < (1L << 30);
  if (!ok) set_error("%s: N, C, H, W > 0 and bf16 | f16 expected (got N=%d C=%d H=%d W=%d dtype=%d)", what, N, C, H, W, dtype);
  return ok;
}

static bool se_gate_args(const char* what, int N, int C, int Cr, bool quiet = false) {
  const bool ok = N > 0 && C > 0 && Cr > 0 && C <= kSeMaxC && Cr <= kSeMaxR;
  if (!ok && !quiet) set_error("%s: N > 0, 0 < C <= %d, 0 < Cr <= %d expected (got N=%d C=%d Cr=%d)", what, kSeMaxC, kSeMaxR, N, C, Cr);
  return ok;
}

template <bool DOT>
static void se_sum_launch(const SeSumParams& p, int dtype, hipStream_t st) {
  if (p.HW < kSeWgPlane) {
    const dim3 grid((unsigned)((p.planes + 3) / 4));
    if (dtype == SSDK_BF16) hipLaunchKernelGGL((se_sum_kernel<SSDK_BF16, 1, DOT>), grid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL((se_sum_kernel<SSDK_F16, 1, DOT>), grid, dim3(256), 0, st, p);
  } else {
    const dim3 grid((unsigned)p.planes);
    if (dtype == SSDK_BF16) hipLaunchKernelGGL((se_sum_kernel<SSDK_BF16, 4, DOT>), grid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL((se_sum_kernel<SSDK_F16, 4, DOT>), grid, dim3(256), 0, st, p);
  }
}

static SeSumParams se_sum_params(const void* u, const void* dz, float* out, int N, int C, int H, int W) {
  SeSumParams p = {};
  p.u = (const u16*)u, p.dz = (const u16*)dz, p.out = out;
  p.planes = (long)N * C;
  p.HW = H * W;
  p.chunk = ((p.HW + 3) / 4 + 7) / 8 * 8;
  p.inv = 1.0f / (float)p.HW;
  return p;
}

extern "C" int ssdk_se_pool_fwd(const void* u, float* pooled, int N, int C, int H, int W, int dtype, void* stream) {
  if (!se_args("se_pool_fwd", N, C, H, W, dtype)) return SSDK_E_BADARG;
  if (!u || !pooled) {
    set_error("se_pool_fwd: null pointer");
    return SSDK_E_BADARG;
  }
  se_sum_launch<false>(se_sum_params(u, nullptr, pooled, N, C, H, W), dtype, (hipStream_t)stream);
  return check_launch("se_sum_kernel");
}

extern "C" int ssdk_se_bwd_reduce(const void* u, const void* dz, float* dgate_raw, int N, int C, int H, int W, int dtype, void* stream) {
  if (!se_args("se_bwd_reduce", N, C, H, W, dtype)) return SSDK_E_BADARG;
  if (!u || !dz || !dgate_raw) {
    set_error("se_bwd_reduce: null pointer");
    return SSDK_E_BADARG;
  }
  se_sum_launch<true>(se_sum_params(u, dz, dgate_raw, N, C, H, W), dtype, (hipStream_t)stream);
  return check_launch("se_sum_kernel");
}

extern "C" int ssdk_se_gate_fwd(const float* pooled, const float* w1, const float* b1, const float* w2, const float* b2, float* hidden_pre,
                                float* gate, int N, int C, int Cr, void* stream) {
  if (!se_gate_args("se_gate_fwd", N, C, Cr)) return SSDK_E_BADARG;
  if (!pooled || !w1 || !b1 || !w2 || !b2 || !hidden_pre || !gate) {
    set_error("se_gate_fwd: null pointer");
    return SSDK_E_BADARG;
  }
  SeGateParams p = {};
  p.pooled = pooled, p.w1 = w1, p.b1 = b1, p.w2 = w2, p.b2 = b2, p.hidden_pre = hidden_pre, p.gate = gate;
  p.N = N, p.C = C, p.R = Cr;
  hipLaunchKernelGGL(se_gate_kernel, dim3((unsigned)N), dim3(256), 0, (hipStream_t)stream, p);
  return check_launch("se_gate_kernel");
}

extern "C" size_t ssdk_se_gate_bwd_workspace_bytes(int N, int C, int Cr) {
  if (!se_gate_args("se_gate_bwd_workspace_bytes", N, C, Cr, true)) return 0;
  return ((size_t)N * C + 2 * (size_t)N * Cr) * sizeof(float);
}

extern "C" int ssdk_se_gate_bwd(const float* dgate_raw, const float* gate, const float* pooled, const float* hidden_pre, const float* w1,
                                const float* w2, float* dpool, float* dw1, float* db1, float* dw2, float* db2, void* workspace,
                                size_t workspace_bytes, int N, int C, int Cr, void* stream) {
  if (!se_gate_args("se_gate_bwd", N, C, Cr)) return SSDK_E_BADARG;
  if (!dgate_raw || !gate || !pooled || !hidden_pre || !w1 || !w2 || !dpool || !dw1 || !db1 || !dw2 || !db2 || !workspace ||
      ((uintptr_t)workspace & 3u) || workspace_bytes < ssdk_se_gate_bwd_workspace_bytes(N, C, Cr)) {
    set_error("se_gate_bwd: null pointer, or workspace too small / misaligned");
    return SSDK_E_BADARG;
  }
  SeGateParams p = {};
  p.dgate_raw = dgate_raw, p.gate = const_cast<float*>(gate), p.pooled = pooled, p.hidden_pre = const_cast<float*>(hidden_pre), p.w1 = w1, p.w2 = w2;
  p.dpool = dpool, p.dw1 = dw1, p.db1 = db1, p.dw2 = dw2, p.db2 = db2;
  p.ws_dv2 = (float*)workspace;
  p.ws_s = p.ws_dv2 + (size_t)N * C;
  p.ws_dh = p.ws_s + (size_t)N * Cr;
  p.N = N, p.C = C, p.R = Cr;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(se_gate_bwd_kernel, dim3((unsigned)N), dim3(256), 0, st, p);
  const long elems = 2L * C * Cr + C + Cr;
  hipLaunchKernelGGL(se_param_grad_kernel, dim3((unsigned)((elems + 255) / 256)), dim3(256), 0, st, p);
  return check_launch("se_gate_bwd_kernel");
}

static int se_elem(const char* what, bool bwd, const void* u, const void* dz, const float* gate, const float* dpool, void* out, int N, int C,
                   int H, int W, int dtype, void* stream) {
  if (!se_args(what, N, C, H, W, dtype)) return SSDK_E_BADARG;
  if (!u || !gate || !out || (bwd && (!dz || !dpool))) {
    set_error("%s: null pointer", what);
    return SSDK_E_BADARG;
  }
  SeElemParams p = {};
  p.u = (const u16*)u, p.dz = (const u16*)dz, p.gate = gate, p.dpool = dpool, p.out = (u16*)out;
  p.HW = H * W;
  p.total = (size_t)N * C * (size_t)p.HW;
  p.inv = 1.0f / (float)p.HW;
  const size_t blocks = (p.total + 2047) / 2048;
  if (blocks >= ((size_t)1 << 31)) {
    set_error("%s: too many workgroups", what);
    return SSDK_E_BADARG;
  }
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)blocks);
  if (dtype == SSDK_BF16) {
    if (bwd) hipLaunchKernelGGL((se_elem_kernel<SSDK_BF16, true>), grid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL((se_elem_kernel<SSDK_BF16, false>), grid, dim3(256), 0, st, p);
  } else {
    if (bwd) hipLaunchKernelGGL((se_elem_kernel<SSDK_F16, true>), grid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL((se_elem_kernel<SSDK_F16, false>), grid, dim3(256), 0, st, p);
  }
  return check_launch("se_elem_kernel");
}

extern "C" int ssdk_se_scale_fwd(const void* u, const float* gate, void* z, int N, int C, int H, int W, int dtype, void* stream) {
  return se_elem("se_scale_fwd", false, u, nullptr, gate, nullptr, z, N, C, H, W, dtype, stream);
}

extern "C" int ssdk_se_bwd_apply(const void* u, const void* dz, const float* gate, const float* dpool, void* du, int N, int C, int H, int W,
                                 int dtype, void* stream) {
  return se_elem("se_bwd_apply", true, u, dz, gate, dpool, du, N, C, H, W, dtype, stream);
}

