// ssdk_pwtrain_kernels.h -- device code and launch geometry of the 1x1 training kernels, shared by ssdk_pwtrain.hip (contiguous
// tensors, K a multiple of 8) and ssdk_shuffletrain.hip (channel slices, any K and M >= 8): see ssdk_pwtrain.hip for the scheme.
#pragma once
#include "ssdk_conv_common.h"

namespace ssdk {

typedef u32x4 pw_u32x4_a2 __attribute__((aligned(2)));
constexpr int PWT_THREADS = 256;
constexpr int PWT_KC = 8;  // k-steps (of 32 channels) of weights staged per chunk in the long-K kernel

struct PwtParams {
  const u16* x;       // [B, K, HW]
  const u16* a;       // [M, K] row-major, 16 bit
  const float* bias;  // [M] or null
  u16* y;             // [B, M, HW]
  int B, K, M, HW;
  int KS;             // ceil(K / 32)
  int nf;             // output fragments (16 rows) per workgroup slice
  u32 gpi;            // 128-pixel groups per image
  u32 groups;         // B * gpi
  u32 wg_iters;       // (P) iterations of a workgroup (4 groups each)
  float* stats;       // optional [gridDim.x * 4 waves][M][2]: per wave (sum y, sum y^2) of its outputs (fp32, before the store's rounding)
  // SL kernels only (channel slices, ssdk_shuffletrain.hip): elements between two images of x / of y, leading dimension of a
  size_t xs, ys;
  u32 lda;
  // AF kernels only (ssdk_densetrain.hip): coef [K][4] = (a, b, ., .) of the operand transform, byte offset of its LDS copy
  const float* coef;
  u32 cf_off;
};

// 8 consecutive 16-bit elements at p (any 2-byte alignment); lanes with nvalid < 8 read element by element and zero-fill
template <bool TAIL>
__device__ __forceinline__ u32x4 pw_load8(const u16* p, int nvalid) {
  if constexpr (!TAIL) {
    return *reinterpret_cast<const pw_u32x4_a2*>(p);
  } else {
    if (nvalid >= 8) return *reinterpret_cast<const pw_u32x4_a2*>(p);
    u32 h[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) h[e] = e < nvalid ? (u32)p[e] : 0u;
    return u32x4{h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16)};
  }
}
template <bool TAIL>
__device__ __forceinline__ void pw_store8(u16* p, const u32x4 v, int nvalid) {
  if constexpr (!TAIL) {
    *reinterpret_cast<pw_u32x4_a2*>(p) = v;
  } else {
    if (nvalid >= 8) {
      *reinterpret_cast<pw_u32x4_a2*>(p) = v;
      return;
    }
#pragma unroll
    for (int e = 0; e < 8; ++e)
      if (e < nvalid) p[e] = (u16)((e & 1) ? (v[e >> 1] >> 16) : (v[e >> 1] & 0xffffu));
  }
}

// raw[j] = 8 pixels of channel j of the lane's 8 channels  ->  bop[t] = the 8 channels of pixel t (MFMA B operand of pixel set t)
__device__ __forceinline__ void pw_transpose8(const u32x4 (&raw)[8], u32x4 (&bop)[8]) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
#pragma unroll
    for (int h = 0; h < 4; ++h) {
      const u32 lo = raw[2 * q][h], hi = raw[2 * q + 1][h];
      bop[2 * h][q] = __builtin_amdgcn_perm(hi, lo, 0x05040100u);      // low halves: pixel 2h of channels 2q, 2q + 1
      bop[2 * h + 1][q] = __builtin_amdgcn_perm(hi, lo, 0x07060302u);  // high halves: pixel 2h + 1
    }
  }
}

// AF: the operand transform of a dense layer's first 1x1 (ssdk_densetrain.hip): op(x) = round_DT(max(fmaf(a, x, b), 0)) with the
// channel's (a, b) of the deferred BatchNorm -- what its apply pass would have stored, formed while the operand is staged.
// Elements >= nvalid (outside the plane) become zero, not max(b, 0): the weight gradient contracts over pixels.
template <int DT>
__device__ __forceinline__ u32x4 pw_affine8(const u32x4 v, float a, float b, int nvalid) {
  u32x4 o;
#pragma unroll
  for (int h = 0; h < 4; ++h) {
    float lo = fmaxf(__builtin_fmaf(a, bits16_to_f32<DT>(v[h] & 0xffffu), b), 0.f);
    float hi = fmaxf(__builtin_fmaf(a, bits16_to_f32<DT>(v[h] >> 16), b), 0.f);
    if (2 * h >= nvalid) lo = 0.f;
    if (2 * h + 1 >= nvalid) hi = 0.f;
    o[h] = pack2_16<DT>(lo, hi);
  }
  return o;
}
// ... of a lane's 8 x 8 block: cf = the LDS copy [32 KS][2] of (a, b), at the block's first channel (zeros for channels >= K)
template <int DT>
__device__ __forceinline__ void pw_affine_raw(u32x4 (&raw)[8], const float* cf, int nvalid) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const f32x4 ab = *reinterpret_cast<const f32x4*>(cf + 4 * q);  // channels 2q, 2q + 1: a lane group reads one address
    raw[2 * q] = pw_affine8<DT>(raw[2 * q], ab[0], ab[1], nvalid);
    raw[2 * q + 1] = pw_affine8<DT>(raw[2 * q + 1], ab[2], ab[3], nvalid);
  }
}
// coef [K][4] -> its LDS copy [32 KS][2] (the caller's barrier behind it)
__device__ __forceinline__ void pw_stage_coef(float* cf, const float* coef, u32 K, u32 KS, u32 tid) {
  for (u32 c = tid; c < KS * 32u; c += PWT_THREADS) {
    cf[2u * c] = c < K ? coef[4u * c] : 0.f;
    cf[2u * c + 1u] = c < K ? coef[4u * c + 1u] : 0.f;
  }
}

// the lane's 8 x 8 block of k-step ks: channels 32 ks + 8 fg + (0..7), pixels px .. px + 7 of image base xb
// KT (any K): a channel >= K is NEVER loaded -- in a slice it is the next image's, behind the last image it is outside the allocation
template <bool TAIL, bool KT = false>
__device__ __forceinline__ void pw_load_raw(const u16* xb, u32 HW, u32 K, u32 chan0, int nvalid, u32x4 (&raw)[8]) {
  if (chan0 < K) {  // (!KT: K is a multiple of 8, all eight channels or none)
    const u16* p = xb + (size_t)chan0 * HW;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (!KT || chan0 + (u32)j < K) raw[j] = pw_load8<TAIL>(p + (size_t)j * HW, nvalid);
      else raw[j] = u32x4{0u, 0u, 0u, 0u};
    }
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) raw[j] = u32x4{0u, 0u, 0u, 0u};
  }
}

// A fragment (f, ks) of the slice: lane (fr, fg) holds a[m0 + 16 f + fr][32 ks + 8 fg .. + 7], zero outside the matrix
// KT: rows of lda >= K elements (lda a multiple of 8); the elements K .. of the last 8-group count as zero whatever they hold
template <bool KT = false>
__device__ __forceinline__ void pw_stage_a(unsigned char* lds, const u16* a, u32 M, u32 K, u32 lda, u32 m0, u32 nf, u32 ks0, u32 nks,
                                           u32 tid) {
  for (u32 i = tid; i < nf * nks * 64u; i += PWT_THREADS) {
    const u32 l = i & 63u, fk = i >> 6, ks = fk % nks, f = fk / nks;
    const u32 row = m0 + 16u * f + (l & 15u), k0 = (ks0 + ks) * 32u + (l >> 4) * 8u;
    u32x4 v = {0u, 0u, 0u, 0u};
    if (row < M && k0 < K) {
      v = *reinterpret_cast<const u32x4*>(a + (size_t)row * lda + k0);
      if constexpr (KT) {
        const u32 nk = K - k0;  // elements of the group inside the matrix
        if (nk < 8u) {
#pragma unroll
          for (u32 w = 0; w < 4u; ++w) v[w] = 2u * w >= nk ? 0u : (2u * w + 1u >= nk ? (v[w] & 0xffffu) : v[w]);
        }
      }
    }
    *reinterpret_cast<u32x4*>(lds + (size_t)i * 16u) = v;
  }
}

// (sum, sum of squares) of row i of the fragment over the lane's 8 pixels that lie inside the plane -- of the fp32 accumulators,
// BEFORE the rounding of the store: the statistics of a BatchNorm over 10^5 ... 10^6 elements do not see 2^-9 of zero-mean
// rounding per element, and unpacking the stored words cost as much as the reduction pass it was meant to save (round 6, first
// version: forward + statistics 1 517 vs 1 088 us per step)
__device__ __forceinline__ void pw_row_moments(const f32x4 (&acc)[8], int i, int nvalid, float& s1, float& s2) {
#pragma unroll
  for (int t = 0; t < 8; ++t) {
    const float v = t < nvalid ? acc[t][i] : 0.f;
    s1 += v;
    s2 += v * v;
  }
}
// sum over the 16 lanes fr of a lane group (all four groups at once)
__device__ __forceinline__ float pw_sum16(float v) {
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// finished accumulators of fragment f (rows 4 fg + i of it, pixels 8 fr + t) -> four 16-byte stores
// STATS: m1[i] / m2[i] += the lane's share of (sum, sum of squares) of row i, over the pixels inside the plane
template <int DT, bool TAIL, bool STATS = false>
__device__ __forceinline__ void pw_store_frag(const f32x4 (&acc)[8], u16* yb, u32 HW, u32 M, u32 row0, int nvalid, float* m1 = nullptr,
                                              float* m2 = nullptr) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (row0 + (u32)i < M) {
      const u32x4 o = {pack2_16<DT>(acc[0][i], acc[1][i]), pack2_16<DT>(acc[2][i], acc[3][i]),
                       pack2_16<DT>(acc[4][i], acc[5][i]), pack2_16<DT>(acc[6][i], acc[7][i])};
      pw_store8<TAIL>(yb + (size_t)(row0 + (u32)i) * HW, o, nvalid);
      if constexpr (STATS) pw_row_moments(acc, i, TAIL ? nvalid : 8, m1[i], m2[i]);
    }
  }
}

// ---- (E) short K (<= 96 channels): the B operands of a 128-pixel group stay in registers, the wave walks over ALL output
// fragments of the slice.  Expansion layers (16 -> 96 ... 96 -> 576) and the input gradients of the projections. ---------------
// SL: x and y are channel slices (own image strides), a has a leading dimension, K and M are any values >= 8
// AF: the operand is op(x) (pw_affine8), coefficients in LDS behind the fragments
template <int DT, int KS, bool STATS = false, bool SL = false, bool AF = false>
__global__ __launch_bounds__(PWT_THREADS) void pw_gemm_short_kernel(const PwtParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const u32 tid = threadIdx.x, lane = tid & 63u;
  const u32 wave = (u32)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
  const u32 fr = lane & 15u, fg = lane >> 4;
  const u32 M = (u32)p.M, K = (u32)p.K, HW = (u32)p.HW;
  const u32 m0 = blockIdx.y * (u32)(16 * p.nf);
  const u32 nf = min((u32)p.nf, (M - m0 + 15u) / 16u);
  pw_stage_a<SL>(smem, p.a, M, K, SL ? p.lda : K, m0, nf, 0u, (u32)KS, tid);
  // STATS: this wave's (sum, sum of squares) per output row of the slice, behind the A fragments: [nf * 16 rows][2]
  float* wst = reinterpret_cast<float*>(smem + (size_t)p.nf * KS * 1024) + (size_t)wave * (u32)p.nf * 32u;
  if constexpr (STATS) {
    for (u32 i = lane; i < (u32)p.nf * 32u; i += 64u) wst[i] = 0.f;
  }
  const float* cf = reinterpret_cast<const float*>(smem + p.cf_off);
  if constexpr (AF) pw_stage_coef(reinterpret_cast<float*>(smem + p.cf_off), p.coef, K, (u32)KS, tid);
  __syncthreads();
  const u32 gstride = gridDim.x * 4u;
  for (u32 g = blockIdx.x * 4u + wave; g < p.groups; g += gstride) {
    const u32 b = g / p.gpi, p0 = (g - b * p.gpi) * 128u + 8u * fr;
    const bool tail = (g - b * p.gpi) * 128u + 128u > HW;  // wave-uniform
    const int nvalid = (int)HW - (int)p0;
    const u16* xb = p.x + (SL ? (size_t)b * p.xs : (size_t)b * K * HW) + p0;
    u16* yb = p.y + (SL ? (size_t)b * p.ys : (size_t)b * M * HW) + p0;
    u32x4 bop[KS][8];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      u32x4 raw[8];
      if (tail) pw_load_raw<true, SL>(xb, HW, K, (u32)ks * 32u + fg * 8u, nvalid, raw);
      else pw_load_raw<false, SL>(xb, HW, K, (u32)ks * 32u + fg * 8u, 8, raw);
      if constexpr (AF) pw_affine_raw<DT>(raw, cf + 2u * ((u32)ks * 32u + fg * 8u), tail ? nvalid : 8);
      pw_transpose8(raw, bop[ks]);
    }
    for (u32 f = 0; f < nf; ++f) {
      f32x4 acc[8];
      const u32 row0 = m0 + 16u * f + 4u * fg;
      f32x4 init = {0.f, 0.f, 0.f, 0.f};
      if (p.bias) {
#pragma unroll
        for (int i = 0; i < 4; ++i) init[i] = row0 + (u32)i < M ? p.bias[row0 + (u32)i] : 0.f;
      }
#pragma unroll
      for (int t = 0; t < 8; ++t) acc[t] = init;
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        const u32x4 wa = *reinterpret_cast<const u32x4*>(smem + ((size_t)(f * (u32)KS + (u32)ks) * 64u + lane) * 16u);
#pragma unroll
        for (int t = 0; t < 8; ++t) acc[t] = mfma16<DT>(wa, bop[ks][t], acc[t]);
      }
      if constexpr (STATS) {
        float m1[4] = {0.f, 0.f, 0.f, 0.f}, m2[4] = {0.f, 0.f, 0.f, 0.f};
        if (tail) pw_store_frag<DT, true, true>(acc, yb, HW, M, row0, nvalid, m1, m2);
        else pw_store_frag<DT, false, true>(acc, yb, HW, M, row0, 8, m1, m2);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float a1 = pw_sum16(m1[i]), a2 = pw_sum16(m2[i]);
          if (fr == 0u) {  // (the wave's own words: no atomics)
            wst[(16u * f + 4u * fg + (u32)i) * 2u + 0u] += a1;
            wst[(16u * f + 4u * fg + (u32)i) * 2u + 1u] += a2;
          }
        }
      } else {
        if (tail) pw_store_frag<DT, true>(acc, yb, HW, M, row0, nvalid);
        else pw_store_frag<DT, false>(acc, yb, HW, M, row0, 8);
      }
    }
  }
  if constexpr (STATS) {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    float* dst = p.stats + ((size_t)(blockIdx.x * 4u + wave) * M + m0) * 2u;
    for (u32 i = lane; i < nf * 32u; i += 64u)
      if (m0 + (i >> 1) < M) dst[i] = wst[i];
  }
}

// ---- (P) long K: NF output fragments x 8 pixel sets of accumulators per wave, k-steps outermost, the weights of the slice
// staged in chunks of PWT_KC k-steps (a workgroup's four waves walk through the chunks together).  Projection layers
// (96 ... 960 -> 16 ... 320) and the input gradients of the expansions. -------------------------------------------------------
template <int DT, int NF, bool STATS = false, bool SL = false, bool AF = false>
__global__ __launch_bounds__(PWT_THREADS) void pw_gemm_long_kernel(const PwtParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const u32 tid = threadIdx.x, lane = tid & 63u;
  const u32 wave = (u32)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
  const u32 fr = lane & 15u, fg = lane >> 4;
  const u32 M = (u32)p.M, K = (u32)p.K, HW = (u32)p.HW, KS = (u32)p.KS;
  const u32 m0 = blockIdx.y * (u32)(16 * NF);
  const bool one_chunk = KS <= (u32)PWT_KC;
  const float* cf = reinterpret_cast<const float*>(smem + p.cf_off);
  if constexpr (AF) {
    pw_stage_coef(reinterpret_cast<float*>(smem + p.cf_off), p.coef, K, KS, tid);
    if (!one_chunk) __syncthreads();
  }
  if (one_chunk) {
    pw_stage_a<SL>(smem, p.a, M, K, SL ? p.lda : K, m0, (u32)NF, 0u, KS, tid);
    __syncthreads();
  }
  float sm1[STATS ? NF : 1][4], sm2[STATS ? NF : 1][4];  // STATS: the lane's share of (sum, sum of squares) per output row
#pragma unroll
  for (int f = 0; f < (STATS ? NF : 1); ++f)
#pragma unroll
    for (int i = 0; i < 4; ++i) sm1[f][i] = sm2[f][i] = 0.f;
  for (u32 it = blockIdx.x; it < p.wg_iters; it += gridDim.x) {
    const u32 g = it * 4u + wave;
    const bool live = g < p.groups;  // wave-uniform; a dead wave still stages and meets the barriers
    const u32 gg = live ? g : p.groups - 1u;
    const u32 b = gg / p.gpi, p0 = (gg - b * p.gpi) * 128u + 8u * fr;
    const bool tail = (gg - b * p.gpi) * 128u + 128u > HW;
    const int nvalid = (int)HW - (int)p0;
    const u16* xb = p.x + (SL ? (size_t)b * p.xs : (size_t)b * K * HW) + p0;
    u16* yb = p.y + (SL ? (size_t)b * p.ys : (size_t)b * M * HW) + p0;
    f32x4 acc[NF][8];
#pragma unroll
    for (int f = 0; f < NF; ++f) {
      const u32 row0 = m0 + 16u * (u32)f + 4u * fg;
      f32x4 init = {0.f, 0.f, 0.f, 0.f};
      if (p.bias) {
#pragma unroll
        for (int i = 0; i < 4; ++i) init[i] = row0 + (u32)i < M ? p.bias[row0 + (u32)i] : 0.f;
      }
#pragma unroll
      for (int t = 0; t < 8; ++t) acc[f][t] = init;
    }
    u32x4 raw[8];
    if (tail) pw_load_raw<true, SL>(xb, HW, K, fg * 8u, nvalid, raw);
    else pw_load_raw<false, SL>(xb, HW, K, fg * 8u, 8, raw);
    for (u32 c0 = 0; c0 < KS; c0 += (u32)PWT_KC) {
      const u32 nks = min((u32)PWT_KC, KS - c0);
      if (!one_chunk) {
        __syncthreads();  // every wave is done with the previous chunk's fragments
        pw_stage_a<SL>(smem, p.a, M, K, SL ? p.lda : K, m0, (u32)NF, c0, nks, tid);
        __syncthreads();
      }
      for (u32 ks = 0; ks < nks; ++ks) {
        u32x4 bop[8];
        if constexpr (AF) pw_affine_raw<DT>(raw, cf + 2u * ((c0 + ks) * 32u + fg * 8u), tail ? nvalid : 8);
        pw_transpose8(raw, bop);
        const u32 kn = c0 + ks + 1u;
        if (kn < KS) {  // the next k-step's block travels under this one's MFMAs
          if (tail) pw_load_raw<true, SL>(xb, HW, K, kn * 32u + fg * 8u, nvalid, raw);
          else pw_load_raw<false, SL>(xb, HW, K, kn * 32u + fg * 8u, 8, raw);
        }
#pragma unroll
        for (int f = 0; f < NF; ++f) {
          const u32x4 wa = *reinterpret_cast<const u32x4*>(smem + ((size_t)((u32)f * nks + ks) * 64u + lane) * 16u);
#pragma unroll
          for (int t = 0; t < 8; ++t) acc[f][t] = mfma16<DT>(wa, bop[t], acc[f][t]);
        }
      }
    }
    if (live) {
#pragma unroll
      for (int f = 0; f < NF; ++f) {
        const u32 row0 = m0 + 16u * (u32)f + 4u * fg;
        if constexpr (STATS) {
          if (tail) pw_store_frag<DT, true, true>(acc[f], yb, HW, M, row0, nvalid, sm1[f], sm2[f]);
          else pw_store_frag<DT, false, true>(acc[f], yb, HW, M, row0, 8, sm1[f], sm2[f]);
        } else {
          if (tail) pw_store_frag<DT, true>(acc[f], yb, HW, M, row0, nvalid);
          else pw_store_frag<DT, false>(acc[f], yb, HW, M, row0, 8);
        }
      }
    }
  }
  if constexpr (STATS) {
    float* dst = p.stats + (size_t)(blockIdx.x * 4u + wave) * M * 2u;
#pragma unroll
    for (int f = 0; f < NF; ++f)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float a1 = pw_sum16(sm1[f][i]), a2 = pw_sum16(sm2[f][i]);
        const u32 row = m0 + 16u * (u32)f + 4u * fg + (u32)i;
        if (fr == 0u && row < M) {
          dst[row * 2u + 0u] = a1;
          dst[row * 2u + 1u] = a2;
        }
      }
  }
}

struct PwtPlan {
  bool is_short;
  int slices, nf;
  unsigned gx;
  size_t lds;
};

// geometry of a y = a x launch (shared by the launch and by the statistics workspace query)
static PwtPlan pw_gemm_plan(PwtParams& p, int B, int K, int M, int HW, bool stats) {
  p.B = B;
  p.K = K;
  p.M = M;
  p.HW = HW;
  p.KS = (K + 31) / 32;
  p.gpi = (u32)((HW + 127) / 128);
  p.groups = (u32)B * p.gpi;
  p.wg_iters = (p.groups + 3u) / 4u;
  const int mf = (M + 15) / 16;
  static const int force_long = getenv("SSDK_PW_LONG") ? atoi(getenv("SSDK_PW_LONG")) : 0;
  PwtPlan pl;
  pl.is_short = p.KS <= 3 && !force_long;
  if (pl.is_short) {
    // slice: all output fragments if their A fragments fit 64 KiB, else equal slices
    int slices = (mf * p.KS + 63) / 64;
    p.nf = (mf + slices - 1) / slices;
    pl.slices = (mf + p.nf - 1) / p.nf;
    pl.nf = p.nf;
    pl.lds = (size_t)p.nf * p.KS * 1024 + (stats ? (size_t)4 * p.nf * 32 * sizeof(float) : 0);
    pl.gx = (unsigned)(256 * 4 / pl.slices);  // ~4 workgroups per CU over all slices
  } else {
    // long K: NF <= 4 fragments per slice, equal slices -- and MORE slices (each re-reads x, from L2) when the pixels alone give the
    // chip too few workgroups: 960 -> 160 on 16 x 16 maps at batch 64 is 32 workgroup iterations; as 3 slices of 4 fragments it
    // ran on 96 workgroups in 33 us (library GEMM: 22), as 5 slices of 2 on 160
    int slices = (mf + 3) / 4;
    const int wanted = (int)((256u + p.wg_iters - 1u) / p.wg_iters);
    if (slices < wanted) slices = wanted < mf ? wanted : mf;
    const int nf = (mf + slices - 1) / slices;
    pl.slices = (mf + nf - 1) / nf;
    pl.nf = p.nf = nf;
    const int nks = p.KS < PWT_KC ? p.KS : PWT_KC;
    pl.lds = (size_t)nf * nks * 1024;
    pl.gx = (unsigned)(256 * 3 / pl.slices);
  }
  if (pl.gx < 1u) pl.gx = 1u;
  if (pl.gx > p.wg_iters) pl.gx = p.wg_iters;
  return pl;
}

// stats_ws (optional): [gx * 4 waves][M][2] fp32 per-wave moments of the stored outputs (the caller reduces them)
// SL: xs / ys / lda as PwtParams describes them (ignored otherwise)
// AF: coef [K][4] of the operand transform (its LDS copy lies behind the plan's bytes)
template <bool SL = false, bool AF = false>
static int pw_gemm_launch(const void* x, const void* a, const float* bias, void* y, int B, int K, int M, int HW, int dtype,
                          hipStream_t stream, float* stats_ws = nullptr, unsigned* rows_out = nullptr, size_t xs = 0, size_t ys = 0,
                          unsigned lda = 0, const float* coef = nullptr) {
  PwtParams p;
  p.x = (const u16*)x;
  p.a = (const u16*)a;
  p.bias = bias;
  p.y = (u16*)y;
  p.stats = stats_ws;
  p.xs = xs;
  p.ys = ys;
  p.lda = lda;
  const bool st = stats_ws != nullptr;
  const PwtPlan pl = pw_gemm_plan(p, B, K, M, HW, st);
  if (rows_out) *rows_out = pl.gx * 4u;
  const dim3 grid(pl.gx, (unsigned)pl.slices);
  p.coef = coef;
  p.cf_off = (u32)pl.lds;
  const size_t lds = pl.lds + (AF ? (size_t)p.KS * 32 * 2 * sizeof(float) : 0);
  const int nf = pl.nf;
  if (pl.is_short) {
#define SSDK_PWS(DT, KS_, ST_)                                                                                         \
  do {                                                                                                                \
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&pw_gemm_short_kernel<DT, KS_, ST_, SL, AF>),                     \
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);                                  \
    hipLaunchKernelGGL((pw_gemm_short_kernel<DT, KS_, ST_, SL, AF>), grid, dim3(PWT_THREADS), lds, stream, p);                \
  } while (0)
#define SSDK_PWSK(DT, KS_)             \
  do {                                 \
    if (st) SSDK_PWS(DT, KS_, true);   \
    else SSDK_PWS(DT, KS_, false);     \
  } while (0)
#define SSDK_PWSD(DT)                     \
  do {                                    \
    if (p.KS == 1) SSDK_PWSK(DT, 1);      \
    else if (p.KS == 2) SSDK_PWSK(DT, 2); \
    else SSDK_PWSK(DT, 3);                \
  } while (0)
    if (dtype == SSDK_BF16) SSDK_PWSD(SSDK_BF16);
    else SSDK_PWSD(SSDK_F16);
#undef SSDK_PWSD
#undef SSDK_PWSK
#undef SSDK_PWS
    return check_launch("pw_gemm_short_kernel");
  }
#define SSDK_PWL(DT, NF_, ST_)                                                                                        \
  do {                                                                                                                \
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&pw_gemm_long_kernel<DT, NF_, ST_, SL, AF>),                      \
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);                                  \
    hipLaunchKernelGGL((pw_gemm_long_kernel<DT, NF_, ST_, SL, AF>), grid, dim3(PWT_THREADS), lds, stream, p);                 \
  } while (0)
#define SSDK_PWLN(DT, NF_)            \
  do {                                \
    if (st) SSDK_PWL(DT, NF_, true);  \
    else SSDK_PWL(DT, NF_, false);    \
  } while (0)
#define SSDK_PWLD(DT)                    \
  do {                                   \
    if (nf == 1) SSDK_PWLN(DT, 1);       \
    else if (nf == 2) SSDK_PWLN(DT, 2);  \
    else if (nf == 3) SSDK_PWLN(DT, 3);  \
    else SSDK_PWLN(DT, 4);               \
  } while (0)
  if (dtype == SSDK_BF16) SSDK_PWLD(SSDK_BF16);
  else SSDK_PWLD(SSDK_F16);
#undef SSDK_PWLD
#undef SSDK_PWLN
#undef SSDK_PWL
  return check_launch("pw_gemm_long_kernel");
}

// ---- weight gradient ------------------------------------------------------------------------------------------------------
struct PwgParams {
  const u16* dy;  // [B, Cout, HW]
  const u16* x;   // [B, Cin, HW], images xs elements apart (Cin * HW, or more: a channel slice)
  size_t xs;
  float* ws;      // [S][Cout][Cin] fp32 partials
  int B, Cout, Cin, HW;
  u32 cpi;        // 128-pixel chunks per image
  u32 chunks;     // B * cpi
  u32 mt, nt;     // tiles of the [Cout, Cin] matrix
  u32 splits;     // pixel ranges
  u32 cps;        // chunks per split
  const float* coef;  // AF kernels only: [Cin][4] = (a, b, ., .), x is read as op(x) (pw_affine8)
};

// AF: a lane's rows of x are fixed for the whole kernel, so their (a, b) live in registers
template <int DT, int MFW, int NFW, bool AF = false>
__global__ __launch_bounds__(PWT_THREADS) void pw_wgrad_kernel(const PwgParams p) {
  const u32 tid = threadIdx.x, lane = tid & 63u;
  const u32 wave = (u32)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
  const u32 fr = lane & 15u, fg = lane >> 4;
  const u32 tiles = p.mt * p.nt;
  const u32 item = blockIdx.x * 4u + wave;
  if (item >= tiles * p.splits) return;
  const u32 tile = item % tiles, s = item / tiles;
  const u32 m0 = (tile / p.nt) * (u32)(16 * MFW), n0 = (tile % p.nt) * (u32)(16 * NFW);
  const u32 Cout = (u32)p.Cout, Cin = (u32)p.Cin, HW = (u32)p.HW;
  f32x4 acc[MFW][NFW];
#pragma unroll
  for (int i = 0; i < MFW; ++i)
#pragma unroll
    for (int j = 0; j < NFW; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  float ca[AF ? NFW : 1], cb[AF ? NFW : 1];
  if constexpr (AF) {
#pragma unroll
    for (int j = 0; j < NFW; ++j) {
      const u32 row = n0 + 16u * (u32)j + fr;
      ca[j] = row < Cin ? p.coef[4u * row] : 0.f;
      cb[j] = row < Cin ? p.coef[4u * row + 1u] : 0.f;
    }
  }
  const u32 c_end = min(p.chunks, (s + 1u) * p.cps);
  for (u32 c = s * p.cps; c < c_end; ++c) {
    // k-step u of the chunk = its pixels 32 u .. 32 u + 31, lane group fg the 8 pixels 32 u + 8 fg ..: ONE load instruction
    // reads 64 contiguous bytes of each of its 16 rows.  (As first written a lane took 32 CONSECUTIVE pixels over its four loads,
    // i.e. every instruction touched sixteen 16-byte pieces 64 bytes apart per row: the 32 x 32 layers ran at 0.19 of the roof.)
    const u32 b = c / p.cpi, p0 = (c - b * p.cpi) * 128u + 8u * fg;
    const bool tail = (c - b * p.cpi) * 128u + 128u > HW;  // wave-uniform
    u32x4 av[MFW][4], bv[NFW][4];
#pragma unroll
    for (int i = 0; i < MFW; ++i) {
      const u32 row = m0 + 16u * (u32)i + fr;
      const u16* src = p.dy + ((size_t)b * Cout + row) * HW + p0;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (row < Cout) av[i][u] = tail ? pw_load8<true>(src + 32 * u, (int)HW - (int)p0 - 32 * u) : pw_load8<false>(src + 32 * u, 8);
        else av[i][u] = u32x4{0u, 0u, 0u, 0u};
      }
    }
#pragma unroll
    for (int j = 0; j < NFW; ++j) {
      const u32 row = n0 + 16u * (u32)j + fr;
      const u16* src = p.x + (size_t)b * p.xs + (size_t)row * HW + p0;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (row < Cin) bv[j][u] = tail ? pw_load8<true>(src + 32 * u, (int)HW - (int)p0 - 32 * u) : pw_load8<false>(src + 32 * u, 8);
        else bv[j][u] = u32x4{0u, 0u, 0u, 0u};
      }
    }
    if constexpr (AF) {  // (rows >= Cin: a = b = 0, the zeros stay zeros)
#pragma unroll
      for (int j = 0; j < NFW; ++j)
#pragma unroll
        for (int u = 0; u < 4; ++u) bv[j][u] = pw_affine8<DT>(bv[j][u], ca[j], cb[j], tail ? (int)HW - (int)p0 - 32 * u : 8);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int i = 0; i < MFW; ++i)
#pragma unroll
        for (int j = 0; j < NFW; ++j) acc[i][j] = mfma16<DT>(av[i][u], bv[j][u], acc[i][j]);
  }
  // partial tile -> workspace: D[row 4 fg + r of fragment i][column fr of fragment j]
  float* ws = p.ws + (size_t)s * Cout * Cin;
#pragma unroll
  for (int i = 0; i < MFW; ++i)
#pragma unroll
    for (int j = 0; j < NFW; ++j) {
      const u32 ci = n0 + 16u * (u32)j + fr;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const u32 co = m0 + 16u * (u32)i + 4u * fg + (u32)r;
        if (co < Cout && ci < Cin) ws[(size_t)co * Cin + ci] = acc[i][j][r];
      }
    }
}

// ---- weight gradient of the layers whose [Cout, Cin] matrix is large on BOTH sides (the 32 x 32 / 16 x 16 blocks: 64 ... 960
// channels either side).  The streaming kernel above re-reads dy once per column tile and x once per row tile -- 4.3 x the bytes
// on 96 -> 576 -- in 16-row x 64-byte pieces: 0.2 of the roof there.  Here a workgroup owns a 128 x 128 tile of dW and walks
// over pixels in chunks of 128: both operand tiles are staged in LDS with full-row 256-byte global reads (12 independent
// 16-byte loads per thread per chunk, the next chunk's requested before this chunk's MFMAs), a wave reads its 4 + 4 fragments
// per k-step from LDS (row stride 288 bytes = 18 x 16: conflict-free for the lane groups of ds_read_b128).
constexpr u32 PWG_RS = 288;
constexpr size_t PWG_LDS = 2 * 128 * PWG_RS;

template <int DT, bool AF = false>
__global__ __launch_bounds__(PWT_THREADS) void pw_wgrad_tiled_kernel(const PwgParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char* la = smem;
  unsigned char* lb = smem + 128 * PWG_RS;
  const u32 tid = threadIdx.x, lane = tid & 63u;
  const u32 wave = (u32)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
  const u32 fr = lane & 15u, fg = lane >> 4, wm = wave >> 1, wn = wave & 1u;
  const u32 tiles = p.mt * p.nt;
  const u32 tile = blockIdx.x % tiles, s = blockIdx.x / tiles;
  const u32 m0 = (tile / p.nt) * 128u, n0 = (tile % p.nt) * 128u;
  const u32 Cout = (u32)p.Cout, Cin = (u32)p.Cin, HW = (u32)p.HW;
  const u32 r16 = tid >> 4, c16 = tid & 15u;  // staging role: row r16 (+ 16 per pass), 16-byte column c16 of the 256-byte row
  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const u32 c_begin = s * p.cps, c_end = min(p.chunks, (s + 1u) * p.cps);
  u32x4 va[8], vb[8];
  float ca[AF ? 8 : 1], cb[AF ? 8 : 1];  // AF: (a, b) of the thread's eight staging rows of x
  int nv = 8;                            // ... and the pixels of the fetched chunk inside the plane
  if constexpr (AF) {
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const u32 rb = n0 + (u32)q * 16u + r16;
      ca[q] = rb < Cin ? p.coef[4u * rb] : 0.f;
      cb[q] = rb < Cin ? p.coef[4u * rb + 1u] : 0.f;
    }
  }
  auto fetch = [&](u32 c) {
    const u32 b = c / p.cpi, p0 = (c - b * p.cpi) * 128u + 8u * c16;
    const int nvalid = (int)HW - (int)p0;
    nv = nvalid;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const u32 ra = m0 + (u32)q * 16u + r16, rb = n0 + (u32)q * 16u + r16;
      va[q] = ra < Cout ? pw_load8<true>(p.dy + ((size_t)b * Cout + ra) * HW + p0, nvalid) : u32x4{0u, 0u, 0u, 0u};
      vb[q] = rb < Cin ? pw_load8<true>(p.x + (size_t)b * p.xs + (size_t)rb * HW + p0, nvalid) : u32x4{0u, 0u, 0u, 0u};
    }
  };
  if (c_begin < c_end) fetch(c_begin);
  for (u32 c = c_begin; c < c_end; ++c) {
    __syncthreads();  // every wave is done with the previous chunk's fragments
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      *reinterpret_cast<u32x4*>(la + ((u32)q * 16u + r16) * PWG_RS + c16 * 16u) = va[q];
      if constexpr (AF) vb[q] = pw_affine8<DT>(vb[q], ca[q], cb[q], nv);  // (on the way to LDS: the fetch stays in flight)
      *reinterpret_cast<u32x4*>(lb + ((u32)q * 16u + r16) * PWG_RS + c16 * 16u) = vb[q];
    }
    __syncthreads();
    if (c + 1u < c_end) fetch(c + 1u);  // travels under this chunk's MFMAs
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      u32x4 af[4], bf[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        af[i] = *reinterpret_cast<const u32x4*>(la + (64u * wm + 16u * (u32)i + fr) * PWG_RS + (u32)u * 64u + fg * 16u);
        bf[i] = *reinterpret_cast<const u32x4*>(lb + (64u * wn + 16u * (u32)i + fr) * PWG_RS + (u32)u * 64u + fg * 16u);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = mfma16<DT>(af[i], bf[j], acc[i][j]);
    }
  }
  float* ws = p.ws + (size_t)s * Cout * Cin;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const u32 ci = n0 + 64u * wn + 16u * (u32)j + fr;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const u32 co = m0 + 64u * wm + 16u * (u32)i + 4u * fg + (u32)r;
        if (co < Cout && ci < Cin) ws[(size_t)co * Cin + ci] = acc[i][j][r];
      }
    }
}

// -> true: the LDS-tiled kernel (128 x 128 tiles of dW), false: the streaming kernel (wave tiles of mfw x nfw fragments)
static bool pw_wgrad_plan(int B, int Cout, int Cin, int HW, PwgParams* p, int* mfw, int* nfw) {
  const int mf = (Cout + 15) / 16, nf = (Cin + 15) / 16;
  p->cpi = (u32)((HW + 127) / 128);
  p->chunks = (u32)B * p->cpi;
  static const int env_tiled = getenv("SSDK_PW_WGRAD_TILED") ? atoi(getenv("SSDK_PW_WGRAD_TILED")) : 1;
  const bool tiled = env_tiled && mf >= 4 && nf >= 4;
  u32 tiles, target;
  if (tiled) {
    *mfw = *nfw = 8;
    p->mt = (u32)((Cout + 127) / 128);
    p->nt = (u32)((Cin + 127) / 128);
    tiles = p->mt * p->nt;
    target = 512u;  // workgroups: two per CU
  } else {
    // wave tile: 3 x 2 fragments (20 vectors of 16 bytes in flight per lane), 3 x 1 for narrow inputs
    *mfw = mf >= 3 ? 3 : mf;
    *nfw = nf >= 2 ? 2 : 1;
    p->mt = (u32)((mf + *mfw - 1) / *mfw);
    p->nt = (u32)((nf + *nfw - 1) / *nfw);
    tiles = p->mt * p->nt;
    target = 4096u;  // waves: ~16 per CU
  }
  u32 splits = target / tiles;
  if (splits < 1u) splits = 1u;
  if (splits > p->chunks) splits = p->chunks;
  p->cps = (p->chunks + splits - 1u) / splits;
  p->splits = (p->chunks + p->cps - 1u) / p->cps;
  return tiled;
}

// sum of `rows` rows of n floats in a fixed order -> dst (ssdk_pwtrain.hip: pw_wgrad_reduce_kernel, <= 4096 rows)
int reduce_rows_fixed_order(const float* src, float* mid, float* dst, unsigned n, unsigned rows, hipStream_t st);

// dW = sum_b dy[b] x[b]^T with the images of x `xs` elements apart; arguments checked by the caller, except the workspace size
// AF: x is read as op(x) with coef [Cin][4]
template <bool AF = false>
static int pw_wgrad_run(const void* dy, const void* x, size_t xs, float* dw, void* ws, size_t ws_bytes, int B, int Cout, int Cin, int HW,
                        int dtype, hipStream_t stream, const char* what, const float* coef = nullptr) {
  PwgParams p;
  int mfw, nfw;
  const bool tiled = pw_wgrad_plan(B, Cout, Cin, HW, &p, &mfw, &nfw);
  if (ws_bytes < ((size_t)p.splits + (size_t)((p.splits + 63u) / 64u)) * (size_t)Cout * (size_t)Cin * sizeof(float)) {
    set_error("%s: workspace too small", what);
    return SSDK_E_WORKSPACE;
  }
  p.dy = (const u16*)dy;
  p.x = (const u16*)x;
  p.xs = xs;
  p.coef = coef;
  p.ws = (float*)ws;
  p.B = B;
  p.Cout = Cout;
  p.Cin = Cin;
  p.HW = HW;
  const u32 items = p.mt * p.nt * p.splits;
  const dim3 grid(tiled ? items : (items + 3u) / 4u);
  hipStream_t st = stream;
  if (tiled) {
    if (dtype == SSDK_BF16) {
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&pw_wgrad_tiled_kernel<SSDK_BF16, AF>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)PWG_LDS);
      hipLaunchKernelGGL((pw_wgrad_tiled_kernel<SSDK_BF16, AF>), grid, dim3(PWT_THREADS), PWG_LDS, st, p);
    } else {
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&pw_wgrad_tiled_kernel<SSDK_F16, AF>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)PWG_LDS);
      hipLaunchKernelGGL((pw_wgrad_tiled_kernel<SSDK_F16, AF>), grid, dim3(PWT_THREADS), PWG_LDS, st, p);
    }
  } else {
#define SSDK_PWG(DT, MF_, NF_) hipLaunchKernelGGL((pw_wgrad_kernel<DT, MF_, NF_, AF>), grid, dim3(PWT_THREADS), 0, st, p)
#define SSDK_PWGD(DT)                                  \
  do {                                                 \
    if (mfw == 3 && nfw == 2) SSDK_PWG(DT, 3, 2);      \
    else if (mfw == 3) SSDK_PWG(DT, 3, 1);             \
    else if (mfw == 2 && nfw == 2) SSDK_PWG(DT, 2, 2); \
    else if (mfw == 2) SSDK_PWG(DT, 2, 1);             \
    else if (nfw == 2) SSDK_PWG(DT, 1, 2);             \
    else SSDK_PWG(DT, 1, 1);                           \
  } while (0)
  if (dtype == SSDK_BF16) SSDK_PWGD(SSDK_BF16);
  else SSDK_PWGD(SSDK_F16);
#undef SSDK_PWGD
#undef SSDK_PWG
  }
  int rc = check_launch(tiled ? "pw_wgrad_tiled_kernel" : "pw_wgrad_kernel");
  if (rc) return rc;
  const u32 n = (u32)Cout * (u32)Cin;
  return reduce_rows_fixed_order((const float*)ws, (float*)ws + (size_t)p.splits * n, dw, n, p.splits, st);
}

}  // namespace ssdk
