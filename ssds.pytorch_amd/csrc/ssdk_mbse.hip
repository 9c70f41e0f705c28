// ssdk_mbse.hip -- the tail of an EfficientNet MBConv block on gfx950 (nets/efficientnet.py MBConvBlock: everything
// behind the expand 1x1): k x k depthwise convolution + folded BN + SiLU, squeeze-and-excitation gate, gated 1x1
// projection + folded BN (+ residual).  NHWC, bf16 | f16, three launches behind one entry point (ssdk_mbse):
//
//   mbse_dw_kernel    x [N][H][W][C] -> t [N][Ho][Wo][C] (k = 3 | 5, stride 1 | 2, pad k / 2), 8 channels per lane as one
//                     16-byte vector, fp32 accumulation in tap order, one rounding.  A workgroup owns a 16 x 16 tile of
//                     output pixels of one image and a slice of <= 32 channel octets; it also sums the values of t AS
//                     STORED (after the rounding) per channel -- per lane over its pixels in index order, then over the
//                     lanes' pixel slots as a fixed binary tree in LDS -- and writes that sum ONCE to
//                     pool_partial [N][T][C].  No atomics: two runs give the same bits.
//   mbse_gate_kernel  one workgroup per image: mean[c] = (sum over the T tiles, four contiguous quarters added in
//                     order) / (Ho Wo); s = silu(W1 mean + b1) (a wave per output, lanes stride over C, butterfly
//                     reduction); gate = sigmoid(W2 s + b2) (a lane per channel, R terms in index order).  fp32 VALU.
//   mbse_proj_kernel  y [M = N Ho Wo][Cout] = (sum_c round16(t[m][c] * gate[n(m)][c]) * Wp[co][c]) * scale[co] + bias[co]
//                     (+ residual), v_mfma_f32_16x16x32: the weights are the A operand (rows = output channels), the
//                     pixels the B operand.  The gate multiplies the t fragment on its way into the matrix core -- each
//                     lane looks up the gate of ITS pixel's image, so a 16-pixel fragment may straddle images -- and the
//                     product is rounded to the tensor dtype (the matrix core takes 16-bit operands; that is also what a
//                     16-bit `x * se(x)` tensor op stores).  A wave owns PT fragments of 16 pixels and up to 8 blocks of 16
//                     output channels; operands come straight from global memory (no LDS, no barrier).  K tails (C % 32 =
//                     8, 16, 24), the Cout tail (Cout % 16 = 8) and the pixel tail are zero fragments / masked stores.
#include "ssdk_conv_common.h"

namespace ssdk {

constexpr int kMbseTile = 16;      // output pixels per tile side (ssdk_mbse_pool_tiles)
constexpr int kMbseMaxC = 4096;    // gate kernel LDS: mean[C]
constexpr int kMbseMaxR = 1024;    // gate kernel LDS: s[R]

struct MbseDwParams {
  const u16* x;
  u16* t;
  float* partial;
  const u16* w;  // [k][k][C]
  const float* scale;
  const float* bias;
  int N, H, W, C, Ho, Wo, stride;
  int tiles_x, T;   // tiles per row, tiles per image
  int cgb, slots;   // channel octets per workgroup slice, pixel slots per workgroup (slots * cgb <= 256)
};

template <int DT, int K>
__global__ __launch_bounds__(256) void mbse_dw_kernel(const MbseDwParams p) {
  __shared__ float red[256 * 8];
  __shared__ u32x4 wl[K * K * 32];  // the slice's weights [tap][octet]: in registers a 5 x 5 window costs 100 VGPRs (one wave per SIMD)
  const int tid = (int)threadIdx.x;
  const int cgl = tid % p.cgb, slot = tid / p.cgb;
  const int cg = (int)blockIdx.y * p.cgb + cgl;
  const int n = (int)blockIdx.z;
  const int ty0 = ((int)blockIdx.x / p.tiles_x) * kMbseTile, tx0 = ((int)blockIdx.x % p.tiles_x) * kMbseTile;
  const bool live = slot < p.slots && cg * 8 < p.C;
  for (int i = tid; i < K * K * p.cgb; i += 256) {
    const int q = i / p.cgb, o = (int)blockIdx.y * p.cgb + i % p.cgb;
    if (o * 8 < p.C) wl[i] = *reinterpret_cast<const u32x4*>(p.w + (size_t)q * p.C + o * 8);
  }
  __syncthreads();
  float sum[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) sum[e] = 0.f;
  if (live) {
    const int c0 = cg * 8;
    float sc[8], bi[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      sc[e] = p.scale[c0 + e];
      bi[e] = p.bias[c0 + e];
    }
    constexpr int PAD = K / 2;
    for (int pix = slot; pix < kMbseTile * kMbseTile; pix += p.slots) {
      const int oy = ty0 + pix / kMbseTile, ox = tx0 + pix % kMbseTile;
      if (oy >= p.Ho || ox >= p.Wo) continue;
      float acc[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] = 0.f;
#pragma unroll
      for (int ky = 0; ky < K; ++ky) {
        const int iy = oy * p.stride + ky - PAD;
        if ((unsigned)iy >= (unsigned)p.H) continue;
#pragma unroll
        for (int kx = 0; kx < K; ++kx) {
          const int ix = ox * p.stride + kx - PAD;
          if ((unsigned)ix >= (unsigned)p.W) continue;
          const u32x4 xv = *reinterpret_cast<const u32x4*>(p.x + (((size_t)n * p.H + iy) * p.W + ix) * p.C + c0);
          const u32x4 ww = wl[(ky * K + kx) * p.cgb + cgl];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            acc[2 * e] = fmaf(bits16_to_f32<DT>(xv[e] & 0xffffu), bits16_to_f32<DT>(ww[e] & 0xffffu), acc[2 * e]);
            acc[2 * e + 1] = fmaf(bits16_to_f32<DT>(xv[e] >> 16), bits16_to_f32<DT>(ww[e] >> 16), acc[2 * e + 1]);
          }
        }
      }
      u32x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float v0 = fmaf(acc[2 * e], sc[2 * e], bi[2 * e]), v1 = fmaf(acc[2 * e + 1], sc[2 * e + 1], bi[2 * e + 1]);
        v0 = v0 * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.442695041f * v0));
        v1 = v1 * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.442695041f * v1));
        o[e] = pack2_16<DT>(v0, v1);
        sum[2 * e] += bits16_to_f32<DT>(o[e] & 0xffffu);  // the pool sees t as stored
        sum[2 * e + 1] += bits16_to_f32<DT>(o[e] >> 16);
      }
      *reinterpret_cast<u32x4*>(p.t + (((size_t)n * p.Ho + oy) * p.Wo + ox) * p.C + c0) = o;
    }
  }
  // slots -> one sum per channel: a fixed binary tree over the slot index (slot s takes slot s + h, h = 128, 64, ... 1)
#pragma unroll
  for (int e = 0; e < 8; ++e) red[tid * 8 + e] = sum[e];
  __syncthreads();
  for (int h = 128; h >= 1; h >>= 1) {
    if (slot < h && slot + h < p.slots && slot < p.slots) {
      const int other = (slot + h) * p.cgb + cgl;
#pragma unroll
      for (int e = 0; e < 8; ++e) red[tid * 8 + e] += red[other * 8 + e];
    }
    __syncthreads();
  }
  if (slot == 0 && cg * 8 < p.C) {
    float* dst = p.partial + ((size_t)n * p.T + blockIdx.x) * p.C + cg * 8;
    *reinterpret_cast<float4*>(dst) = make_float4(red[tid * 8], red[tid * 8 + 1], red[tid * 8 + 2], red[tid * 8 + 3]);
    *reinterpret_cast<float4*>(dst + 4) = make_float4(red[tid * 8 + 4], red[tid * 8 + 5], red[tid * 8 + 6], red[tid * 8 + 7]);
  }
}

struct MbseGateParams {
  const float* partial;
  float* gate;
  const float* w1;
  const float* b1;
  const float* w2;
  const float* b2;
  int C, R, T;
  float hw;  // Ho * Wo
};

__global__ __launch_bounds__(256) void mbse_gate_kernel(const MbseGateParams p) {
  __shared__ float mean[kMbseMaxC];
  __shared__ float sq[kMbseMaxR];
  __shared__ float part[4][64];
  const int tid = (int)threadIdx.x, n = (int)blockIdx.x;
  const int q = tid >> 6, cl = tid & 63;
  const int tq = (p.T + 3) / 4;  // tiles per quarter
  const float* src = p.partial + (size_t)n * p.T * p.C;
  for (int c0 = 0; c0 < p.C; c0 += 64) {
    const int c = c0 + cl;
    float s = 0.f;
    if (c < p.C) {
      const int t1 = min(p.T, (q + 1) * tq);
      for (int t = q * tq; t < t1; ++t) s += src[(size_t)t * p.C + c];
    }
    part[q][cl] = s;
    __syncthreads();
    if (q == 0 && c < p.C) mean[c] = (((part[0][cl] + part[1][cl]) + part[2][cl]) + part[3][cl]) / p.hw;
    __syncthreads();
  }
  // FC1 + SiLU: wave q takes outputs q, q + 4, ...; lane l sums channels l, l + 64, ... in order, then a butterfly
  for (int r = q; r < p.R; r += 4) {
    const float* w = p.w1 + (size_t)r * p.C;
    float s = 0.f;
    for (int c = cl; c < p.C; c += 64) s = fmaf(w[c], mean[c], s);
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) s += __shfl_xor(s, d);
    if (cl == 0) {
      const float v = s + p.b1[r];
      sq[r] = v * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.442695041f * v));
    }
  }
  __syncthreads();
  for (int c = tid; c < p.C; c += 256) {
    const float* w = p.w2 + (size_t)c * p.R;
    float s = 0.f;
    for (int r = 0; r < p.R; ++r) s = fmaf(w[r], sq[r], s);
    const float v = s + p.b2[c];
    p.gate[(size_t)n * p.C + c] = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.442695041f * v));
  }
}

struct MbseProjParams {
  const u16* t;
  const float* gate;
  const u16* w;  // [Cout][C]
  const float* scale;
  const float* bias;
  const u16* res;
  u16* y;
  int M, HW, C, Cout;
  int cpc;  // blocks of 16 output channels per blockIdx.y (<= 8)
};

template <int DT, int PT>
__global__ __launch_bounds__(256) void mbse_proj_kernel(const MbseProjParams p) {
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  const int l15 = lane & 15, l4 = lane >> 4;
  const long m0 = ((long)blockIdx.x * 4 + wave) * (16 * PT);
  if (m0 >= p.M) return;  // (wave-uniform; the kernel has no barrier)
  const int cb0 = (int)blockIdx.y * p.cpc;
  const int ncb = min(p.cpc, (p.Cout + 15) / 16 - cb0);
  long pix[PT];
  bool pok[PT];
  const u16* tp[PT];
  const float* gp[PT];
#pragma unroll
  for (int i = 0; i < PT; ++i) {
    pix[i] = m0 + 16 * i + l15;
    pok[i] = pix[i] < p.M;
    const long pc = pok[i] ? pix[i] : 0;
    tp[i] = p.t + (size_t)pc * p.C;
    gp[i] = p.gate + (size_t)(pc / p.HW) * p.C;
  }
  f32x4 acc[PT][8];
#pragma unroll
  for (int i = 0; i < PT; ++i)
#pragma unroll
    for (int b = 0; b < 8; ++b) acc[i][b] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int ksteps = (p.C + 31) / 32;
  for (int ks = 0; ks < ksteps; ++ks) {
    const int k0 = ks * 32 + 8 * l4;
    const bool kok = k0 < p.C;  // K tail: C is a multiple of 8, so an octet is all in or all out
    u32x4 bf[PT];
#pragma unroll
    for (int i = 0; i < PT; ++i) {
      bf[i] = u32x4{0u, 0u, 0u, 0u};
      if (kok && pok[i]) {
        const u32x4 tv = *reinterpret_cast<const u32x4*>(tp[i] + k0);
        const float4 g0 = *reinterpret_cast<const float4*>(gp[i] + k0);
        const float4 g1 = *reinterpret_cast<const float4*>(gp[i] + k0 + 4);
        bf[i][0] = pack2_16<DT>(bits16_to_f32<DT>(tv[0] & 0xffffu) * g0.x, bits16_to_f32<DT>(tv[0] >> 16) * g0.y);
        bf[i][1] = pack2_16<DT>(bits16_to_f32<DT>(tv[1] & 0xffffu) * g0.z, bits16_to_f32<DT>(tv[1] >> 16) * g0.w);
        bf[i][2] = pack2_16<DT>(bits16_to_f32<DT>(tv[2] & 0xffffu) * g1.x, bits16_to_f32<DT>(tv[2] >> 16) * g1.y);
        bf[i][3] = pack2_16<DT>(bits16_to_f32<DT>(tv[3] & 0xffffu) * g1.z, bits16_to_f32<DT>(tv[3] >> 16) * g1.w);
      }
    }
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      if (b < ncb) {
        const int row = (cb0 + b) * 16 + l15;
        u32x4 af = u32x4{0u, 0u, 0u, 0u};
        if (kok && row < p.Cout) af = *reinterpret_cast<const u32x4*>(p.w + (size_t)row * p.C + k0);
#pragma unroll
        for (int i = 0; i < PT; ++i) acc[i][b] = mfma16<DT>(af, bf[i], acc[i][b]);
      }
    }
  }
  // D: column (pixel) = lane & 15, rows (output channels) = 4 (lane >> 4) + 0..3 of the block
#pragma unroll
  for (int b = 0; b < 8; ++b) {
    if (b < ncb) {
      const int co = (cb0 + b) * 16 + 4 * l4;
      if (co < p.Cout) {  // Cout is a multiple of 8: a group of 4 is all in or all out
        const float4 sc = *reinterpret_cast<const float4*>(p.scale + co);
        const float4 bi = *reinterpret_cast<const float4*>(p.bias + co);
#pragma unroll
        for (int i = 0; i < PT; ++i) {
          if (!pok[i]) continue;
          float v0 = fmaf(acc[i][b][0], sc.x, bi.x), v1 = fmaf(acc[i][b][1], sc.y, bi.y);
          float v2 = fmaf(acc[i][b][2], sc.z, bi.z), v3 = fmaf(acc[i][b][3], sc.w, bi.w);
          const size_t off = (size_t)pix[i] * p.Cout + co;
          if (p.res) {
            const uint2 rv = *reinterpret_cast<const uint2*>(p.res + off);
            v0 += bits16_to_f32<DT>(rv.x & 0xffffu);
            v1 += bits16_to_f32<DT>(rv.x >> 16);
            v2 += bits16_to_f32<DT>(rv.y & 0xffffu);
            v3 += bits16_to_f32<DT>(rv.y >> 16);
          }
          *reinterpret_cast<uint2*>(p.y + off) = make_uint2(pack2_16<DT>(v0, v1), pack2_16<DT>(v2, v3));
        }
      }
    }
  }
}

}  // namespace ssdk

using namespace ssdk;

extern "C" size_t ssdk_mbse_desc_bytes(void) { return sizeof(ssdk_mbse_desc); }

extern "C" int ssdk_mbse_pool_tiles(int H, int W, int k, int stride) {
  if (H < 1 || W < 1 || (k != 3 && k != 5) || (stride != 1 && stride != 2)) return 0;
  const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
  return ((Ho + kMbseTile - 1) / kMbseTile) * ((Wo + kMbseTile - 1) / kMbseTile);
}

extern "C" int ssdk_mbse(const ssdk_mbse_desc* d, void* stream) {
  if (!d) {
    set_error("mbse: null descriptor");
    return SSDK_E_BADARG;
  }
  const int stages = d->stages == 0 ? 7 : d->stages;
  if (stages < 0 || stages > 7) {
    set_error("mbse: stages must be a mask of 1 (depthwise + pool), 2 (gate), 4 (projection) or 0 (all), got %d", d->stages);
    return SSDK_E_BADARG;
  }
  if (d->dtype != SSDK_BF16 && d->dtype != SSDK_F16) {
    set_error("mbse: dtype must be bf16 or f16");
    return SSDK_E_BADARG;
  }
  if (d->N < 1 || d->H < 1 || d->W < 1 || d->C < 8 || (d->C % 8) || d->C > kMbseMaxC || d->Cout < 8 || (d->Cout % 8) ||
      (d->k != 3 && d->k != 5) || (d->stride != 1 && d->stride != 2) || d->R < 1 || d->R > kMbseMaxR || d->N > 65535) {
    set_error("mbse: bad geometry N=%d H=%d W=%d C=%d R=%d Cout=%d k=%d stride=%d (N <= 65535, C and Cout multiples of 8, C <= %d, "
              "k 3 | 5, stride 1 | 2, 1 <= R <= %d)", d->N, d->H, d->W, d->C, d->R, d->Cout, d->k, d->stride, kMbseMaxC, kMbseMaxR);
    return SSDK_E_BADARG;
  }
  const int Ho = (d->H - 1) / d->stride + 1, Wo = (d->W - 1) / d->stride + 1;
  const long long M = (long long)d->N * Ho * Wo;
  if (M > 0x7fffffffLL || (long long)d->N * d->H * d->W > 0x7fffffffLL) {
    set_error("mbse: more than 2^31 - 1 pixels");
    return SSDK_E_BADARG;
  }
  const bool s1 = stages & 1, s2 = stages & 2, s3 = stages & 4;
  if ((s1 && (!d->x || !d->t || !d->pool_partial || !d->w_dw || !d->scale_dw || !d->bias_dw)) ||
      (s2 && (!d->pool_partial || !d->gate || !d->w_se1 || !d->b_se1 || !d->w_se2 || !d->b_se2)) ||
      (s3 && (!d->t || !d->gate || !d->y || !d->w_proj || !d->scale_proj || !d->bias_proj))) {
    set_error("mbse: null pointer among the buffers of the requested stages (mask %d)", stages);
    return SSDK_E_BADARG;
  }
  if (((uintptr_t)d->x | (uintptr_t)d->t | (uintptr_t)d->pool_partial | (uintptr_t)d->gate | (uintptr_t)d->y |
       (uintptr_t)d->residual | (uintptr_t)d->w_dw | (uintptr_t)d->w_proj | (uintptr_t)d->scale_dw | (uintptr_t)d->bias_dw |
       (uintptr_t)d->scale_proj | (uintptr_t)d->bias_proj) & 15) {
    set_error("mbse: tensors, gate, pool_partial, weights and the folded BN vectors must be 16-byte aligned");
    return SSDK_E_BADARG;
  }
  if (((uintptr_t)d->w_se1 | (uintptr_t)d->b_se1 | (uintptr_t)d->w_se2 | (uintptr_t)d->b_se2) & 3) {
    set_error("mbse: the squeeze-excite weights must be 4-byte aligned");
    return SSDK_E_BADARG;
  }
  hipStream_t st = (hipStream_t)stream;
  const int tiles_x = (Wo + kMbseTile - 1) / kMbseTile, T = tiles_x * ((Ho + kMbseTile - 1) / kMbseTile);
  if (s1) {
    MbseDwParams p;
    p.x = (const u16*)d->x;
    p.t = (u16*)d->t;
    p.partial = d->pool_partial;
    p.w = (const u16*)d->w_dw;
    p.scale = d->scale_dw;
    p.bias = d->bias_dw;
    p.N = d->N, p.H = d->H, p.W = d->W, p.C = d->C, p.Ho = Ho, p.Wo = Wo, p.stride = d->stride;
    p.tiles_x = tiles_x, p.T = T;
    const int CG = d->C / 8, nchunk = (CG + 31) / 32;
    p.cgb = (CG + nchunk - 1) / nchunk;
    p.slots = 256 / p.cgb;
    const dim3 grid((unsigned)T, (unsigned)nchunk, (unsigned)d->N);
    if (d->dtype == SSDK_BF16) {
      if (d->k == 3) hipLaunchKernelGGL((mbse_dw_kernel<SSDK_BF16, 3>), grid, dim3(256), 0, st, p);
      else hipLaunchKernelGGL((mbse_dw_kernel<SSDK_BF16, 5>), grid, dim3(256), 0, st, p);
    } else {
      if (d->k == 3) hipLaunchKernelGGL((mbse_dw_kernel<SSDK_F16, 3>), grid, dim3(256), 0, st, p);
      else hipLaunchKernelGGL((mbse_dw_kernel<SSDK_F16, 5>), grid, dim3(256), 0, st, p);
    }
    if (int rc = check_launch("mbse_dw_kernel")) return rc;
  }
  if (s2) {
    MbseGateParams p;
    p.partial = d->pool_partial;
    p.gate = d->gate;
    p.w1 = d->w_se1, p.b1 = d->b_se1, p.w2 = d->w_se2, p.b2 = d->b_se2;
    p.C = d->C, p.R = d->R, p.T = T;
    p.hw = (float)(Ho * Wo);
    hipLaunchKernelGGL(mbse_gate_kernel, dim3((unsigned)d->N), dim3(256), 0, st, p);
    if (int rc = check_launch("mbse_gate_kernel")) return rc;
  }
  if (s3) {
    MbseProjParams p;
    p.t = (const u16*)d->t;
    p.gate = d->gate;
    p.w = (const u16*)d->w_proj;
    p.scale = d->scale_proj, p.bias = d->bias_proj;
    p.res = (const u16*)d->residual;
    p.y = (u16*)d->y;
    p.M = (int)M, p.HW = Ho * Wo, p.C = d->C, p.Cout = d->Cout;
    // big maps: 32 pixels x 128 output channels per wave (the weights are re-read once per 32 pixels); small ones: 16 x 32, so
    // that a 7 x 7 map still spreads over the chip
    const int cblocks = (d->Cout + 15) / 16;
    const bool big = ((M + 127) / 128) * ((cblocks + 7) / 8) >= 512;
    p.cpc = big ? 8 : 2;
    const int ppb = big ? 128 : 64;
    const dim3 grid((unsigned)((M + ppb - 1) / ppb), (unsigned)((cblocks + p.cpc - 1) / p.cpc));
    if (d->dtype == SSDK_BF16) {
      if (big) hipLaunchKernelGGL((mbse_proj_kernel<SSDK_BF16, 2>), grid, dim3(256), 0, st, p);
      else hipLaunchKernelGGL((mbse_proj_kernel<SSDK_BF16, 1>), grid, dim3(256), 0, st, p);
    } else {
      if (big) hipLaunchKernelGGL((mbse_proj_kernel<SSDK_F16, 2>), grid, dim3(256), 0, st, p);
      else hipLaunchKernelGGL((mbse_proj_kernel<SSDK_F16, 1>), grid, dim3(256), 0, st, p);
    }
    if (int rc = check_launch("mbse_proj_kernel")) return rc;
  }
  if (stages == 7) return check_launch("mbse_dw_kernel+mbse_gate_kernel+mbse_proj_kernel");
  return SSDK_OK;
}
