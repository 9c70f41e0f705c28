// ssdk_dkres.hip -- one DarkNet residual block (nets/darknet.py Residual: Conv 1x1 + BN + ReLU6, C -> C/2, then Conv 3x3 / pad 1 +
// BN + ReLU6, C/2 -> C, then + x) as ONE launch on gfx950, the intermediate map in LDS (include/ssdk_dkres.h).
//
// Why: as two launches the block moves x in, mid out, mid in, x in again for the add and y out -- about 4 C bytes per pixel where
// 2 C suffice -- and on the high-resolution stages of DarkNet53 (64 channels at H/2, 128 at H/4) that traffic, not the MFMA work,
// is the time.  Here a workgroup (4 waves) owns (image, tile of kDkTH x kDkTW output pixels):
//   phase 1  mid[hp][cm] = act1(bn1(x[hp][:] . W1[cm][:])) on the tile PLUS its one-pixel halo ((kDkTH + 2) x (kDkTW + 2) pixels,
//            padded to 12 fragments of 16; wave w owns fragments w, w + 4, w + 8), MFMA operands straight from global memory /
//            L2, results to LDS in the tensor dtype.  The 1x1 is a tenth of the block's FLOPs, so recomputing the halo (180 / 128)
//            is cheap.  A halo position OUTSIDE THE IMAGE gets ZEROS, not act1(bias1): the 3x3 pads mid, not x.
//   phase 2  y[px][co] = act2(bn2(sum_tap,cm mid[px + tap][cm] . W2[co][tap][cm])) + x[px][co]: an implicit GEMM whose B operand
//            is read from the LDS map (ds_read_b128, row stride C + 16 bytes: conflict-free) and whose A operand (weights)
//            streams from L2 through a register ring; wave w owns pixel rows 4 (w & 1) .. + 3 of the tile and half (w >> 1) of
//            the output channels, at most 4 x 4 fragments of accumulators at a time (two passes at C = 256).  The add is done in
//            fp32 on the accumulator, y is rounded once; x for the add is re-read (L2-hot: phase 1 has just read it).
// Both k-loops are unrolled completely and branch-free, as in ssdk_xpair.hip, so the compiler counts the loads in flight.
// Widths: C = 64 | 128 | 256 (LDS 15 / 27 / 51 KiB per workgroup: three workgroups per CU).  C = 512 needs 99 KiB (one workgroup
// of 4 waves per CU) and C = 1024 does not fit; those stages are MFMA-bound anyway and stay two launches (ssdk_dkres_supported).
#include "ssdk_conv_common.h"
#include "../../include/ssdk_dkres.h"

namespace ssdk {

struct DkresParams {
  const u16* x;
  u16* y;
  const u16* w1;
  const float* s1;
  const float* b1;
  const u16* w2;
  const float* s2;
  const float* b2;
  int H, W, tiles_y, tiles_x, act1, act2;
};

constexpr int kDkThreads = 256;
constexpr int kDkTH = SSDK_DKRES_TILE_H, kDkTW = SSDK_DKRES_TILE_W;
constexpr int kDkHW = kDkTW + 2;                  // width of the halo tile
constexpr int kDkHP = (kDkTH + 2) * (kDkTW + 2);  // 180 halo pixels
constexpr int kDkMF = 3;                          // pixel fragments per wave in phase 1: 4 waves x 3 x 16 = 192 LDS rows
constexpr int kDkRows = 4 * kDkMF * 16;
static_assert(kDkTW == 16 && kDkTH == 8 && kDkHP <= kDkRows, "tile");

// the activation as clamp bounds, set up once per phase: no branch per element (none: the value passes untouched)
struct DkAct {
  float lo, hi;
  bool on;
};
__device__ __forceinline__ DkAct dk_act_of(int act) {
  DkAct a;
  a.on = act == SSDK_ACT_RELU || act == SSDK_ACT_RELU6;
  a.lo = 0.f;
  a.hi = act == SSDK_ACT_RELU6 ? 6.f : __builtin_inff();
  return a;
}
__device__ __forceinline__ float dk_act(float v, const DkAct a) {
  const float c = __builtin_fminf(__builtin_fmaxf(v, a.lo), a.hi);
  return a.on ? c : v;
}

constexpr size_t dk_lds_bytes(int C) { return (size_t)kDkRows * (C + 16); }

// PK: both weight matrices come as fragment-major images (ssdk.h ssdk_weight_frag_bytes: 1 KiB contiguous per wave load)
template <int DT, int C, bool PK>
__global__ __launch_bounds__(kDkThreads) void dkres_kernel(const DkresParams p) {
  constexpr int CM = C / 2;                 // channels of the intermediate map
  constexpr int CS1 = C / 32;               // k-steps of the 1x1
  constexpr int CSM = CM / 32;              // 32-channel slices of the intermediate map
  constexpr int F1 = CM / 16;               // mid-channel fragments
  constexpr int NCM = F1 < 4 ? F1 : 4;      // ... per pass of phase 1
  constexpr int F2 = C / 32;                // output-channel fragments of a wave (half of C / 16)
  constexpr int NCO = F2 < 4 ? F2 : 4;      // ... per pass of phase 2
  constexpr int MS = CM * 2 + 16;           // LDS row stride of the intermediate map (bytes)
  constexpr int Q = 9 * CSM;                // k-steps of the 3x3
  constexpr int PF = 3;                     // weight ring of phase 2: k-steps ahead
  static_assert(F1 % NCM == 0 && F2 % NCO == 0 && CSM >= 1, "shape");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const u32 tid = threadIdx.x, lane = tid & 63u, wave = (u32)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
  const u32 fr = lane & 15u, fg = lane >> 4;
  int b = (int)blockIdx.x;
  const int tx0 = (b % p.tiles_x) * kDkTW;
  b /= p.tiles_x;
  const int ty0 = (b % p.tiles_y) * kDkTH;
  const int n = b / p.tiles_y;
  const int H = p.H, W = p.W;
  const size_t img = (size_t)n * H * W * C;
  const u16* xn = p.x + img;
  const DkAct act1 = dk_act_of(p.act1), act2 = dk_act_of(p.act2);

  // ---- phase 1: the 1x1 convolution on the tile and its halo ----------------------------------------------------------
  {
    const u16* xa[kDkMF];
    u32 row[kDkMF];
    bool inside[kDkMF];
#pragma unroll
    for (int m = 0; m < kDkMF; ++m) {
      const int hp = ((int)wave + 4 * m) * 16 + (int)fr;
      const int hy = hp / kDkHW, hx = hp - hy * kDkHW;
      int iy = ty0 - 1 + hy, ix = tx0 - 1 + hx;
      inside[m] = hp < kDkHP && (unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W;
      if (!inside[m]) iy = ty0, ix = tx0;  // computed on a pixel of the image, stored as zeros
      xa[m] = xn + ((size_t)iy * W + ix) * C + fg * 8;
      row[m] = (u32)hp * MS;
    }
#pragma unroll
    for (int ps = 0; ps < F1 / NCM; ++ps) {
      f32x4 acc[NCM][kDkMF];
#pragma unroll
      for (int a = 0; a < NCM; ++a)
#pragma unroll
        for (int m = 0; m < kDkMF; ++m) acc[a][m] = f32x4{0.f, 0.f, 0.f, 0.f};
      const u16* wa[NCM];
#pragma unroll
      for (int a = 0; a < NCM; ++a) {
        const int cf = ps * NCM + a;
        wa[a] = PK ? p.w1 + (size_t)cf * CS1 * 512 + lane * 8 : p.w1 + (size_t)(cf * 16 + (int)fr) * C + fg * 8;
      }
#pragma unroll
      for (int ks = 0; ks < CS1; ++ks) {
        u32x4 ra[NCM], rb[kDkMF];
#pragma unroll
        for (int a = 0; a < NCM; ++a) ra[a] = *reinterpret_cast<const u32x4*>(wa[a] + ks * (PK ? 512 : 32));
#pragma unroll
        for (int m = 0; m < kDkMF; ++m) rb[m] = *reinterpret_cast<const u32x4*>(xa[m] + ks * 32);
#pragma unroll
        for (int a = 0; a < NCM; ++a)
#pragma unroll
          for (int m = 0; m < kDkMF; ++m) acc[a][m] = mfma16<DT>(ra[a], rb[m], acc[a][m]);  // D[cm = 4fg + r][px = fr]
      }
#pragma unroll
      for (int a = 0; a < NCM; ++a) {
        const int cm = (ps * NCM + a) * 16 + (int)fg * 4;
        const f32x4 sc = *reinterpret_cast<const f32x4*>(p.s1 + cm), bi = *reinterpret_cast<const f32x4*>(p.b1 + cm);
#pragma unroll
        for (int m = 0; m < kDkMF; ++m) {
          float v[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) v[r] = inside[m] ? dk_act(acc[a][m][r] * sc[r] + bi[r], act1) : 0.f;
          *reinterpret_cast<uint2*>(smem + row[m] + cm * 2) = make_uint2(pack2_16<DT>(v[0], v[1]), pack2_16<DT>(v[2], v[3]));
        }
      }
    }
  }

  // ---- phase 2: the 3x3 convolution on the LDS map, + x -----------------------------------------------------------------
  const int pxh = (int)wave & 1, coh = (int)wave >> 1;
  u32 boff[4];  // LDS byte offset of tap (0, 0) of output pixel (row 4 pxh + m, column fr), this lane's 8 channels of slice 0
#pragma unroll
  for (int m = 0; m < 4; ++m) boff[m] = (u32)(((pxh * 4 + m) * kDkHW + (int)fr) * MS) + fg * 16u;
  __syncthreads();  // the intermediate map is complete
#pragma unroll
  for (int ps = 0; ps < F2 / NCO; ++ps) {
    const int cf0 = coh * F2 + ps * NCO;  // first output-channel fragment of this pass
    f32x4 acc[NCO][4];
#pragma unroll
    for (int a = 0; a < NCO; ++a)
#pragma unroll
      for (int m = 0; m < 4; ++m) acc[a][m] = f32x4{0.f, 0.f, 0.f, 0.f};
    const u16* wrow[NCO];
#pragma unroll
    for (int a = 0; a < NCO; ++a)
      wrow[a] = PK ? p.w2 + (size_t)(cf0 + a) * Q * 512 + lane * 8 : p.w2 + (size_t)((cf0 + a) * 16 + (int)fr) * 9 * CM + fg * 8;
    u32x4 rw[PF][NCO], rm[2][4];
    auto issue_w = [&](int slot, int q) {  // weights of k-step q = (tap, slice): K index tap * CM + 32 slice
#pragma unroll
      for (int a = 0; a < NCO; ++a) rw[slot][a] = *reinterpret_cast<const u32x4*>(wrow[a] + (size_t)q * (PK ? 512 : 32));
    };
    auto read_m = [&](int slot, int q) {
      const int t = q / CSM, s = q % CSM;
      const u32 off = (u32)(((t / 3) * kDkHW + t % 3) * MS + s * 64);
#pragma unroll
      for (int m = 0; m < 4; ++m) rm[slot][m] = *reinterpret_cast<const u32x4*>(smem + boff[m] + off);
    };
#pragma unroll
    for (int s = 0; s < PF; ++s) issue_w(s, s);
    read_m(0, 0);
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      if (q + 1 < Q) read_m((q + 1) & 1, q + 1);  // (compile-time conditions)
#pragma unroll
      for (int a = 0; a < NCO; ++a)
#pragma unroll
        for (int m = 0; m < 4; ++m) acc[a][m] = mfma16<DT>(rw[q % PF][a], rm[q & 1][m], acc[a][m]);  // D[co = 4fg + r][px = fr]
      if (q + PF < Q) issue_w(q % PF, q + PF);
      __builtin_amdgcn_sched_barrier(0);
    }
    const int ox = tx0 + (int)fr;
#pragma unroll
    for (int a = 0; a < NCO; ++a) {
      const int co = (cf0 + a) * 16 + (int)fg * 4;
      const f32x4 sc = *reinterpret_cast<const f32x4*>(p.s2 + co), bi = *reinterpret_cast<const f32x4*>(p.b2 + co);
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        const int oy = ty0 + pxh * 4 + m;
        if (oy < H && ox < W) {
          const size_t off = img + ((size_t)oy * W + ox) * C + co;
          const uint2 xv = *reinterpret_cast<const uint2*>(p.x + off);
          const float xr[4] = {bits16_to_f32<DT>(xv.x & 0xffffu), bits16_to_f32<DT>(xv.x >> 16), bits16_to_f32<DT>(xv.y & 0xffffu),
                               bits16_to_f32<DT>(xv.y >> 16)};
          float v[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) v[r] = dk_act(acc[a][m][r] * sc[r] + bi[r], act2) + xr[r];
          *reinterpret_cast<uint2*>(p.y + off) = make_uint2(pack2_16<DT>(v[0], v[1]), pack2_16<DT>(v[2], v[3]));
        }
      }
    }
  }
}

template <int DT, int C>
static void dk_launch(const DkresParams& p, bool packed, unsigned blocks, hipStream_t stream) {
  if (packed) hipLaunchKernelGGL((dkres_kernel<DT, C, true>), dim3(blocks), dim3(kDkThreads), dk_lds_bytes(C), stream, p);
  else hipLaunchKernelGGL((dkres_kernel<DT, C, false>), dim3(blocks), dim3(kDkThreads), dk_lds_bytes(C), stream, p);
}

}  // namespace ssdk

using namespace ssdk;

extern "C" size_t ssdk_dkres_desc_bytes(void) { return sizeof(ssdk_dkres_desc); }

extern "C" int ssdk_dkres_supported(int C, int H, int W, int dtype) {
  return (C == 64 || C == 128 || C == 256) && H >= 1 && W >= 1 && H <= 32768 && W <= 32768 && (dtype == SSDK_BF16 || dtype == SSDK_F16);
}

extern "C" int ssdk_dkres(const ssdk_dkres_desc* d, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!d) {
    set_error("dkres: null descriptor");
    return SSDK_E_BADARG;
  }
  if (!ssdk_dkres_supported(d->C, d->H, d->W, d->dtype)) {
    set_error("dkres: unsupported block C=%d H=%d W=%d dtype=%d (C 64 | 128 | 256, 1 <= H, W <= 32768, bf16 | f16)", d->C, d->H, d->W,
              d->dtype);
    return SSDK_E_BADARG;
  }
  const bool acts_ok = (d->act1 == SSDK_ACT_NONE || d->act1 == SSDK_ACT_RELU || d->act1 == SSDK_ACT_RELU6) &&
                       (d->act2 == SSDK_ACT_NONE || d->act2 == SSDK_ACT_RELU || d->act2 == SSDK_ACT_RELU6);
  if (!acts_ok) {
    set_error("dkres: act1=%d act2=%d (none, relu or relu6)", d->act1, d->act2);
    return SSDK_E_BADARG;
  }
  const int tiles_y = (d->H + kDkTH - 1) / kDkTH, tiles_x = (d->W + kDkTW - 1) / kDkTW;
  const long long blocks = (long long)d->N * tiles_y * tiles_x;
  if (d->N < 1 || blocks > 0x7fffffffLL) {
    set_error("dkres: N=%d with %d x %d tiles (N >= 1, fewer than 2^31 workgroups)", d->N, tiles_y, tiles_x);
    return SSDK_E_BADARG;
  }
  if (!d->x || !d->y || !d->w1 || !d->w2 || !d->scale1 || !d->bias1 || !d->scale2 || !d->bias2) {
    set_error("dkres: null pointer (x, y, w1, w2 and the four folded BN vectors are required)");
    return SSDK_E_BADARG;
  }
  if ((d->w1_frag == nullptr) != (d->w2_frag == nullptr)) {
    set_error("dkres: w1_frag and w2_frag come together or not at all");
    return SSDK_E_BADARG;
  }
  if (((uintptr_t)d->x | (uintptr_t)d->y | (uintptr_t)d->w1 | (uintptr_t)d->w2 | (uintptr_t)d->scale1 | (uintptr_t)d->bias1 |
       (uintptr_t)d->scale2 | (uintptr_t)d->bias2 | (uintptr_t)d->w1_frag | (uintptr_t)d->w2_frag) & 15) {
    set_error("dkres: every pointer must be 16-byte aligned");
    return SSDK_E_BADARG;
  }
  const size_t bytes = (size_t)d->N * d->H * d->W * d->C * 2;
  const uintptr_t xa = (uintptr_t)d->x, ya = (uintptr_t)d->y;
  if (xa < ya + bytes && ya < xa + bytes) {
    set_error("dkres: y overlaps x (a workgroup reads its neighbours' x: the block cannot run in place)");
    return SSDK_E_BADARG;
  }
  static const int env_pk = getenv("SSDK_WFRAG") ? atoi(getenv("SSDK_WFRAG")) : 1;
  const bool packed = d->w1_frag && d->w2_frag && env_pk != 0;
  DkresParams p;
  p.x = (const u16*)d->x;
  p.y = (u16*)d->y;
  p.w1 = (const u16*)(packed ? d->w1_frag : d->w1);
  p.s1 = d->scale1;
  p.b1 = d->bias1;
  p.w2 = (const u16*)(packed ? d->w2_frag : d->w2);
  p.s2 = d->scale2;
  p.b2 = d->bias2;
  p.H = d->H;
  p.W = d->W;
  p.tiles_y = tiles_y;
  p.tiles_x = tiles_x;
  p.act1 = d->act1;
  p.act2 = d->act2;
#define SSDK_DK(DT)                                                        \
  do {                                                                     \
    if (d->C == 64) dk_launch<DT, 64>(p, packed, (unsigned)blocks, stream);        \
    else if (d->C == 128) dk_launch<DT, 128>(p, packed, (unsigned)blocks, stream); \
    else dk_launch<DT, 256>(p, packed, (unsigned)blocks, stream);                  \
  } while (0)
  if (d->dtype == SSDK_BF16) SSDK_DK(SSDK_BF16);
  else SSDK_DK(SSDK_F16);
#undef SSDK_DK
  return check_launch("dkres_kernel");
}
