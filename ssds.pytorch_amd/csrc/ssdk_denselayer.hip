// ssdk_denselayer.hip -- one DenseNet dense layer (nets/densenet.py _DenseLayer: BN + ReLU, Conv 1x1 Cin -> 128, BN + ReLU, Conv 3x3 /
// pad 1 128 -> 32, the result concatenated behind the input) as ONE launch on gfx950, plus the two small kernels a dense block needs
// around it: the front of a transition (BN + ReLU + 2x2 average) and the copy that places a dense map into a block's buffer
// (include/ssdk_denselayer.h).
//
// Why: a dense block of L layers on library kernels re-concatenates everything before each layer (traffic quadratic in L), runs two
// BatchNorm + ReLU passes over stored tensors and writes a 128-channel middle map that only the next convolution reads.  Here the
// block owns ONE buffer [N][H][W][ld]; layer j reads channels [0, Cin) of it and writes [Cin, Cin + 32): "read Cin, write 32" per
// pixel, the algorithmic minimum.  The structure is ssdk_dkres.hip's.  A workgroup (4 waves) owns (image, tile of kDnTH x kDnTW
// output pixels):
//   phase 1  m[hp][cm] = relu(bn2(relu(bn1(x[hp][:])) . W1[cm][:])) on the tile PLUS its one-pixel halo (180 pixels padded to 12
//            fragments of 16; wave w owns fragments w, w + 4, w + 8) for all 128 middle channels at once: 8 x 3 accumulator
//            fragments per wave, ONE pass over x.  norm1 + ReLU is a different affine per consuming layer, so it cannot be folded
//            into a producer: it is applied in fp32 to the x fragment between its load and the MFMA (unpack, mul, add, max, pack:
//            the B operand is what a stored relu(bn1(x)) tensor would hold).  x and (a, b) of the next k-step are in flight while
//            this one computes; each weight fragment is refilled in place behind its last MFMA.  A halo position OUTSIDE THE IMAGE
//            gets ZEROS, not relu(bias1): the 3x3 pads m, not x -- and relu(b) of an absent pixel is not zero either.
//   phase 2  y[px][co] = sum_tap,cm m[px + tap][cm] . W2[co][tap][cm] from the LDS map (row stride 256 + 16 bytes: conflict-free
//            ds_read_b128), weights streamed from L2 through a register ring; wave w owns pixel rows 4 (w & 1) .. + 3 and output
//            channels 16 (w >> 1) .. + 15.  Rounded once, stored with pixel stride ld at y.
// LDS 192 x 272 B = 51 KiB per workgroup; __launch_bounds__(256, 2) asks for two waves per SIMD, so that one wave's pre-activation
// VALU work runs under another's MFMAs.
#include "ssdk_conv_common.h"
#include "../../include/ssdk_denselayer.h"

namespace ssdk {

struct DenseParams {
  const u16* x;
  u16* y;
  const u16* w1;
  const float* a;
  const float* b;
  const float* s1;
  const float* b1;
  const u16* w2;
  int H, W, tiles_y, tiles_x, Cin, ld;
};

constexpr int kDnThreads = 256;
constexpr int kDnTH = SSDK_DENSE_TILE_H, kDnTW = SSDK_DENSE_TILE_W;
constexpr int kDnCM = SSDK_DENSE_CMID, kDnCO = SSDK_DENSE_COUT;
constexpr int kDnHW = kDnTW + 2;                  // width of the halo tile
constexpr int kDnHP = (kDnTH + 2) * (kDnTW + 2);  // 180 halo pixels
constexpr int kDnMF = 3;                          // pixel fragments per wave in phase 1: 4 waves x 3 x 16 = 192 LDS rows
constexpr int kDnRows = 4 * kDnMF * 16;
constexpr int kDnF1 = kDnCM / 16;                 // 8 middle-channel fragments
constexpr int kDnMS = kDnCM * 2 + 16;             // LDS row stride of the middle map (bytes)
constexpr size_t kDnLds = (size_t)kDnRows * kDnMS;
static_assert(kDnTW == 16 && kDnTH == 8 && kDnHP <= kDnRows && kDnCM == 128 && kDnCO == 32, "tile");

// relu(a * x + b) on the 8 channels of an operand fragment, fp32, rounded once to the tensor dtype (-ffp-contract=off: mul, then add)
template <int DT>
__device__ __forceinline__ u32x4 dn_preact(const u32x4 v, const f32x4 a0, const f32x4 a1, const f32x4 b0, const f32x4 b1) {
  u32x4 o;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float al = j < 2 ? a0[2 * j] : a1[2 * j - 4], ah = j < 2 ? a0[2 * j + 1] : a1[2 * j - 3];
    const float bl = j < 2 ? b0[2 * j] : b1[2 * j - 4], bh = j < 2 ? b0[2 * j + 1] : b1[2 * j - 3];
    const float lo = __builtin_fmaxf(bits16_to_f32<DT>(v[j] & 0xffffu) * al + bl, 0.f);
    const float hi = __builtin_fmaxf(bits16_to_f32<DT>(v[j] >> 16) * ah + bh, 0.f);
    o[j] = pack2_16<DT>(lo, hi);
  }
  return o;
}

struct DnStage {  // the x fragments and the affine of one k-step (32 input channels)
  u32x4 x[kDnMF];
  f32x4 a0, a1, b0, b1;
};

// PK: both weight matrices come as fragment-major images (ssdk.h ssdk_weight_frag_bytes: 1 KiB contiguous per wave load)
template <int DT, bool PK>
__global__ __launch_bounds__(kDnThreads, 2) void dense_layer_kernel(const DenseParams p) {
  constexpr int CSM = kDnCM / 32;  // 32-channel slices of the middle map
  constexpr int Q = 9 * CSM;       // k-steps of the 3x3
  constexpr int PF = 3;            // weight ring of phase 2: k-steps ahead
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const u32 tid = threadIdx.x, lane = tid & 63u, wave = (u32)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
  const u32 fr = lane & 15u, fg = lane >> 4;
  int blk = (int)blockIdx.x;
  const int tx0 = (blk % p.tiles_x) * kDnTW;
  blk /= p.tiles_x;
  const int ty0 = (blk % p.tiles_y) * kDnTH;
  const int n = blk / p.tiles_y;
  const int H = p.H, W = p.W, Cin = p.Cin, CS1 = p.Cin >> 5;
  const size_t ld = (size_t)p.ld, img = (size_t)n * H * W * ld;

  // ---- phase 1: relu(bn1(x)) -> 1x1 -> relu(bn2(.)) on the tile and its halo --------------------------------------------
  {
    const u16* xa[kDnMF];
    u32 row[kDnMF];
    bool inside[kDnMF];
#pragma unroll
    for (int m = 0; m < kDnMF; ++m) {
      const int hp = ((int)wave + 4 * m) * 16 + (int)fr;
      const int hy = hp / kDnHW, hx = hp - hy * kDnHW;
      int iy = ty0 - 1 + hy, ix = tx0 - 1 + hx;
      inside[m] = hp < kDnHP && (unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W;
      if (!inside[m]) iy = ty0, ix = tx0;  // computed on a pixel of the image, stored as zeros
      xa[m] = p.x + img + ((size_t)iy * W + ix) * ld + fg * 8;
      row[m] = (u32)hp * kDnMS;
    }
    const float* pa = p.a + fg * 8;
    const float* pb = p.b + fg * 8;
    // weight fragment cf of k-step ks
    const u16* wa = PK ? p.w1 + lane * 8 : p.w1 + (size_t)fr * Cin + fg * 8;
    const size_t wcf = PK ? (size_t)CS1 * 512 : (size_t)16 * Cin;
    constexpr int wks = PK ? 512 : 32;
    f32x4 acc[kDnF1][kDnMF];
#pragma unroll
    for (int a = 0; a < kDnF1; ++a)
#pragma unroll
      for (int m = 0; m < kDnMF; ++m) acc[a][m] = f32x4{0.f, 0.f, 0.f, 0.f};
    auto load_stage = [&](DnStage& s, int ks) {
#pragma unroll
      for (int m = 0; m < kDnMF; ++m) s.x[m] = *reinterpret_cast<const u32x4*>(xa[m] + ks * 32);
      s.a0 = *reinterpret_cast<const f32x4*>(pa + ks * 32);
      s.a1 = *reinterpret_cast<const f32x4*>(pa + ks * 32 + 4);
      s.b0 = *reinterpret_cast<const f32x4*>(pb + ks * 32);
      s.b1 = *reinterpret_cast<const f32x4*>(pb + ks * 32 + 4);
    };
    u32x4 rw[kDnF1];
#pragma unroll
    for (int a = 0; a < kDnF1; ++a) rw[a] = *reinterpret_cast<const u32x4*>(wa + a * wcf);
    auto compute = [&](const DnStage& s, int ks) {  // ks: this k-step; its weights are in rw, which is refilled for ks + 1
      u32x4 xb[kDnMF];
#pragma unroll
      for (int m = 0; m < kDnMF; ++m) xb[m] = dn_preact<DT>(s.x[m], s.a0, s.a1, s.b0, s.b1);
      const bool more = ks + 1 < CS1;  // (uniform)
#pragma unroll
      for (int a = 0; a < kDnF1; ++a) {
#pragma unroll
        for (int m = 0; m < kDnMF; ++m) acc[a][m] = mfma16<DT>(rw[a], xb[m], acc[a][m]);  // D[cm = 4fg + r][px = fr]
        if (more) rw[a] = *reinterpret_cast<const u32x4*>(wa + a * wcf + (size_t)(ks + 1) * wks);
      }
    };
    DnStage s0, s1;
    load_stage(s0, 0);
    for (int ks = 0; ks < CS1; ks += 2) {
      if (ks + 1 < CS1) load_stage(s1, ks + 1);
      compute(s0, ks);
      if (ks + 1 < CS1) {
        if (ks + 2 < CS1) load_stage(s0, ks + 2);
        compute(s1, ks + 1);
      }
    }
#pragma unroll
    for (int a = 0; a < kDnF1; ++a) {
      const int cm = a * 16 + (int)fg * 4;
      const f32x4 sc = *reinterpret_cast<const f32x4*>(p.s1 + cm), bi = *reinterpret_cast<const f32x4*>(p.b1 + cm);
#pragma unroll
      for (int m = 0; m < kDnMF; ++m) {
        float v[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = inside[m] ? __builtin_fmaxf(acc[a][m][r] * sc[r] + bi[r], 0.f) : 0.f;
        *reinterpret_cast<uint2*>(smem + row[m] + cm * 2) = make_uint2(pack2_16<DT>(v[0], v[1]), pack2_16<DT>(v[2], v[3]));
      }
    }
  }

  // ---- phase 2: the 3x3 convolution on the LDS map ---------------------------------------------------------------------
  const int pxh = (int)wave & 1, cf = (int)wave >> 1;  // pixel rows 4 pxh .. + 3, output-channel fragment cf
  u32 boff[4];  // LDS byte offset of tap (0, 0) of output pixel (row 4 pxh + m, column fr), this lane's 8 channels of slice 0
#pragma unroll
  for (int m = 0; m < 4; ++m) boff[m] = (u32)(((pxh * 4 + m) * kDnHW + (int)fr) * kDnMS) + fg * 16u;
  __syncthreads();  // the middle map is complete
  f32x4 acc[4];
#pragma unroll
  for (int m = 0; m < 4; ++m) acc[m] = f32x4{0.f, 0.f, 0.f, 0.f};
  const u16* wrow = PK ? p.w2 + (size_t)cf * Q * 512 + lane * 8 : p.w2 + (size_t)(cf * 16 + (int)fr) * 9 * kDnCM + fg * 8;
  u32x4 rw[PF], rm[2][4];
  auto issue_w = [&](int slot, int q) {  // weights of k-step q = (tap, slice): K index tap * 128 + 32 slice
    rw[slot] = *reinterpret_cast<const u32x4*>(wrow + (size_t)q * (PK ? 512 : 32));
  };
  auto read_m = [&](int slot, int q) {
    const int t = q / CSM, s = q % CSM;
    const u32 off = (u32)(((t / 3) * kDnHW + t % 3) * kDnMS + s * 64);
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
    for (int m = 0; m < 4; ++m) acc[m] = mfma16<DT>(rw[q % PF], rm[q & 1][m], acc[m]);  // D[co = 4fg + r][px = fr]
    if (q + PF < Q) issue_w(q % PF, q + PF);
    __builtin_amdgcn_sched_barrier(0);
  }
  const int ox = tx0 + (int)fr, co = cf * 16 + (int)fg * 4;
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    const int oy = ty0 + pxh * 4 + m;
    if (oy < H && ox < W)
      *reinterpret_cast<uint2*>(p.y + img + ((size_t)oy * W + ox) * ld + co) =
          make_uint2(pack2_16<DT>(acc[m][0], acc[m][1]), pack2_16<DT>(acc[m][2], acc[m][3]));
  }
}

// ---- the front of a transition: relu(a x + b), 2x2 average; one lane per (output pixel, 8 channels) --------------------------
struct DensePoolParams {
  const u16* x;
  u16* y;
  const float* a;
  const float* b;
  int H, W, Ho, Wo, C8;
  size_t ld, total;
};

template <int DT>
__global__ __launch_bounds__(256) void dense_pool_kernel(const DensePoolParams p) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= p.total) return;
  const int c8 = (int)(i % (size_t)p.C8);
  size_t px = i / (size_t)p.C8;
  const int ox = (int)(px % (size_t)p.Wo);
  px /= (size_t)p.Wo;
  const int oy = (int)(px % (size_t)p.Ho);
  const size_t n = px / (size_t)p.Ho;
  const f32x4 a0 = *reinterpret_cast<const f32x4*>(p.a + c8 * 8), a1 = *reinterpret_cast<const f32x4*>(p.a + c8 * 8 + 4);
  const f32x4 b0 = *reinterpret_cast<const f32x4*>(p.b + c8 * 8), b1 = *reinterpret_cast<const f32x4*>(p.b + c8 * 8 + 4);
  const float av[8] = {a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3]};
  const float bv[8] = {b0[0], b0[1], b0[2], b0[3], b1[0], b1[1], b1[2], b1[3]};
  float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int dy = 0; dy < 2; ++dy)
#pragma unroll
    for (int dx = 0; dx < 2; ++dx) {
      const u32x4 v = *reinterpret_cast<const u32x4*>(p.x + ((n * p.H + (size_t)(2 * oy + dy)) * p.W + (size_t)(2 * ox + dx)) * p.ld + c8 * 8);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        s[2 * j] += __builtin_fmaxf(bits16_to_f32<DT>(v[j] & 0xffffu) * av[2 * j] + bv[2 * j], 0.f);
        s[2 * j + 1] += __builtin_fmaxf(bits16_to_f32<DT>(v[j] >> 16) * av[2 * j + 1] + bv[2 * j + 1], 0.f);
      }
    }
  u32x4 o;
#pragma unroll
  for (int j = 0; j < 4; ++j) o[j] = pack2_16<DT>(s[2 * j] * 0.25f, s[2 * j + 1] * 0.25f);
  *reinterpret_cast<u32x4*>(p.y + i * 8) = o;
}

// ---- dense [pixels][C] -> channels [0, C) of a buffer with pixel stride ld; one lane per 16 bytes ---------------------------------
__global__ __launch_bounds__(256) void dense_place_kernel(const u16* __restrict__ x, u16* __restrict__ y, int C8, size_t ld, size_t total) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const size_t px = i / (size_t)C8, c8 = i % (size_t)C8;
  *reinterpret_cast<u32x4*>(y + px * ld + c8 * 8) = *reinterpret_cast<const u32x4*>(x + i * 8);
}

static bool dn_ranges_overlap(uintptr_t a, size_t na, uintptr_t b, size_t nb) { return a < b + nb && b < a + na; }

}  // namespace ssdk

using namespace ssdk;

extern "C" size_t ssdk_dense_layer_desc_bytes(void) { return sizeof(ssdk_dense_layer_desc); }
extern "C" size_t ssdk_dense_pool_desc_bytes(void) { return sizeof(ssdk_dense_pool_desc); }
extern "C" size_t ssdk_dense_place_desc_bytes(void) { return sizeof(ssdk_dense_place_desc); }

extern "C" int ssdk_dense_layer_supported(int Cin, int H, int W, int ld, int dtype) {
  return Cin % 32 == 0 && Cin >= 32 && Cin <= 2048 && ld % 8 == 0 && (long long)ld >= (long long)Cin + kDnCO && H >= 1 && W >= 1 &&
         H <= 32768 && W <= 32768 && (dtype == SSDK_BF16 || dtype == SSDK_F16);
}

extern "C" int ssdk_dense_layer(const ssdk_dense_layer_desc* d, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!d) {
    set_error("dense_layer: null descriptor");
    return SSDK_E_BADARG;
  }
  if (!ssdk_dense_layer_supported(d->Cin, d->H, d->W, d->ld, d->dtype)) {
    set_error("dense_layer: unsupported layer Cin=%d H=%d W=%d ld=%d dtype=%d (Cin %% 32 == 0, 32 <= Cin <= 2048, ld %% 8 == 0, "
              "ld >= Cin + 32, 1 <= H, W <= 32768, bf16 | f16)", d->Cin, d->H, d->W, d->ld, d->dtype);
    return SSDK_E_BADARG;
  }
  const int tiles_y = (d->H + kDnTH - 1) / kDnTH, tiles_x = (d->W + kDnTW - 1) / kDnTW;
  const long long blocks = (long long)d->N * tiles_y * tiles_x;
  if (d->N < 1 || blocks > 0x7fffffffLL) {
    set_error("dense_layer: N=%d with %d x %d tiles (N >= 1, fewer than 2^31 workgroups)", d->N, tiles_y, tiles_x);
    return SSDK_E_BADARG;
  }
  if (!d->x || !d->y || !d->w1 || !d->w2 || !d->a || !d->b || !d->scale1 || !d->bias1) {
    set_error("dense_layer: null pointer (x, y, w1, w2, a, b, scale1 and bias1 are required)");
    return SSDK_E_BADARG;
  }
  if ((d->w1_frag == nullptr) != (d->w2_frag == nullptr)) {
    set_error("dense_layer: w1_frag and w2_frag come together or not at all");
    return SSDK_E_BADARG;
  }
  if (((uintptr_t)d->x | (uintptr_t)d->y | (uintptr_t)d->w1 | (uintptr_t)d->w2 | (uintptr_t)d->a | (uintptr_t)d->b |
       (uintptr_t)d->scale1 | (uintptr_t)d->bias1 | (uintptr_t)d->w1_frag | (uintptr_t)d->w2_frag) & 15) {
    set_error("dense_layer: every pointer must be 16-byte aligned");
    return SSDK_E_BADARG;
  }
  // y may live in x's buffer, but no written channel may be a read one: other workgroups read x while this one writes y
  const size_t px = (size_t)d->N * d->H * d->W;
  const uintptr_t xa = (uintptr_t)d->x, ya = (uintptr_t)d->y;
  if (dn_ranges_overlap(xa, ((px - 1) * d->ld + d->Cin) * 2, ya, ((px - 1) * d->ld + kDnCO) * 2)) {
    const long long ldb = 2LL * d->ld;
    long long off = ((long long)ya - (long long)xa) % ldb;
    if (off < 0) off += ldb;
    if (off < 2LL * d->Cin || off + 2LL * kDnCO > ldb) {
      set_error("dense_layer: y's 32 channels overlap the %d channels x is read from (channel offset %lld of pixel stride %d)",
                d->Cin, off / 2, d->ld);
      return SSDK_E_BADARG;
    }
  }
  static const int env_pk = getenv("SSDK_WFRAG") ? atoi(getenv("SSDK_WFRAG")) : 1;
  const bool packed = d->w1_frag && d->w2_frag && env_pk != 0;
  DenseParams p;
  p.x = (const u16*)d->x;
  p.y = (u16*)d->y;
  p.w1 = (const u16*)(packed ? d->w1_frag : d->w1);
  p.a = d->a;
  p.b = d->b;
  p.s1 = d->scale1;
  p.b1 = d->bias1;
  p.w2 = (const u16*)(packed ? d->w2_frag : d->w2);
  p.H = d->H;
  p.W = d->W;
  p.tiles_y = tiles_y;
  p.tiles_x = tiles_x;
  p.Cin = d->Cin;
  p.ld = d->ld;
#define SSDK_DN(DT)                                                                                                              \
  do {                                                                                                                           \
    if (packed) hipLaunchKernelGGL((dense_layer_kernel<DT, true>), dim3((unsigned)blocks), dim3(kDnThreads), kDnLds, stream, p); \
    else hipLaunchKernelGGL((dense_layer_kernel<DT, false>), dim3((unsigned)blocks), dim3(kDnThreads), kDnLds, stream, p);       \
  } while (0)
  if (d->dtype == SSDK_BF16) SSDK_DN(SSDK_BF16);
  else SSDK_DN(SSDK_F16);
#undef SSDK_DN
  return check_launch("dense_layer_kernel");
}

// shared argument rules of the pool and the place: a dense tensor of C channels and a buffer of pixel stride ld
static int dn_check_strided(const char* who, int N, int H, int W, int C, int ld, int dtype, int hw_min) {
  if (!(C % 8 == 0 && C >= 8 && ld % 8 == 0 && ld >= C && H >= hw_min && W >= hw_min && H <= 32768 && W <= 32768 && N >= 1 &&
        (dtype == SSDK_BF16 || dtype == SSDK_F16))) {
    set_error("%s: N=%d H=%d W=%d C=%d ld=%d dtype=%d (C %% 8 == 0, 8 <= C <= ld, ld %% 8 == 0, %d <= H, W <= 32768, N >= 1, bf16 | f16)",
              who, N, H, W, C, ld, dtype, hw_min);
    return SSDK_E_BADARG;
  }
  return SSDK_OK;
}

extern "C" int ssdk_dense_pool(const ssdk_dense_pool_desc* d, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!d) {
    set_error("dense_pool: null descriptor");
    return SSDK_E_BADARG;
  }
  if (int rc = dn_check_strided("dense_pool", d->N, d->H, d->W, d->C, d->ld, d->dtype, 2)) return rc;
  if (!d->x || !d->y || !d->a || !d->b) {
    set_error("dense_pool: null pointer (x, y, a and b are required)");
    return SSDK_E_BADARG;
  }
  if (((uintptr_t)d->x | (uintptr_t)d->y | (uintptr_t)d->a | (uintptr_t)d->b) & 15) {
    set_error("dense_pool: every pointer must be 16-byte aligned");
    return SSDK_E_BADARG;
  }
  const int Ho = d->H / 2, Wo = d->W / 2;
  const size_t total = (size_t)d->N * Ho * Wo * (d->C / 8);
  const size_t blocks = (total + 255) / 256;
  if (blocks > 0x7fffffffULL) {
    set_error("dense_pool: %zu workgroups (fewer than 2^31)", blocks);
    return SSDK_E_BADARG;
  }
  if (dn_ranges_overlap((uintptr_t)d->x, (((size_t)d->N * d->H * d->W - 1) * d->ld + d->C) * 2, (uintptr_t)d->y, total * 16)) {
    set_error("dense_pool: y overlaps the buffer x is read from");
    return SSDK_E_BADARG;
  }
  DensePoolParams p;
  p.x = (const u16*)d->x;
  p.y = (u16*)d->y;
  p.a = d->a;
  p.b = d->b;
  p.H = d->H;
  p.W = d->W;
  p.Ho = Ho;
  p.Wo = Wo;
  p.C8 = d->C / 8;
  p.ld = (size_t)d->ld;
  p.total = total;
  if (d->dtype == SSDK_BF16) hipLaunchKernelGGL((dense_pool_kernel<SSDK_BF16>), dim3((unsigned)blocks), dim3(256), 0, stream, p);
  else hipLaunchKernelGGL((dense_pool_kernel<SSDK_F16>), dim3((unsigned)blocks), dim3(256), 0, stream, p);
  return check_launch("dense_pool_kernel");
}

extern "C" int ssdk_dense_place(const ssdk_dense_place_desc* d, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!d) {
    set_error("dense_place: null descriptor");
    return SSDK_E_BADARG;
  }
  if (int rc = dn_check_strided("dense_place", d->N, d->H, d->W, d->C, d->ld, d->dtype, 1)) return rc;
  if (!d->x || !d->y) {
    set_error("dense_place: null pointer (x and y are required)");
    return SSDK_E_BADARG;
  }
  if (((uintptr_t)d->x | (uintptr_t)d->y) & 15) {
    set_error("dense_place: every pointer must be 16-byte aligned");
    return SSDK_E_BADARG;
  }
  const size_t px = (size_t)d->N * d->H * d->W;
  const size_t total = px * (d->C / 8);
  const size_t blocks = (total + 255) / 256;
  if (blocks > 0x7fffffffULL) {
    set_error("dense_place: %zu workgroups (fewer than 2^31)", blocks);
    return SSDK_E_BADARG;
  }
  if (dn_ranges_overlap((uintptr_t)d->x, total * 16, (uintptr_t)d->y, ((px - 1) * d->ld + d->C) * 2)) {
    set_error("dense_place: x overlaps the buffer y lives in");
    return SSDK_E_BADARG;
  }
  hipLaunchKernelGGL(dense_place_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, (const u16*)d->x, (u16*)d->y, d->C / 8,
                     (size_t)d->ld, total);
  return check_launch("dense_place_kernel");
}
