// ssdk_dconv.hip -- the dilated 3x3 convolution (dilation d, stride 1, padding d) + folded BN + activation of the BasicRFB extra
// layers (ssds/modeling/layers/rfb_layers.py) on gfx950 (include/ssdk_dconv.h).
//
// The convolution as a GEMM: rows = output pixels m of the flattened [N * H * W] index, k = tap * Cin + ci (tap = 3 ky + kx),
// Kpad = 32 * ceil(9 Cin / 32) -- the k order of the grouped image, so the weights come as the fragment-major image of [Cout][Kpad]
// (1 KiB contiguous per wave load, zero columns behind 9 Cin).  Cin % 8 == 0, so the 8 consecutive k one lane owns never straddle a
// tap: the pixel operand of a 16-pixel group is ONE 16-byte load per lane straight from the NHWC map -- no LDS staging and no halo
// tile (a halo of d = 5 around an 8 x 16 tile would stage 3.6 x the tile; the shipped maps are 8 x 8 and smaller and sit in L2).
//   * a lane whose source pixel is outside the image, whose k >= 9 Cin, or whose pixel is past the last one issues NO load: zeros;
//   * a k-step in which no lane of the wave has a source inside the image is skipped wave-uniformly, weights and MFMAs included
//     (a 4 x 4 map with d = 5 keeps the centre tap only: 9 x less work); it would have added exact zeros, so no bit changes.
// The shipped shapes have 512 ... 2048 pixel rows at batch 32, so 16 pixels x all of Cout per wave would leave most of 256 CUs
// idle: a workgroup owns 16 pixels x (NCO <= 4 fragments of 16 output channels), its 4 waves take the k-steps ks = wave, wave + 4,
// ... (interleaved, so the steps a border skips spread over the waves) and the partial accumulators meet in ONE LDS round, summed in
// a fixed order: wave a < NCO reduces fragment a, applies scale / bias / act and stores 8 bytes per lane.  NCO is chosen per launch
// so that the grid has at least one workgroup per CU; the loaded pixel operand stays in registers across the NCO MFMAs that use it.
#include "ssdk_conv_common.h"
#include "../../include/ssdk_dconv.h"

namespace ssdk {

struct DconvParams {
  const u16* x;
  const u16* wf;
  const float* scale;  // may be NULL: 1
  const float* bias;
  u16* y;
  int H, W, Cin, Cout, M, d, KS, G, cgs, relu;
};

constexpr int kDcSplit = SSDK_DCONV_KSPLIT;
constexpr int kDcThreads = 64 * kDcSplit;
static_assert(SSDK_DCONV_TILE_PIXELS == 16 && SSDK_DCONV_FRAG_COUT == 16 && SSDK_DCONV_TILE_COUT == 64 && kDcSplit == 4, "tile");

template <int DT, int NCO>
__global__ __launch_bounds__(kDcThreads) void dconv3x3_kernel(const DconvParams p) {
  __shared__ f32x4 part[kDcSplit][NCO][64];
  const u32 tid = threadIdx.x, lane = tid & 63u;
  const int wave = __builtin_amdgcn_readfirstlane((int)(tid >> 6));
  const u32 fr = lane & 15u, fg = lane >> 4;
  const int cg = (int)(blockIdx.x % (u32)p.cgs), pg = (int)(blockIdx.x / (u32)p.cgs);
  const int cf0 = cg * NCO;  // first output-channel fragment of this workgroup
  const int H = p.H, W = p.W, Cin = p.Cin, d = p.d;
  const int m = pg * 16 + (int)fr;  // this lane's output pixel (B operand row / accumulator column)
  const bool live = m < p.M;
  const int hw = H * W;
  const int mm = live ? m : 0;
  const int n = mm / hw, rem = mm - n * hw;
  const int oy = rem / W, ox = rem - oy * W;
  const u16* xn = p.x + (size_t)n * hw * Cin;
  f32x4 acc[NCO];
#pragma unroll
  for (int a = 0; a < NCO; ++a) acc[a] = f32x4{0.f, 0.f, 0.f, 0.f};
  const u16* wl = p.wf + (size_t)cf0 * p.KS * 512 + lane * 8;

  for (int ks = wave; ks < p.KS; ks += kDcSplit) {
    const int k0 = ks * 32 + (int)fg * 8;  // this lane's 8 consecutive k: one tap, channels ci .. ci + 7
    const int tap = k0 / Cin, ci = k0 - tap * Cin;
    const int ky = tap / 3, kx = tap - 3 * ky;
    const int iy = oy + d * (ky - 1), ix = ox + d * (kx - 1);
    const bool ok = live && tap < 9 && (unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W;
    if (__builtin_amdgcn_ballot_w64(ok) == 0) continue;  // wave-uniform: nothing of this k-step is inside the image
    u32x4 b = u32x4{0u, 0u, 0u, 0u};
    if (ok) b = *reinterpret_cast<const u32x4*>(xn + ((size_t)iy * W + ix) * Cin + ci);  // (no load outside the image)
    u32x4 wa[NCO];
#pragma unroll
    for (int a = 0; a < NCO; ++a)
      if (cf0 + a < p.G) wa[a] = *reinterpret_cast<const u32x4*>(wl + ((size_t)a * p.KS + ks) * 512);
#pragma unroll
    for (int a = 0; a < NCO; ++a)
      if (cf0 + a < p.G) acc[a] = mfma16<DT>(wa[a], b, acc[a]);  // D[co = 4fg + r][px = fr]
  }

#pragma unroll
  for (int a = 0; a < NCO; ++a) part[wave][a][lane] = acc[a];
  __syncthreads();
  if (wave < NCO && cf0 + wave < p.G) {
    const int a = wave;
    const f32x4 s = (part[0][a][lane] + part[1][a][lane]) + (part[2][a][lane] + part[3][a][lane]);
    const int co = (cf0 + a) * 16 + (int)fg * 4;
    if (live && co < p.Cout) {  // (Cout % 8 == 0: the four channels are inside together)
      const f32x4 bi = *reinterpret_cast<const f32x4*>(p.bias + co);
      f32x4 sc = f32x4{1.f, 1.f, 1.f, 1.f};
      if (p.scale) sc = *reinterpret_cast<const f32x4*>(p.scale + co);
      float v[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        v[r] = s[r] * sc[r] + bi[r];
        if (p.relu) v[r] = __builtin_fmaxf(v[r], 0.f);
      }
      *reinterpret_cast<uint2*>(p.y + (size_t)m * p.Cout + co) = make_uint2(pack2_16<DT>(v[0], v[1]), pack2_16<DT>(v[2], v[3]));
    }
  }
}

template <int DT>
static void dc_launch(const DconvParams& p, int nco, unsigned blocks, hipStream_t stream) {
  if (nco == 4) hipLaunchKernelGGL((dconv3x3_kernel<DT, 4>), dim3(blocks), dim3(kDcThreads), 0, stream, p);
  else if (nco == 2) hipLaunchKernelGGL((dconv3x3_kernel<DT, 2>), dim3(blocks), dim3(kDcThreads), 0, stream, p);
  else hipLaunchKernelGGL((dconv3x3_kernel<DT, 1>), dim3(blocks), dim3(kDcThreads), 0, stream, p);
}

}  // namespace ssdk

using namespace ssdk;

extern "C" int ssdk_dconv3x3_supported(int Cin, int Cout, int H, int W, int dilation, int dtype) {
  return Cin >= 8 && Cout >= 8 && Cin <= SSDK_DCONV_MAX_CHANNELS && Cout <= SSDK_DCONV_MAX_CHANNELS && Cin % 8 == 0 && Cout % 8 == 0 &&
         dilation >= SSDK_DCONV_MIN_DILATION && dilation <= SSDK_DCONV_MAX_DILATION && H >= 1 && W >= 1 && H <= SSDK_DCONV_MAX_SIDE &&
         W <= SSDK_DCONV_MAX_SIDE && (dtype == SSDK_BF16 || dtype == SSDK_F16);
}

extern "C" int ssdk_dconv3x3(const ssdk_conv_desc* c, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!c) {
    set_error("dconv3x3: null descriptor");
    return SSDK_E_BADARG;
  }
  const int dil = ((c->res_mode & SSDK_CONV_DILATION_MASK) >> SSDK_CONV_DILATION_SHIFT) + 1;
  if (c->res_mode & ~SSDK_CONV_DILATION_MASK) {
    set_error("dconv3x3: res_mode=%d (only the dilation bits 8-11 may be set: a dilated convolution takes no residual)", c->res_mode);
    return SSDK_E_BADARG;
  }
  if (c->k != 3 || c->stride != 1 || c->groups > 1 || c->in_layout != SSDK_LAYOUT_NHWC || c->out_layout != SSDK_LAYOUT_NHWC) {
    set_error("dconv3x3: dilation %d with k=%d stride=%d groups=%d layouts %d/%d (a dilated convolution is k 3, stride 1, groups 1, NHWC "
              "in and out)", dil, c->k, c->stride, c->groups, c->in_layout, c->out_layout);
    return SSDK_E_BADARG;
  }
  if (c->residual || c->y2) {
    set_error("dconv3x3: dilation %d with %s (a dilated convolution has one output and no residual)", dil,
              c->residual ? "a residual" : "a second output y2");
    return SSDK_E_BADARG;
  }
  if (!c->w_frag) {
    set_error("dconv3x3: dilation %d without w_frag (the kernel reads the fragment-major image of [Cout][32 * ceil(9 Cin / 32)] only)", dil);
    return SSDK_E_BADARG;
  }
  if (!ssdk_dconv3x3_supported(c->Cin, c->Cout, c->H, c->W, dil, c->dtype)) {
    set_error("dconv3x3: unsupported layer Cin=%d Cout=%d H=%d W=%d dilation=%d dtype=%d (Cin, Cout multiples of 8 from 8 to %d, "
              "dilation %d ... %d, 1 <= H, W <= %d, bf16 | f16)", c->Cin, c->Cout, c->H, c->W, dil, c->dtype, SSDK_DCONV_MAX_CHANNELS,
              SSDK_DCONV_MIN_DILATION, SSDK_DCONV_MAX_DILATION, SSDK_DCONV_MAX_SIDE);
    return SSDK_E_BADARG;
  }
  if (c->act != SSDK_ACT_NONE && c->act != SSDK_ACT_RELU) {
    set_error("dconv3x3: act=%d (none or relu)", c->act);
    return SSDK_E_BADARG;
  }
  const long long M = (long long)c->N * c->H * c->W;
  const int G = (c->Cout + 15) / 16;
  const long long groups = (M + 15) / 16;
  if (c->N < 1 || M >= (1ll << 31) || groups * G > 0x7fffffffLL) {
    set_error("dconv3x3: N=%d on %d x %d (N >= 1, fewer than 2^31 output pixels and workgroups)", c->N, c->H, c->W);
    return SSDK_E_BADARG;
  }
  if (!c->x || !c->y || !c->w || !c->bias) {
    set_error("dconv3x3: null pointer (x, y, w, w_frag and bias are required)");
    return SSDK_E_BADARG;
  }
  if (((uintptr_t)c->x | (uintptr_t)c->y | (uintptr_t)c->w | (uintptr_t)c->w_frag | (uintptr_t)c->scale | (uintptr_t)c->bias) & 15) {
    set_error("dconv3x3: every pointer must be 16-byte aligned");
    return SSDK_E_BADARG;
  }
  const uintptr_t xa = (uintptr_t)c->x, ya = (uintptr_t)c->y;
  if (xa < ya + (size_t)M * c->Cout * 2 && ya < xa + (size_t)M * c->Cin * 2) {
    set_error("dconv3x3: y overlaps x (a workgroup reads its neighbours' x: the layer cannot run in place)");
    return SSDK_E_BADARG;
  }
  // output-channel fragments per workgroup: as many as still leave every CU a workgroup (the pixel operand is loaded once per
  // workgroup and k-step, whatever NCO is)
  int nco = 1;
  if (groups * ((G + 3) / 4) >= 512) nco = 4;
  else if (groups * ((G + 1) / 2) >= 256) nco = 2;
  DconvParams p;
  p.x = (const u16*)c->x;
  p.wf = (const u16*)c->w_frag;
  p.scale = c->scale;
  p.bias = c->bias;
  p.y = (u16*)c->y;
  p.H = c->H;
  p.W = c->W;
  p.Cin = c->Cin;
  p.Cout = c->Cout;
  p.M = (int)M;
  p.d = dil;
  p.KS = (9 * c->Cin + 31) / 32;
  p.G = G;
  p.cgs = (G + nco - 1) / nco;
  p.relu = c->act == SSDK_ACT_RELU;
  const unsigned blocks = (unsigned)(groups * p.cgs);
  if (c->dtype == SSDK_BF16) dc_launch<SSDK_BF16>(p, nco, blocks, stream);
  else dc_launch<SSDK_F16>(p, nco, blocks, stream);
  return check_launch("dconv3x3_kernel");
}
