// ssdk_gconv_any.hip -- grouped 3x3 convolution for any group width gw (+ folded BN + activation) on gfx950.
//
// Reference: the bottleneck 3x3 of RegNetX (ssds/modeling/nets/regnet.py: `b = Conv2d(w_b, w_b, 3, stride, groups = w_b / gw)`)
// and of ResNeXt (nets/resnet.py: Bottleneck.conv2 with groups = 32).  ssdk_gconv.hip keeps gw = 16; this file takes every
// other width: gw a multiple of 8 from 8 to 256 (gw = 4 arrives here as 8: the packer merges neighbouring groups into
// block-diagonal ones, fused_conv.pack_grouped_frag).  Same contract as launch_gconv3x3_g16: pad 1, stride 1 | 2,
// Cin == Cout == groups * gw, NHWC in / NHWC out, bf16 | fp16, fp32 accumulation on mfma16<DT>, y = act(acc * scale + bias).
//
// Shape of the work (generalised from gconv3x3_g16_tile_kernel):
//   * a workgroup (4 waves) stages the halo of a patch of TH fragments for a run of whole groups ONCE, with 16-byte loads
//     along the channels (NHWC), into LDS rows of RS bytes per halo pixel, RS an odd number of 16-byte slots;
//       run: as many whole groups as fit 256 B per pixel at stride 1, 128 B at stride 2; one group where gw alone is more;
//       fragment: 16 output pixels = (16 / TW) output rows x TW columns, TW = 16 | 8 | 4 by the map's width, so the narrow last
//       maps of a backbone (4x4 .. 8x8) fill their fragments;  TH = 8 | 4 | 2 fragments, the most that keeps the halo <= 64 KiB.
//   * GEMM view per group: D[gw rows, padded to RB = ceil(gw/16) row blocks][16 pixels] += W[rows][K] * X^T, k = tap * gw + ci,
//     K = 9 gw padded with zero weights to KS = ceil(9 gw / 32) k-steps.  gw % 8 == 0, so a lane's 8-element chunk lies inside
//     one tap: one ds_read_b128 per lane per k-step; the chunks of the K padding (tap >= 9) are zeroed in the register.
//   * weights come from the fragment-major image (include/ssdk.h, "grouped image"): the A operand of (group, row block, k-step)
//     is one coalesced 1 KiB wave load from L2, requested two k-steps ahead.  A wave's work item is (group, RBT row blocks, FT fragments): RBT x FT
//     accumulators stay in registers over the whole k loop, each k-step loads RBT A and FT B operands for RBT x FT MFMAs.
//     Padded rows (gw % 16 == 8: the upper half of the last row block) have zero weights and are not stored; the 8-byte
//     store of 4 consecutive channels per lane is wholly live or wholly padding because gw % 8 == 0.
//
// Width classes (template <RBT, FT>), chosen by RB, not per width:
//   class S  <1, 4>  gw = 8 (and the merged gw = 4)         the k loop is 3 steps: the group's weights are loaded once per
//                                                           4 fragments, i.e. stay in registers across them
//   class M  <2, 4>  gw = 24, 32                            both row blocks of the group in one item
//   class L  <4, 2>  gw = 40 .. 256 (40 48 56 64 112 120    weights streamed per k-step, each reused on 2 fragments; groups of
//                    128 168 of the registered backbones)   more than 4 row blocks take ceil(RB / 4) items, the last one partial
// Compiler figures for gfx950 (-Rpass-analysis=kernel-resource-usage; bf16 / fp16 alike, stride 1 | 2; no scratch anywhere;
// LDS is dynamic, 64 KiB at most except gw > 168 at stride 2):
//   S: 102 VGPRs, 4 waves per SIMD   M: 122 VGPRs, 3 waves per SIMD   L: 126 VGPRs, 3 waves per SIMD
// The halo (43 .. 61 KiB per workgroup) allows 2 .. 3 workgroups = 8 .. 12 waves per CU = 2 .. 3 per SIMD: registers and LDS
// meet there.  (Requesting the NEXT item's first stages before the epilogue costs 120 / 156 / 180 VGPRs, a wave per SIMD less,
// and measured slower on every shape but gw = 168; requesting scale / bias at the item's start costs 110 / 138 / 162 and
// measured slower at stride 2 and at gw = 56, 112: docs/HISTORY.md.)
#include "ssdk_conv_common.h"

namespace ssdk {

struct GanyParams {
  const u16* x;
  const u16* wf;  // fragment-major grouped image: [groups * RB][KS][4][16][8]
  const float* scale;
  const float* bias;
  u16* y;
  int N, H, W, C, Ho, Wo, act;
  int groups, gw;      // effective (after the packer's merge of 4-wide groups)
  int RB, KS;          // row blocks per group, k-steps
  int gw8_inv;         // ceil(65536 / (gw / 8)): (a * gw8_inv) >> 16 == a / (gw / 8) while a * (gw / 8) < 65536 (a <= 287 at gw = 256)
  int ngr;             // groups per workgroup (the channel run)
  int cblocks, tiles_x, tiles_y;
  int TH, tw_log2;     // fragments per patch; log2 of the fragment width
  int IH, IW, RS;      // halo rows, columns, LDS bytes per halo pixel
  int ppp_log2;        // staging: 16-byte pieces per pixel rounded up to a power of two
};

template <int DT, int S, int RBT, int FT>
__global__ __launch_bounds__(256) void gconv3x3_any_kernel(const GanyParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char gsm[];
  const u32 tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const u32 fr = lane & 15u, fg = lane >> 4;
  u32 b = blockIdx.x;
  const u32 cb = b % (u32)p.cblocks;
  b /= (u32)p.cblocks;
  const u32 tx = b % (u32)p.tiles_x;
  b /= (u32)p.tiles_x;
  const u32 ty = b % (u32)p.tiles_y;
  const u32 n = b / (u32)p.tiles_y;
  const int C = p.C, gw = p.gw, IW = p.IW, RS = p.RS;
  const int TW = 1 << p.tw_log2, RPF = 16 >> p.tw_log2;  // fragment: RPF output rows x TW columns
  const int g0 = (int)cb * p.ngr;
  const int ng = p.groups - g0 < p.ngr ? p.groups - g0 : p.ngr;  // groups of this block (the last run may be partial)
  const int oy0 = (int)ty * p.TH * RPF, ox0 = (int)tx * TW, iy0 = oy0 * S - 1, ix0 = ox0 * S - 1;

  // ---- halo: IH x IW pixels x (ng gw) channels in 16-byte pieces; a thread keeps its piece index and walks the pixels; LD
  // loads are issued before their LDS stores (one round for runs of <= 256 B on the 8 x 16 patch).  Pixels outside the image and the channels of a partial run store zeros.
  {
    const int ppp = (p.ngr * gw) >> 3;                 // pieces per pixel of a full run
    const int live = (ng * gw) >> 3;                   // ... that exist in this block
    const int pc = (int)(tid & ((1u << p.ppp_log2) - 1u));
    const int npx = p.IH * IW, pstep = 256 >> p.ppp_log2;
    const int drow = pstep / IW, dcol = pstep % IW;
    int px = (int)(tid >> p.ppp_log2);
    int row = px / IW, col = px % IW;
    const u16* xin = p.x + (size_t)n * p.H * p.W * C + (size_t)g0 * gw + pc * 8;
    if (pc < ppp) {
      while (px < npx) {
        constexpr int LD = 12;
        u32x4 v[LD];
        int r_ = row, c_ = col;
#pragma unroll
        for (int k = 0; k < LD; ++k) {
          const int iy = iy0 + r_, ix = ix0 + c_;
          v[k] = u32x4{0u, 0u, 0u, 0u};
          if (px + k * pstep < npx && pc < live && (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W)
            v[k] = *reinterpret_cast<const u32x4*>(xin + ((size_t)iy * p.W + ix) * C);
          r_ += drow;
          c_ += dcol;
          if (c_ >= IW) {
            c_ -= IW;
            ++r_;
          }
        }
#pragma unroll
        for (int k = 0; k < LD; ++k) {
          const int q = px + k * pstep;
          if (q < npx) *reinterpret_cast<u32x4*>(gsm + (size_t)q * RS + pc * 16) = v[k];
        }
        px += LD * pstep;
        row = r_;
        col = c_;
      }
    }
  }
  __syncthreads();

  const ActSel as = act_sel(p.act);
  const bool any_sig = act_is_sig(p.act), any_clamp = act_is_clamp(p.act);
  const int RB = p.RB, KS = p.KS;
  const int nrc = (RB + RBT - 1) / RBT, nfc = p.TH / FT;
  const int items = ng * nrc * nfc;
  // this lane's pixel inside a fragment and its halo offset for tap (0, 0)
  const int oyf = (int)(fr >> p.tw_log2), oxf = (int)(fr & (u32)(TW - 1));
  const u32 pix0 = (u32)((oyf * S * IW + oxf * S) * RS);
  const u32 fstr = (u32)(RPF * S * IW * RS);  // LDS bytes from one fragment to the next

  for (int it = (int)wave; it < items; it += 4) {  // wave-uniform; the fragment chunk runs fastest: neighbouring waves share A
    const int fc = it % nfc;
    const int t_ = it / nfc;
    const int rc = t_ % nrc, gl = t_ / nrc;
    const int f0 = fc * FT, rb0 = rc * RBT;
    if (oy0 + f0 * RPF >= p.Ho) continue;  // fragments below the map
    const u32 g = (u32)(g0 + gl);
    const u16* wbase = p.wf + ((size_t)(g * (u32)RB + (u32)rb0) * KS) * 512 + lane * 8u;
    const u32 xbase = pix0 + (u32)f0 * fstr + (u32)(gl * gw * 2);

    f32x4 acc[RBT][FT];
#pragma unroll
    for (int r = 0; r < RBT; ++r)
#pragma unroll
      for (int f = 0; f < FT; ++f) acc[r][f] = f32x4{0.f, 0.f, 0.f, 0.f};

    // One k-step's operands: RBT A fragments from the image (L2), FT B fragments from the halo (LDS).  The k loop runs on a ring
    // of three such stages, loads two k-steps ahead of the MFMAs that consume them: an L2 round trip is several k-steps of MFMA
    // work, and with 2 .. 3 waves per SIMD nothing else would cover it.
    struct Stage {
      u32x4 w[RBT], x[FT];
      bool kin;  // false: K padding (tap >= 9) -- zero weights, and the B operand is zeroed before use as well
    };
    auto load = [&](Stage& st, int s) {
      // k = 32 s + 8 fg .. + 7 -> tap = k / gw, channel ci = k % gw of the group (in units of 8 channels: a8 / (gw / 8))
      const int a8 = s * 4 + (int)fg;
      const int tap = (a8 * p.gw8_inv) >> 16;
      const int ci8 = a8 - tap * (gw >> 3);
      st.kin = tap < 9;
      const int tyk = st.kin ? (tap * 11) >> 5 : 0;  // tap / 3 for tap < 9
      const int txk = st.kin ? tap - 3 * tyk : 0;
      const u32 xo = xbase + (u32)((tyk * IW + txk) * RS + (st.kin ? ci8 : 0) * 16);  // (padding: an in-bounds address)
#pragma unroll
      for (int r = 0; r < RBT; ++r) {
        st.w[r] = u32x4{0u, 0u, 0u, 0u};
        if (rb0 + r < RB) st.w[r] = *reinterpret_cast<const u32x4*>(wbase + ((size_t)r * KS + s) * 512);
      }
#pragma unroll
      for (int f = 0; f < FT; ++f) st.x[f] = *reinterpret_cast<const u32x4*>(gsm + xo + (u32)f * fstr);
    };
    auto mma = [&](const Stage& st) {
#pragma unroll
      for (int f = 0; f < FT; ++f) {
        const u32x4 xv = st.kin ? st.x[f] : u32x4{0u, 0u, 0u, 0u};
#pragma unroll
        for (int r = 0; r < RBT; ++r) acc[r][f] = mfma16<DT>(st.w[r], xv, acc[r][f]);  // D[channel fg*4+e][pixel fr]
      }
    };
    Stage s0, s1, s2;
    load(s0, 0);
    if (KS > 1) load(s1, 1);
    for (int s = 0; s < KS; s += 3) {  // wave-uniform guards
      if (s + 2 < KS) load(s2, s + 2);
      mma(s0);
      if (s + 1 < KS) {
        if (s + 3 < KS) load(s0, s + 3);
        mma(s1);
      }
      if (s + 2 < KS) {
        if (s + 4 < KS) load(s1, s + 4);
        mma(s2);
      }
    }

#pragma unroll
    for (int r = 0; r < RBT; ++r) {
      const int cl = (rb0 + r) * 16 + (int)fg * 4;  // channel inside the group
      if (rb0 + r >= RB || cl >= gw) continue;      // row padding
      const u32 c = g * (u32)gw + (u32)cl;
      const f32x4 sc = *reinterpret_cast<const f32x4*>(p.scale + c);
      const f32x4 bi = *reinterpret_cast<const f32x4*>(p.bias + c);
#pragma unroll
      for (int f = 0; f < FT; ++f) {
        const int oy = oy0 + (f0 + f) * RPF + oyf, ox = ox0 + oxf;
        if (oy < p.Ho && ox < p.Wo) {
          float v[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = acc[r][f][e] * sc[e] + bi[e];
          if (any_sig) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const float sg = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.442695041f * v[e]));
              v[e] = as.mode == 1 ? sg : v[e] * sg;
            }
          }
          if (any_clamp) {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = __builtin_fminf(__builtin_fmaxf(v[e], as.lo), as.hi);
          }
          *reinterpret_cast<uint2*>(p.y + (((size_t)n * p.Ho + oy) * p.Wo + ox) * C + c) =
              make_uint2(pack2_16<DT>(v[0], v[1]), pack2_16<DT>(v[2], v[3]));
        }
      }
    }
  }
}

template <int DT, int S, int RBT, int FT>
static bool gany_launch(const GanyParams& p, long grid, size_t lds, hipStream_t stream) {
  // (halos above 64 KiB -- gw > 168 at stride 2 -- depend on this attribute: a refusal is an error, not a launch that fails later)
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(&gconv3x3_any_kernel<DT, S, RBT, FT>),
                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  hipLaunchKernelGGL((gconv3x3_any_kernel<DT, S, RBT, FT>), dim3((unsigned)grid), dim3(256), lds, stream, p);
  return true;
}

template <int DT, int S>
static bool gany_launch_class(const GanyParams& p, long grid, size_t lds, hipStream_t stream) {
  if (p.RB == 1) return gany_launch<DT, S, 1, 4>(p, grid, lds, stream);
  if (p.RB == 2) return gany_launch<DT, S, 2, 4>(p, grid, lds, stream);
  return gany_launch<DT, S, 4, 2>(p, grid, lds, stream);
}

int launch_gconv3x3_any(const ssdk_conv_desc* d, int Ho, int Wo, hipStream_t stream) {
  int groups = d->groups, gw = groups > 0 ? d->Cin / groups : 0;
  if (gw == 4 && (groups % 2) == 0) {  // the packer merged pairs of 4-wide groups into block-diagonal 8-wide ones
    gw = 8;
    groups /= 2;
  }
  if (d->k != 3 || d->Cin != d->Cout || groups < 1 || groups * gw != d->Cin || gw < 8 || gw > 256 || (gw % 8) || !d->scale ||
      d->residual || d->y2 || d->in_layout != LAYOUT_NHWC || d->out_layout != LAYOUT_NHWC ||
      (d->stride != 1 && d->stride != 2) || (d->dtype != SSDK_BF16 && d->dtype != SSDK_F16)) {
    set_error("conv: grouped convolution is built for k=3, stride 1|2, Cin == Cout, channels per group 4 (an even number of "
              "groups) or a multiple of 8 up to 256, bf16|f16, NHWC in/out, folded BN scale, no residual (Cin=%d Cout=%d "
              "groups=%d)", d->Cin, d->Cout, d->groups);
    return SSDK_E_BADARG;
  }
  if (!d->w_frag) {
    set_error("conv: grouped convolution with %d channels per group reads the fragment-major grouped image: w_frag is NULL",
              d->Cin / d->groups);
    return SSDK_E_BADARG;
  }
  if (((uintptr_t)d->x | (uintptr_t)d->w_frag | (uintptr_t)d->y | (uintptr_t)d->scale | (uintptr_t)d->bias) & 15) {
    set_error("conv: grouped convolution needs 16-byte aligned x, w_frag, y, scale, bias");
    return SSDK_E_BADARG;
  }
  const int S = d->stride;
  GanyParams p;
  p.x = (const u16*)d->x;
  p.wf = (const u16*)d->w_frag;
  p.scale = d->scale;
  p.bias = d->bias;
  p.y = (u16*)d->y;
  p.N = d->N;
  p.H = d->H;
  p.W = d->W;
  p.C = d->Cin;
  p.Ho = Ho;
  p.Wo = Wo;
  p.act = d->act;
  p.groups = groups;
  p.gw = gw;
  p.RB = (gw + 15) / 16;
  p.KS = (9 * gw + 31) / 32;
  p.gw8_inv = (65536 + gw / 8 - 1) / (gw / 8);
  // the channel run of a workgroup: whole groups in 256 B (stride 1) | 128 B (stride 2) per pixel, at least one
  const int run_bytes = S == 1 ? 256 : 128;
  p.ngr = run_bytes / (gw * 2) > 0 ? run_bytes / (gw * 2) : 1;
  if (p.ngr > groups) p.ngr = groups;
  p.cblocks = (groups + p.ngr - 1) / p.ngr;
  const int slots = p.ngr * gw / 8;              // 16-byte slots per halo pixel
  p.RS = (slots | 1) * 16;                       // odd: the 16 pixels of a ds_read_b128 lane group start in different banks
  p.ppp_log2 = 0;
  while ((1 << p.ppp_log2) < slots) ++p.ppp_log2;
  p.tw_log2 = Wo > 8 ? 4 : (Wo > 4 ? 3 : 2);
  const int TW = 1 << p.tw_log2, RPF = 16 / TW;
  const int FT = p.RB <= 2 ? 4 : 2;              // (gany_launch_class)
  p.TH = S == 1 ? 8 : 4;
  p.IW = (TW - 1) * S + 3;
  for (;;) {
    p.IH = (p.TH * RPF - 1) * S + 3;
    const bool fits = (size_t)p.IH * p.IW * p.RS <= 64u * 1024u;
    const bool needed = (p.TH / 2) * RPF >= Ho;  // half the patch still covers the map
    if (p.TH > FT && (!fits || needed)) p.TH /= 2;
    else break;
  }
  const size_t lds = (size_t)p.IH * p.IW * p.RS;
  if (lds > 128u * 1024u || p.ppp_log2 > 8) {
    set_error("conv: grouped convolution halo of %zu bytes does not fit (channels per group %d)", lds, gw);
    return SSDK_E_BADARG;
  }
  p.tiles_y = (Ho + p.TH * RPF - 1) / (p.TH * RPF);
  p.tiles_x = (Wo + TW - 1) / TW;
  const long grid = (long)d->N * p.tiles_y * p.tiles_x * p.cblocks;
  if (grid >= (1l << 31) || grid < 1) {
    set_error("conv: grouped convolution grid too large");
    return SSDK_E_BADARG;
  }
  bool ok;
  if (d->dtype == SSDK_BF16) ok = S == 1 ? gany_launch_class<SSDK_BF16, 1>(p, grid, lds, stream) : gany_launch_class<SSDK_BF16, 2>(p, grid, lds, stream);
  else ok = S == 1 ? gany_launch_class<SSDK_F16, 1>(p, grid, lds, stream) : gany_launch_class<SSDK_F16, 2>(p, grid, lds, stream);
  if (!ok) {
    set_error("conv: grouped convolution: %zu bytes of LDS per workgroup were refused (channels per group %d)", lds, gw);
    return SSDK_E_LAUNCH;
  }
  return check_launch("gconv3x3_any_kernel");
}

}  // namespace ssdk
