// ssdk_gconvtrain.hip -- the grouped 3x3 convolution of the TRAINING step on gfx950: forward, input gradient, weight gradient.
//
// Reference: the bottleneck 3x3 of RegNetX (ssds/modeling/nets/regnet.py: `b = Conv2d(w_b, w_b, 3, stride, groups = w_b / gw)`)
// and of ResNeXt (nets/resnet.py: Bottleneck.conv2 with groups = 32) inside the DDP step.  pad 1, stride 1 | 2,
// Cin == Cout == groups * gw, gw = 4 (an even number of groups: neighbouring pairs run as block-diagonal groups of 8) or a
// multiple of 8 up to 256 -- 16 included.  Tensors are bf16 | fp16, NCHW contiguous in and out (the layout of the 1x1 and
// BatchNorm kernels around the layer), fp32 accumulation on mfma16<DT>.  No BatchNorm fold, no activation.
//
//   prepare   gconv_train_prepare_kernel: the fp32 master weight [C, gw, 3, 3] -> two 16-bit grouped images (include/ssdk.h,
//             "grouped image"): the forward image (fused_conv.pack_grouped_frag of the cast weight) and the input-gradient image
//             (groupedconv.pack_grouped_frag_dgrad: per group transposed, taps flipped).  Replaces autocast's cast.
//   forward / input gradient   gconv_train_conv_kernel<DT, S, T, RBT, FT>.  The work decomposition of gconv3x3_any_kernel: a
//             workgroup stages the halo of TH fragments of 16 output pixels for a run of whole groups in LDS as [pixel][channel]
//             rows of RS bytes (RS an odd number of 16-byte slots), a wave item is (group, RBT channel blocks, FT fragments) and
//             streams its weights from the image with a three-stage ring.  What differs:
//               * the halo is read from NCHW: a lane takes one pixel of two neighbouring channels (2-byte loads, 16 lanes on 16
//                 consecutive pixels of a row) and stores them as ONE dword; lanes 4 q + j of a wave hold pixel q, channel pair j, so
//                 the 64 dwords of a store instruction fall into 64 different banks (pixel stride = 4 * odd dwords);
//               * the MFMA operand roles are swapped (A = pixels, B = weights): a lane's four accumulator values are four
//                 consecutive pixels of ONE channel, an 8-byte store along W;
//               * T (input gradient at stride 2) is a real transposed convolution: an input pixel (2a + py, 2b + px) sees the
//                 (1 + py)(1 + px) taps whose output pixel exists, 9 taps per 2 x 2 pixels, not 36.  An item computes both column
//                 parities of a row parity and interleaves them into one 16-byte store; its k loop walks the taps of its parity
//                 class and picks their 16-byte chunks out of the stride-1 input-gradient image (no second image).
//             Stride 1 input gradient = the forward kernel on the input-gradient image.
//   weight gradient   gconv_train_wgrad_kernel: dW[co][ci][tap] = sum over pixels dy[co][p] x[ci][p + tap] contracts over pixels,
//             contiguous along W in both operands.  A wave owns one 16 x 16 (co, ci) tile of a group, all nine taps (9 accumulators)
//             and a range of output rows; a k-step is 32 pixels, 8 per lane group: A = 16 bytes of a dy row, B = the x row window
//             of the three kx shifts from one 16-byte load + 2 elements (stride 1: v_alignbit; stride 2: two loads and the even /
//             odd pick with v_perm_b32, as stem_wgrad_kernel).  Narrow maps put 2 | 4 rows into a k-step.  The fp32 partial tiles
//             go to caller-owned workspace [split][tile][9][16][16]; gconv_train_wgrad_reduce_kernel adds them in split order: no
//             float atomics, bit-reproducible.
//
// Compiler figures for gfx950 (-Rpass-analysis=kernel-resource-usage; bf16 / fp16 alike; no scratch anywhere; the LDS of the conv
// kernel is dynamic, the halo, 64 KiB at most except gw > 168 at stride 2):
//   conv, forward / stride-1 input gradient   <RBT, FT> = <1,4>: 108 VGPRs, 4 waves per SIMD   <2,4>: 122, 3   <4,2>: 131, 3
//   conv, stride-2 input gradient (T)         <1,2>: 89, 4   <2,2>: 112, 4   <4,1>: 131, 3   (two parity accumulators per fragment)
//   wgrad   stride 1 / 2, FAST: 56 / 69 VGPRs, 5 / 4 waves per SIMD; element-wise rows: 78 / 106, 4 / 3
//   prepare 10, reduce 11 VGPRs
#include "ssdk_conv_common.h"

namespace ssdk {

// ---- effective grouping: 4-wide groups run in block-diagonal pairs --------------------------------------------------------------
struct GtShape {
  int gw0, groups_e, gwe, RB, KS;
};
static bool gt_shape(int C, int groups, GtShape* s) {
  if (C < 1 || groups < 1 || C % groups) return false;
  const int gw = C / groups;
  if (gw == 4 && (groups % 2) == 0) {
    s->gwe = 8;
    s->groups_e = groups / 2;
  } else if (gw >= 8 && gw <= 256 && (gw % 8) == 0) {
    s->gwe = gw;
    s->groups_e = groups;
  } else {
    return false;
  }
  s->gw0 = gw;
  s->RB = (s->gwe + 15) / 16;
  s->KS = (9 * s->gwe + 31) / 32;
  return true;
}

// ---- prepare ------------------------------------------------------------------------------------------------------------------------
struct GtPrepParams {
  const float* w;  // [C][gw0][3][3]
  u16* img[2];     // forward | input-gradient image, either may be NULL
  int gw0, gwe, RB, KS;
  u32 total;       // elements of one image
};

template <int DT>
__global__ __launch_bounds__(256) void gconv_train_prepare_kernel(const GtPrepParams p) {
  const u32 idx = blockIdx.x * 256u + threadIdx.x;
  const int which = (int)blockIdx.y;
  u16* out = p.img[which];
  if (idx >= p.total || !out) return;
  // image element [row block][k-step][k % 32 / 8][row % 16][k % 8]
  const int e8 = (int)(idx & 7u), r16 = (int)((idx >> 3) & 15u), c4 = (int)((idx >> 7) & 3u);
  const int blk = (int)(idx >> 9), ks = blk % p.KS, rbk = blk / p.KS;
  const int ge = rbk / p.RB, row = (rbk % p.RB) * 16 + r16;
  const int k = ks * 32 + c4 * 8 + e8, tap = k / p.gwe, cl = k - tap * p.gwe;
  float v = 0.f;
  const bool merged = p.gw0 == 4;
  if (row < p.gwe && tap < 9 && (!merged || (row >> 2) == (cl >> 2))) {
    int co, ci, t;
    if (which == 0) {  // rows: output channels, k = tap * gw + ci
      co = ge * p.gwe + row;
      ci = merged ? (cl & 3) : cl;
      t = tap;
    } else {  // rows: input channels, k = tap' * gw + co with tap' the flipped tap
      co = ge * p.gwe + cl;
      ci = merged ? (row & 3) : row;
      t = 8 - tap;
    }
    v = p.w[((size_t)co * p.gw0 + ci) * 9 + t];
  }
  out[idx] = (u16)f32_to_bits16<DT>(v);
}

// ---- forward / input gradient ---------------------------------------------------------------------------------------------------------
struct GtConvParams {
  const u16* x;   // [N, C, H, W]
  const u16* wf;  // grouped image [groups * RB][KS][4][16][8]
  u16* y;         // [N, C, Ho, Wo]
  int N, C, H, W, Ho, Wo;
  int Pa, Pb;      // the grid the patches tile: the output map, or (T) the half-resolution grid of one parity class
  int groups, gw;  // effective
  int RB, KS, gw8_inv, ngr, cblocks, tiles_x, tiles_y, TH, tw_log2, IH, IW, iw_inv, RS;
};

template <int DT, int S, bool T, int RBT, int FT>
__global__ __launch_bounds__(256) void gconv_train_conv_kernel(const GtConvParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char gsm[];
  constexpr int NPX = T ? 2 : 1;
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
  const int TW = 1 << p.tw_log2, RPF = 16 >> p.tw_log2;  // fragment: RPF rows x TW columns of the patch grid
  const int g0 = (int)cb * p.ngr;
  const int ng = p.groups - g0 < p.ngr ? p.groups - g0 : p.ngr;
  const int a0 = (int)ty * p.TH * RPF, b0 = (int)tx * TW;
  const int iy0 = T ? a0 : a0 * S - 1, ix0 = T ? b0 : b0 * S - 1;
  const size_t plane_in = (size_t)p.H * p.W;

  // ---- halo: IH x IW pixels x (ng gw) channels, NCHW -> [pixel][channel]; pixels outside the image are zeros
  {
    const int npx = p.IH * IW, nc8 = (ng * gw) >> 3;
    const int cpl = (int)(tid & 3u);
    const u16* xin = p.x + ((size_t)n * C + (size_t)g0 * gw) * plane_in;
    for (int c8 = 0; c8 < nc8; ++c8) {
      const int ch = c8 * 8 + cpl * 2;
      const u16* x0 = xin + (size_t)ch * plane_in;
      const u16* x1 = x0 + plane_in;
#pragma unroll 4
      for (int q = (int)(tid >> 2); q < npx; q += 64) {
        const int row = (q * p.iw_inv) >> 16, col = q - row * IW;
        const int iy = iy0 + row, ix = ix0 + col;
        const bool ok = (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W;
        const int off = ok ? iy * p.W + ix : 0;
        const u32 lo = x0[off], hi = x1[off];
        *reinterpret_cast<u32*>(gsm + (size_t)q * RS + ch * 2) = ok ? (lo | (hi << 16)) : 0u;
      }
    }
  }
  __syncthreads();

  const int RB = p.RB, KS = p.KS, gw8 = gw >> 3;
  const int nrc = (RB + RBT - 1) / RBT, nfc = p.TH / FT;
  const int items = ng * nrc * nfc * NPX;
  // A operand: this lane's pixel fr of a fragment and its halo offset for tap (0, 0)
  const int oyf = (int)(fr >> p.tw_log2), oxf = (int)(fr & (u32)(TW - 1));
  const int SH = T ? 1 : S;
  const u32 pix0 = (u32)((oyf * SH * IW + oxf * SH) * RS);
  const u32 fstr = (u32)(RPF * SH * IW * RS);
  // D: this lane's four pixels 4 fg .. 4 fg + 3 of a fragment (one row of it, consecutive columns)
  const int oyd = (int)((fg * 4u) >> p.tw_log2), oxd = (int)((fg * 4u) & (u32)(TW - 1));

  for (int it = (int)wave; it < items; it += 4) {  // wave-uniform
    int t_ = it;
    const int fc = t_ % nfc;
    t_ /= nfc;
    const int rc = t_ % nrc;
    t_ /= nrc;
    const int py = T ? (t_ & 1) : 0;
    const int gl = T ? (t_ >> 1) : t_;
    const int f0 = fc * FT, rb0 = rc * RBT;
    if (a0 + f0 * RPF >= p.Pa) continue;  // fragments below the grid
    const u32 g = (u32)(g0 + gl);
    const u16* wbase = p.wf + ((size_t)(g * (u32)RB + (u32)rb0) * KS) * 512 + fr * 8u;
    const u32 xbase = pix0 + (u32)f0 * fstr + (u32)(gl * gw * 2);

    f32x4 acc[NPX][RBT][FT];
#pragma unroll
    for (int h = 0; h < NPX; ++h)
#pragma unroll
      for (int r = 0; r < RBT; ++r)
#pragma unroll
        for (int f = 0; f < FT; ++f) acc[h][r][f] = f32x4{0.f, 0.f, 0.f, 0.f};

#pragma unroll
    for (int px = 0; px < NPX; ++px) {
      const int ntaps = T ? (1 + py) * (1 + px) : 9;
      const int ksteps = T ? (ntaps * gw + 31) >> 5 : KS;
      struct Stage {
        u32x4 w[RBT], x[FT];
        bool kin;  // false: K padding
      };
      auto load = [&](Stage& st, int s) {
        // k = 32 s + 8 fg .. + 7 of this class -> tap = k / gw, channel chunk ci8 = (k % gw) / 8
        const int a8 = s * 4 + (int)fg;
        int tap = (a8 * p.gw8_inv) >> 16;
        int ci8 = a8 - tap * gw8;
        st.kin = tap < ntaps;
        if (!st.kin) tap = 0, ci8 = 0;  // (an in-bounds address; both operands are zeroed)
        int tyk, txk, itap;
        if constexpr (!T) {
          tyk = (tap * 11) >> 5;  // tap / 3 for tap < 9
          txk = tap - 3 * tyk;
          itap = tap;
        } else {
          // the class's taps in (row, column) order of the output pixels (a + tyk, b + txk); in the input-gradient image the
          // tap of output row a + tyk is ky' = 2 tyk (odd input rows: ky' = 0 | 2) or 1 (even input rows), columns alike
          tyk = px ? (tap >> 1) : tap;
          txk = px ? (tap & 1) : 0;
          itap = 3 * (py ? 2 * tyk : 1) + (px ? 2 * txk : 1);
        }
        const u32 xo = xbase + (u32)((tyk * IW + txk) * RS + ci8 * 16);
        const int a8g = itap * gw8 + ci8;  // the chunk's place in the image row: k-step a8g / 4, lane group a8g % 4
        const u32 wo = (u32)((a8g >> 2) * 512 + (a8g & 3) * 128);
#pragma unroll
        for (int r = 0; r < RBT; ++r) {
          st.w[r] = u32x4{0u, 0u, 0u, 0u};
          if (rb0 + r < RB && st.kin) st.w[r] = *reinterpret_cast<const u32x4*>(wbase + (size_t)r * KS * 512 + wo);
        }
#pragma unroll
        for (int f = 0; f < FT; ++f) st.x[f] = *reinterpret_cast<const u32x4*>(gsm + xo + (u32)f * fstr);
      };
      auto mma = [&](const Stage& st) {
#pragma unroll
        for (int f = 0; f < FT; ++f) {
          const u32x4 xv = st.kin ? st.x[f] : u32x4{0u, 0u, 0u, 0u};
#pragma unroll
          for (int r = 0; r < RBT; ++r) acc[px][r][f] = mfma16<DT>(xv, st.w[r], acc[px][r][f]);  // D[pixel fg*4+e][channel fr]
        }
      };
      Stage s0, s1, s2;
      load(s0, 0);
      if (ksteps > 1) load(s1, 1);
      for (int s = 0; s < ksteps; s += 3) {  // wave-uniform guards
        if (s + 2 < ksteps) load(s2, s + 2);
        mma(s0);
        if (s + 1 < ksteps) {
          if (s + 3 < ksteps) load(s0, s + 3);
          mma(s1);
        }
        if (s + 2 < ksteps) {
          if (s + 4 < ksteps) load(s1, s + 4);
          mma(s2);
        }
      }
    }

    const size_t plane_out = (size_t)p.Ho * p.Wo;
#pragma unroll
    for (int r = 0; r < RBT; ++r) {
      const int cl = (rb0 + r) * 16 + (int)fr;  // channel inside the group
      if (rb0 + r >= RB || cl >= gw) continue;  // row padding
      u16* yc = p.y + ((size_t)n * C + (size_t)g * gw + cl) * plane_out;
#pragma unroll
      for (int f = 0; f < FT; ++f) {
        const int a = a0 + (f0 + f) * RPF + oyd, bq = b0 + oxd;
        if constexpr (!T) {
          if (a < p.Ho && bq < p.Wo) {
            u16* dst = yc + (size_t)a * p.Wo + bq;
            const f32x4 v = acc[0][r][f];
            if ((p.Wo & 3) == 0 && (((uintptr_t)p.y) & 7u) == 0) {  // uniform: the four pixels exist and are 8-byte aligned
              *reinterpret_cast<uint2*>(dst) = make_uint2(pack2_16<DT>(v[0], v[1]), pack2_16<DT>(v[2], v[3]));
            } else {
#pragma unroll
              for (int e = 0; e < 4; ++e)
                if (bq + e < p.Wo) dst[e] = (u16)f32_to_bits16<DT>(v[e]);
            }
          }
        } else {
          const int iy = 2 * a + py, ix = 2 * bq;
          if (iy < p.Ho && ix < p.Wo) {
            u16* dst = yc + (size_t)iy * p.Wo + ix;
            const f32x4 v0 = acc[0][r][f], v1 = acc[NPX - 1][r][f];
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

template <int DT, int S, bool T, int RBT, int FT>
static bool gt_conv_launch(const GtConvParams& p, long grid, size_t lds, hipStream_t stream) {
  // (halos above 64 KiB depend on this attribute: a refusal is an error, not a launch that fails later)
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(&gconv_train_conv_kernel<DT, S, T, RBT, FT>),
                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  hipLaunchKernelGGL((gconv_train_conv_kernel<DT, S, T, RBT, FT>), dim3((unsigned)grid), dim3(256), lds, stream, p);
  return true;
}

template <int DT, int S, bool T>
static bool gt_conv_launch_class(const GtConvParams& p, long grid, size_t lds, hipStream_t stream) {
  // width classes by row blocks, as gconv3x3_any_kernel; T carries two parity accumulators per fragment: half the fragments
  if (p.RB == 1) return gt_conv_launch<DT, S, T, 1, T ? 2 : 4>(p, grid, lds, stream);
  if (p.RB == 2) return gt_conv_launch<DT, S, T, 2, T ? 2 : 4>(p, grid, lds, stream);
  return gt_conv_launch<DT, S, T, 4, T ? 1 : 2>(p, grid, lds, stream);
}

// x [N, C, H, W] -> y [N, C, Ho, Wo]; transposed: x is the output gradient [N, C, H, W] of a stride-2 layer, y its input gradient
static int gt_conv(const char* what, const void* x, const void* wf, void* y, int N, int C, int H, int W, int Ho, int Wo, const GtShape& sh,
                   int stride, bool transposed, int dtype, hipStream_t stream) {
  GtConvParams p;
  memset(&p, 0, sizeof(p));
  p.x = (const u16*)x;
  p.wf = (const u16*)wf;
  p.y = (u16*)y;
  p.N = N;
  p.C = C;
  p.H = H;
  p.W = W;
  p.Ho = Ho;
  p.Wo = Wo;
  p.Pa = transposed ? (Ho + 1) / 2 : Ho;
  p.Pb = transposed ? (Wo + 1) / 2 : Wo;
  p.groups = sh.groups_e;
  p.gw = sh.gwe;
  p.RB = sh.RB;
  p.KS = sh.KS;
  const int gw = sh.gwe, S = transposed ? 1 : stride;
  p.gw8_inv = (65536 + gw / 8 - 1) / (gw / 8);
  // the channel run of a workgroup: whole groups in 256 B (stride 1) | 128 B (stride 2) per halo pixel, at least one
  const int run_bytes = S == 1 ? 256 : 128;
  p.ngr = run_bytes / (gw * 2) > 0 ? run_bytes / (gw * 2) : 1;
  if (p.ngr > p.groups) p.ngr = p.groups;
  p.cblocks = (p.groups + p.ngr - 1) / p.ngr;
  const int slots = p.ngr * gw / 8;
  p.RS = (slots | 1) * 16;  // odd: conflict-free ds_read_b128 over 16 pixels and conflict-free dword stores of the staging
  p.tw_log2 = p.Pb > 8 ? 4 : (p.Pb > 4 ? 3 : 2);
  const int TW = 1 << p.tw_log2, RPF = 16 / TW;
  const int FT = transposed ? (p.RB <= 2 ? 2 : 1) : (p.RB <= 2 ? 4 : 2);  // (gt_conv_launch_class)
  p.TH = S == 1 ? 8 : 4;
  p.IW = transposed ? TW + 1 : (TW - 1) * S + 3;
  for (;;) {
    p.IH = transposed ? p.TH * RPF + 1 : (p.TH * RPF - 1) * S + 3;
    const bool fits = (size_t)p.IH * p.IW * p.RS <= 64u * 1024u;
    const bool needed = (p.TH / 2) * RPF >= p.Pa;  // half the patch still covers the grid
    if (p.TH > FT && (!fits || needed)) p.TH /= 2;
    else break;
  }
  p.iw_inv = (65536 + p.IW - 1) / p.IW;
  const size_t lds = (size_t)p.IH * p.IW * p.RS;
  if (lds > 128u * 1024u || p.IH * p.IW >= 1900) {
    set_error("%s: halo of %zu bytes does not fit (channels per group %d)", what, lds, gw);
    return SSDK_E_BADARG;
  }
  p.tiles_y = (p.Pa + p.TH * RPF - 1) / (p.TH * RPF);
  p.tiles_x = (p.Pb + TW - 1) / TW;
  const long grid = (long)N * p.tiles_y * p.tiles_x * p.cblocks;
  if (grid >= (1l << 31) || grid < 1) {
    set_error("%s: grid too large", what);
    return SSDK_E_BADARG;
  }
  bool ok;
  if (dtype == SSDK_BF16) {
    ok = transposed ? gt_conv_launch_class<SSDK_BF16, 1, true>(p, grid, lds, stream)
                    : (S == 1 ? gt_conv_launch_class<SSDK_BF16, 1, false>(p, grid, lds, stream)
                              : gt_conv_launch_class<SSDK_BF16, 2, false>(p, grid, lds, stream));
  } else {
    ok = transposed ? gt_conv_launch_class<SSDK_F16, 1, true>(p, grid, lds, stream)
                    : (S == 1 ? gt_conv_launch_class<SSDK_F16, 1, false>(p, grid, lds, stream)
                              : gt_conv_launch_class<SSDK_F16, 2, false>(p, grid, lds, stream));
  }
  if (!ok) {
    set_error("%s: %zu bytes of LDS per workgroup were refused (channels per group %d)", what, lds, gw);
    return SSDK_E_LAUNCH;
  }
  return SSDK_OK;
}

// ---- weight gradient ------------------------------------------------------------------------------------------------------------------
struct GtWgradParams {
  const u16* x;   // [N, C, H, W]
  const u16* dy;  // [N, C, Ho, Wo]
  float* part;    // [splits][ntiles][9][16][16]
  float* dw;      // [C][gw0][3][3]
  int N, C, H, W, Ho, Wo;
  int gw0, gwe, RB, ntiles, splits, rows_per_split, ck_log2;
};

// The window of one x row behind eight output pixels ox .. ox + 7 as dwords D: element E[i] = column S * ox - 1 + i (zero outside
// the row); D[0] = (-, E0), D[1 + i] = (E[1 + 2 i], E[2 + 2 i]); stride 1: i < 4 and D[5] = (E9, -); stride 2: i < 8.
// FAST (W a multiple of 8 S, 16-byte aligned tensor): the eight pixels lie inside the row, the middle is S aligned 16-byte loads.
template <int S, bool FAST>
__device__ __forceinline__ void gt_window_load(const u16* row, int ox, int W, u32 (&d)[10]) {
  const int cb = S * ox, last = W - 1;
  if constexpr (FAST) {
    const u32 left = row[cb > 0 ? cb - 1 : 0];
    d[0] = cb > 0 ? left << 16 : 0u;
    const u32x4 q0 = *reinterpret_cast<const u32x4*>(row + cb);
    d[1] = q0[0];
    d[2] = q0[1];
    d[3] = q0[2];
    d[4] = q0[3];
    if constexpr (S == 1) {
      const u32 right = row[cb + 8 < last ? cb + 8 : last];
      d[5] = cb + 8 < W ? right : 0u;
    } else {
      const u32x4 q1 = *reinterpret_cast<const u32x4*>(row + cb + 8);
      d[5] = q1[0];
      d[6] = q1[1];
      d[7] = q1[2];
      d[8] = q1[3];
    }
  } else {
    constexpr int NE = S == 1 ? 10 : 17;
    u32 e[NE + 1];
#pragma unroll
    for (int i = 0; i < NE; ++i) {
      const int c = cb - 1 + i;
      const u32 t = row[c < 0 ? 0 : (c < last ? c : last)];
      e[i] = (c >= 0 && c < W) ? t : 0u;
    }
    e[NE] = 0u;
    d[0] = e[0] << 16;
#pragma unroll
    for (int i = 0; i < (S == 1 ? 5 : 8); ++i) d[1 + i] = e[1 + 2 * i] | (e[2 + 2 * i] << 16);
  }
}
template <int S>
__device__ __forceinline__ u32x4 gt_window_pick(const u32 (&d)[10], bool ok, int kx) {  // kx compile-time after unrolling
  u32x4 out;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    u32 t;
    if constexpr (S == 1) {
      t = kx == 1 ? d[1 + j] : (kx == 0 ? __builtin_amdgcn_alignbit(d[j + 1], d[j], 16) : __builtin_amdgcn_alignbit(d[j + 2], d[j + 1], 16));
    } else {
      // kx = 0: high halves of (d[2j], d[2j + 1]); kx = 1: low halves of (d[2j + 1], d[2j + 2]); kx = 2: their high halves
      const u32 lo = kx == 0 ? d[2 * j] : d[1 + 2 * j], hi = kx == 0 ? d[1 + 2 * j] : d[2 + 2 * j];
      t = kx == 1 ? __builtin_amdgcn_perm(hi, lo, 0x05040100u) : __builtin_amdgcn_perm(hi, lo, 0x07060302u);
    }
    out[j] = ok ? t : 0u;
  }
  return out;
}
template <bool FAST>
__device__ __forceinline__ u32x4 gt_dy_load(const u16* row, int ox, int Wo, bool ok) {  // eight pixels ox .. ox + 7 of one channel row
  u32x4 out;
  if constexpr (FAST) {
    out = *reinterpret_cast<const u32x4*>(row + ox);
  } else {
    const int last = Wo - 1;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int c = ox + 2 * i;
      const u32 e0 = row[c < last ? c : last], e1 = row[c + 1 < last ? c + 1 : last];
      out[i] = (c < Wo ? e0 : 0u) | ((c + 1 < Wo ? e1 : 0u) << 16);
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) out[i] = ok ? out[i] : 0u;
  return out;
}

template <int DT, int S, bool FAST>
__global__ __launch_bounds__(256) void gconv_train_wgrad_kernel(const GtWgradParams p) {
  const u32 tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const int fr = (int)(lane & 15u), fg = (int)(lane >> 4);
  const int tile = (int)(blockIdx.x * 4u + wave);
  if (tile >= p.ntiles) return;  // (wave-uniform; the kernel has no barrier)
  const int split = (int)blockIdx.y;
  const int RB = p.RB, gwe = p.gwe;
  const int ge = tile / (RB * RB), ta = (tile / RB) % RB, tb = tile % RB;
  // this lane's output-gradient channel (A rows) and input channel (B columns); padding lanes read the group's last channel, their
  // tile rows / columns are dropped by the reduce
  const int co = ge * gwe + (ta * 16 + fr < gwe ? ta * 16 + fr : gwe - 1);
  const int ci = ge * gwe + (tb * 16 + fr < gwe ? tb * 16 + fr : gwe - 1);
  const int CK = 1 << p.ck_log2, RK = 4 >> p.ck_log2;  // a k-step: RK output rows x CK groups of 8 pixels
  const int total_rows = p.N * p.Ho;
  const int R0 = split * p.rows_per_split, R1 = R0 + p.rows_per_split < total_rows ? R0 + p.rows_per_split : total_rows;
  const size_t plane_x = (size_t)p.H * p.W, plane_y = (size_t)p.Ho * p.Wo;
  f32x4 acc[9];
#pragma unroll
  for (int t = 0; t < 9; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int oxl = 8 * (fg & (CK - 1));
  for (int R = R0; R < R1; R += RK) {  // wave-uniform
    const int myR = R + (fg >> p.ck_log2);
    const bool rowok = myR < R1;
    const int Rc = rowok ? myR : R0;
    const int n = Rc / p.Ho, oy = Rc - n * p.Ho;
    const u16* grow = p.dy + ((size_t)n * p.C + co) * plane_y + (size_t)oy * p.Wo;
    const u16* xrow[3];
    bool xok[3];
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
      const int iy = oy * S + ky - 1;
      xok[ky] = rowok && (unsigned)iy < (unsigned)p.H;
      xrow[ky] = p.x + ((size_t)n * p.C + ci) * plane_x + (size_t)(xok[ky] ? iy : 0) * p.W;
    }
    for (int ox0 = 0; ox0 < p.Wo; ox0 += 8 * CK) {  // wave-uniform
      const int ox = ox0 + oxl;
      const bool in = ox < p.Wo;
      const int oxc = in ? ox : 0;  // (FAST: a group of eight pixels is wholly inside the row or wholly outside)
      const u32x4 A = gt_dy_load<FAST>(grow, oxc, p.Wo, rowok && in);
      u32 D[3][10];
#pragma unroll
      for (int ky = 0; ky < 3; ++ky) gt_window_load<S, FAST>(xrow[ky], oxc, p.W, D[ky]);
#pragma unroll
      for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) acc[ky * 3 + kx] = mfma16<DT>(A, gt_window_pick<S>(D[ky], xok[ky] && in, kx), acc[ky * 3 + kx]);
    }
  }
  // D[m = 4 fg + j][n = fr] of tap t = dW[co = 16 ta + m][ci = 16 tb + n][t]
  float* out = p.part + ((size_t)split * p.ntiles + tile) * 2304;
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int j = 0; j < 4; ++j) out[t * 256 + (fg * 4 + j) * 16 + fr] = acc[t][j];
}

// dw = the partial tiles added in split order; one thread per tile element
__global__ __launch_bounds__(256) void gconv_train_wgrad_reduce_kernel(const GtWgradParams p) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t per = (size_t)p.ntiles * 2304;
  if (i >= per) return;
  float s = 0.f;
  for (int q = 0; q < p.splits; ++q) s += p.part[(size_t)q * per + i];
  const int tile = (int)(i / 2304), r = (int)(i % 2304);
  const int t = r >> 8, m = (r >> 4) & 15, nn = r & 15;
  const int RB = p.RB, ge = tile / (RB * RB), ta = (tile / RB) % RB, tb = tile % RB;
  const int col = ta * 16 + m, cil = tb * 16 + nn;
  if (col >= p.gwe || cil >= p.gwe) return;
  if (p.gw0 == 4 && (col >> 2) != (cil >> 2)) return;  // the off-diagonal blocks of a merged pair
  const int co = ge * p.gwe + col, ci = p.gw0 == 4 ? (cil & 3) : cil;
  p.dw[((size_t)co * p.gw0 + ci) * 9 + t] = s;
}

static void gt_wgrad_plan(int N, int Ho, int Wo, const GtShape& sh, GtWgradParams* p) {
  p->ntiles = sh.groups_e * sh.RB * sh.RB;
  p->ck_log2 = Wo > 16 ? 2 : (Wo > 8 ? 1 : 0);
  const int RK = 4 >> p->ck_log2;
  const long rows = (long)N * Ho;
  long target = 2048 / p->ntiles;  // ~2048 waves
  if (target > 256) target = 256;
  if (target < 1) target = 1;
  long rps = (rows + target - 1) / target;
  rps = (rps + RK - 1) / RK * RK;
  p->rows_per_split = (int)rps;
  p->splits = (int)((rows + rps - 1) / rps);
}

static int gt_check(const char* what, int N, int C, int H, int W, int groups, int stride, int dtype, GtShape* sh) {
  if (N < 1 || H < 1 || W < 1 || (stride != 1 && stride != 2) || (dtype != SSDK_BF16 && dtype != SSDK_F16) || !gt_shape(C, groups, sh)) {
    set_error("%s: built for 3x3, pad 1, stride 1|2, C == groups * gw with gw = 4 (an even number of groups) or a multiple of 8 up to "
              "256, bf16|f16 NCHW tensors (N=%d C=%d H=%d W=%d groups=%d stride=%d dtype=%d)", what, N, C, H, W, groups, stride, dtype);
    return SSDK_E_BADARG;
  }
  if ((size_t)H * W >= (1ull << 30) || (size_t)N * C * H * W >= (1ull << 40) || (size_t)N * H >= (1ull << 30)) {
    set_error("%s: tensor too large", what);
    return SSDK_E_BADARG;
  }
  return SSDK_OK;
}

}  // namespace ssdk

using namespace ssdk;

extern "C" int ssdk_gconv3x3_train_prepare(const float* w32, void* w_fwd, void* w_dgrad, int C, int groups, int dtype, void* stream) {
  GtShape sh;
  if (int rc = gt_check("gconv3x3_train_prepare", 1, C, 1, 1, groups, 1, dtype, &sh)) return rc;
  if (!w32 || (!w_fwd && !w_dgrad) || (((uintptr_t)w_fwd | (uintptr_t)w_dgrad) & 15u)) {
    set_error("gconv3x3_train_prepare: null weights, no image asked for, or an image that is not 16-byte aligned");
    return SSDK_E_BADARG;
  }
  GtPrepParams p;
  p.w = w32;
  p.img[0] = (u16*)w_fwd;
  p.img[1] = (u16*)w_dgrad;
  p.gw0 = sh.gw0;
  p.gwe = sh.gwe;
  p.RB = sh.RB;
  p.KS = sh.KS;
  const size_t total = (size_t)sh.groups_e * sh.RB * sh.KS * 512;
  if (total >= (1ull << 31)) {
    set_error("gconv3x3_train_prepare: image too large");
    return SSDK_E_BADARG;
  }
  p.total = (u32)total;
  const dim3 grid((unsigned)((total + 255) / 256), 2);
  if (dtype == SSDK_BF16) hipLaunchKernelGGL((gconv_train_prepare_kernel<SSDK_BF16>), grid, dim3(256), 0, (hipStream_t)stream, p);
  else hipLaunchKernelGGL((gconv_train_prepare_kernel<SSDK_F16>), grid, dim3(256), 0, (hipStream_t)stream, p);
  return check_launch("gconv_train_prepare_kernel");
}

extern "C" int ssdk_gconv3x3_train_forward(const void* x, const void* w_fwd, void* y, int N, int C, int H, int W, int groups, int stride,
                                           int dtype, void* stream) {
  GtShape sh;
  if (int rc = gt_check("gconv3x3_train_forward", N, C, H, W, groups, stride, dtype, &sh)) return rc;
  if (!x || !w_fwd || !y || ((uintptr_t)w_fwd & 15u) || (((uintptr_t)x | (uintptr_t)y) & 1u)) {
    set_error("gconv3x3_train_forward: null pointer, or an image that is not 16-byte aligned");
    return SSDK_E_BADARG;
  }
  const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
  if (int rc = gt_conv("gconv3x3_train_forward", x, w_fwd, y, N, C, H, W, Ho, Wo, sh, stride, false, dtype, (hipStream_t)stream)) return rc;
  return check_launch("gconv_train_fwd_kernel");
}

extern "C" int ssdk_gconv3x3_train_dgrad(const void* dy, const void* w_dgrad, void* dx, int N, int C, int H, int W, int groups, int stride,
                                         int dtype, void* stream) {
  GtShape sh;
  if (int rc = gt_check("gconv3x3_train_dgrad", N, C, H, W, groups, stride, dtype, &sh)) return rc;
  if (!dy || !w_dgrad || !dx || ((uintptr_t)w_dgrad & 15u) || (((uintptr_t)dy | (uintptr_t)dx) & 1u)) {
    set_error("gconv3x3_train_dgrad: null pointer, or an image that is not 16-byte aligned");
    return SSDK_E_BADARG;
  }
  const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
  int rc;
  if (stride == 1) rc = gt_conv("gconv3x3_train_dgrad", dy, w_dgrad, dx, N, C, H, W, H, W, sh, 1, false, dtype, (hipStream_t)stream);
  else rc = gt_conv("gconv3x3_train_dgrad", dy, w_dgrad, dx, N, C, Ho, Wo, H, W, sh, 2, true, dtype, (hipStream_t)stream);
  if (rc) return rc;
  return check_launch(stride == 1 ? "gconv_train_dgrad_kernel" : "gconv_train_dgrad_s2_kernel");
}

extern "C" size_t ssdk_gconv3x3_train_wgrad_workspace_bytes(int N, int C, int H, int W, int groups, int stride) {
  GtShape sh;
  if (N < 1 || H < 1 || W < 1 || (stride != 1 && stride != 2) || !gt_shape(C, groups, &sh)) return 0;
  GtWgradParams p;
  gt_wgrad_plan(N, (H - 1) / stride + 1, (W - 1) / stride + 1, sh, &p);
  return (size_t)p.splits * p.ntiles * 2304 * sizeof(float);
}

extern "C" int ssdk_gconv3x3_train_wgrad(const void* x, const void* dy, float* dw, void* workspace, size_t workspace_bytes, int N, int C,
                                         int H, int W, int groups, int stride, int dtype, void* stream) {
  GtShape sh;
  if (int rc = gt_check("gconv3x3_train_wgrad", N, C, H, W, groups, stride, dtype, &sh)) return rc;
  if (!x || !dy || !dw || !workspace || ((uintptr_t)workspace & 15u) || (((uintptr_t)x | (uintptr_t)dy) & 1u) || ((uintptr_t)dw & 3u) ||
      workspace_bytes < ssdk_gconv3x3_train_wgrad_workspace_bytes(N, C, H, W, groups, stride)) {
    set_error("gconv3x3_train_wgrad: null pointer, or workspace too small / misaligned (%zu bytes given, %zu needed)", workspace_bytes,
              ssdk_gconv3x3_train_wgrad_workspace_bytes(N, C, H, W, groups, stride));
    return SSDK_E_BADARG;
  }
  GtWgradParams p;
  memset(&p, 0, sizeof(p));
  p.x = (const u16*)x;
  p.dy = (const u16*)dy;
  p.dw = dw;
  p.part = (float*)workspace;
  p.N = N;
  p.C = C;
  p.H = H;
  p.W = W;
  p.Ho = (H - 1) / stride + 1;
  p.Wo = (W - 1) / stride + 1;
  p.gw0 = sh.gw0;
  p.gwe = sh.gwe;
  p.RB = sh.RB;
  gt_wgrad_plan(N, p.Ho, p.Wo, sh, &p);
  if (p.splits > 65535) {
    set_error("gconv3x3_train_wgrad: too many pixel ranges (%d)", p.splits);
    return SSDK_E_BADARG;
  }
  hipStream_t st = (hipStream_t)stream;
  const bool fast = (W % (8 * stride)) == 0 && ((((uintptr_t)x) | ((uintptr_t)dy)) & 15u) == 0;
  const dim3 grid((unsigned)((p.ntiles + 3) / 4), (unsigned)p.splits);
#define SSDK_GT_W(DT)                                                                                              \
  do {                                                                                                             \
    if (stride == 1) {                                                                                             \
      if (fast) hipLaunchKernelGGL((gconv_train_wgrad_kernel<DT, 1, true>), grid, dim3(256), 0, st, p);            \
      else hipLaunchKernelGGL((gconv_train_wgrad_kernel<DT, 1, false>), grid, dim3(256), 0, st, p);                \
    } else {                                                                                                       \
      if (fast) hipLaunchKernelGGL((gconv_train_wgrad_kernel<DT, 2, true>), grid, dim3(256), 0, st, p);            \
      else hipLaunchKernelGGL((gconv_train_wgrad_kernel<DT, 2, false>), grid, dim3(256), 0, st, p);                \
    }                                                                                                              \
  } while (0)
  if (dtype == SSDK_BF16) SSDK_GT_W(SSDK_BF16);
  else SSDK_GT_W(SSDK_F16);
#undef SSDK_GT_W
  const size_t per = (size_t)p.ntiles * 2304;
  hipLaunchKernelGGL(gconv_train_wgrad_reduce_kernel, dim3((unsigned)((per + 255) / 256)), dim3(256), 0, st, p);
  return check_launch("gconv_train_wgrad_kernel");
}
