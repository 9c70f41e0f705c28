// ssdk_convt.hip -- transposed 3x3 convolution, stride 2, padding 1 (+ bias, + skip) on gfx950: the decoder step of the Shelf
// neck (ssds/shelf.py ShelfPyramid: ConvTranspose2d(C_{i-1}, C_i, 3, stride=2, padding=1)(x) + xx[i]).  NHWC, bf16 | f16, one
// launch behind ssdk_convt3x3s2 (include/ssdk_convt.h).
//
//   convt3x3s2_kernel  y [N][2H-1][2W-1][Cout] = act(convT(x [N][H][W][Cin]) + bias) (+ skip), by PARITY CLASS of the output
//                      pixel: with oy = 2 iy - 1 + ky an even row takes ky = 1 from iy = oy / 2, an odd row ky = 2 from
//                      iy = (oy - 1) / 2 and ky = 0 from iy + 1; columns alike.  Class (py, px) is an ordinary GEMM with
//                      K = (1 + py)(1 + px) Cin over the (H - py) x (W - px) input pixels that have the neighbours it needs, so
//                      there is no zero-inserted tensor (4 x the MACs) and no border masking inside the k-loop.
//                      A workgroup owns PT fragments of 16 input pixels (flat over N H W: a fragment may straddle rows and
//                      images) and up to 4 blocks of 16 output channels, and walks the classes of its pixels one behind the
//                      other: the 2 x 2 output quad of every pixel it owns.  The pixel and its three neighbours are read nine
//                      times in all, back to back by the same workgroup -- from HBM once, the rest from L1 / L2.
//                      Its four waves SPLIT K: wave w takes the k-steps ks = w, w + 4, ... (a 512-channel four-tap class is
//                      64 dependent load -> MFMA steps, and with operands straight from global memory the chain's latency,
//                      not the matrix core, is what a launch waits for), the partial accumulators meet in LDS, and wave b adds
//                      the four partials of channel block b in wave order and runs its epilogue -- a fixed order, no atomics:
//                      two runs give the same bits.  v_mfma_f32_16x16x32: the weights are the A operand (rows = output
//                      channels), 1 KiB contiguous per wave instruction from the class's fragment-major image
//                      (ssdk_weight_frag_bytes; built by fused_conv.ConvTPack), the pixels the B operand.  k = tap * Cin + ci:
//                      a lane's octet lies inside one tap (Cin % 8 == 0) but a k-step may straddle taps, so every lane walks
//                      its own (tap, ci).  K tails and the Cout tail are the zero rows / columns of the image; pixels without
//                      the class's neighbours (last row / column) and the pixel tail are zero fragments and masked stores.
//                      Epilogue: + bias, activation, + skip, ONE rounding.
//                      Launch (a function of the shape alone; every choice computes the same bits): PT = 2 where that still
//                      gives 256 workgroups (the weights are re-read once per 32 pixels), else PT = 1, and while there are
//                      fewer than 256 workgroups the classes go to blockIdx.z and the channel blocks per workgroup from 4 to
//                      2 to 1 (a 5 x 4 map of 512 channels: 192 workgroups of 16-step chains instead of 4 of 144).
#include "ssdk_conv_common.h"
#include "../../include/ssdk_convt.h"

namespace ssdk {

constexpr int kConvtCB = 4;  // blocks of 16 output channels per workgroup (at most; ConvtParams::cpc)

struct ConvtParams {
  const u16* x;
  const u16* w;  // the four parity images, one behind the other
  const float* bias;
  const u16* skip;
  u16* y;
  int M, H, W, Cin, Cout, act;  // M = N * H * W input pixels
  int cblocks;                  // ceil(Cout / 16)
  int cpc;                      // channel blocks per workgroup: 1, 2 or 4
  int clsplit;                  // 1: blockIdx.z is the parity class; 0: a workgroup walks all four
  int ks[4];                    // k-steps of 32 per class image
  unsigned woff[4];             // first element of each class image
};

template <int DT, int PT>
__global__ __launch_bounds__(256) void convt3x3s2_kernel(const ConvtParams p) {
  __shared__ f32x4 red[4][PT * kConvtCB][64];  // [wave][fragment * 4 + channel block][lane]: 16 KiB (PT = 1) | 32 KiB (PT = 2)
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  const int l15 = lane & 15, l4 = lane >> 4;
  const long m0 = (long)blockIdx.x * (16 * PT);
  const int cb0 = (int)blockIdx.y * p.cpc;
  const int ncb = min(p.cpc, p.cblocks - cb0);
  const int Ho = 2 * p.H - 1, Wo = 2 * p.W - 1;
  bool pok[PT];
  int iy[PT], ix[PT];
  const u16* xp[PT];
  size_t yoff[PT];  // element offset of output pixel (2 iy, 2 ix), channel 0
#pragma unroll
  for (int i = 0; i < PT; ++i) {
    const long pix = m0 + 16 * i + l15;
    pok[i] = pix < p.M;
    const long pc = pok[i] ? pix : 0;
    const int n = (int)(pc / ((long)p.H * p.W)), r = (int)(pc % ((long)p.H * p.W));
    iy[i] = r / p.W;
    ix[i] = r % p.W;
    xp[i] = p.x + (size_t)pc * p.Cin;
    yoff[i] = (((size_t)n * Ho + 2 * iy[i]) * Wo + 2 * ix[i]) * p.Cout;
  }
  const int cls0 = p.clsplit ? (int)blockIdx.z : 0, cls1 = p.clsplit ? (int)blockIdx.z + 1 : 4;
  for (int cls = cls0; cls < cls1; ++cls) {  // (workgroup-uniform, like everything that decides whether a barrier is reached)
    const int py = cls >> 1, px = cls & 1;
    if ((py && p.H == 1) || (px && p.W == 1)) continue;  // an empty class
    const int ntaps = (1 + py) * (1 + px);
    bool ok[PT];
#pragma unroll
    for (int i = 0; i < PT; ++i) ok[i] = pok[i] && (!py || iy[i] < p.H - 1) && (!px || ix[i] < p.W - 1);
    f32x4 acc[PT][kConvtCB];
#pragma unroll
    for (int i = 0; i < PT; ++i)
#pragma unroll
      for (int b = 0; b < kConvtCB; ++b) acc[i][b] = f32x4{0.f, 0.f, 0.f, 0.f};
    const u16* wc = p.w + p.woff[cls];
    const int ksteps = p.ks[cls];
    int tap = 0, ci = 32 * wave + 8 * l4;  // this lane's octet of this wave's current k-step: k = tap * Cin + ci
    while (ci >= p.Cin) {
      ci -= p.Cin;
      ++tap;
    }
    for (int ks = wave; ks < ksteps; ks += 4) {
      u32x4 bf[PT];
      // tap = dy * (1 + px) + dx reads input pixel (iy + dy, ix + dx); past the last tap: the zero columns of the image
      const int dy = px ? tap >> 1 : tap, dx = px ? tap & 1 : 0;
      const int toff = (dy * p.W + dx) * p.Cin + ci;
#pragma unroll
      for (int i = 0; i < PT; ++i) {
        bf[i] = u32x4{0u, 0u, 0u, 0u};
        if (ok[i] && tap < ntaps) bf[i] = *reinterpret_cast<const u32x4*>(xp[i] + toff);
      }
#pragma unroll
      for (int b = 0; b < kConvtCB; ++b) {
        if (b < ncb) {
          const u32x4 af = *reinterpret_cast<const u32x4*>(wc + (((size_t)(cb0 + b) * ksteps + ks) * 64 + lane) * 8);
#pragma unroll
          for (int i = 0; i < PT; ++i) acc[i][b] = mfma16<DT>(af, bf[i], acc[i][b]);
        }
      }
      ci += 128;
      while (ci >= p.Cin) {
        ci -= p.Cin;
        ++tap;
      }
    }
    // the four waves' partial sums meet in LDS; wave b owns channel block b from here on
#pragma unroll
    for (int i = 0; i < PT; ++i)
#pragma unroll
      for (int b = 0; b < kConvtCB; ++b) red[wave][i * kConvtCB + b][lane] = acc[i][b];
    __syncthreads();
    // D: column (pixel) = lane & 15, rows (output channels) = 4 (lane >> 4) + 0..3 of the block
    const int co = (cb0 + wave) * 16 + 4 * l4;
    if (wave < ncb && co < p.Cout) {  // Cout is a multiple of 8: a group of 4 is all in or all out
      float4 bi = make_float4(0.f, 0.f, 0.f, 0.f);
      if (p.bias) bi = *reinterpret_cast<const float4*>(p.bias + co);
#pragma unroll
      for (int i = 0; i < PT; ++i) {
        if (!ok[i]) continue;
        const int e = i * kConvtCB + wave;
        const f32x4 a = ((red[0][e][lane] + red[1][e][lane]) + red[2][e][lane]) + red[3][e][lane];
        float v0 = apply_act(a[0] + bi.x, p.act), v1 = apply_act(a[1] + bi.y, p.act);
        float v2 = apply_act(a[2] + bi.z, p.act), v3 = apply_act(a[3] + bi.w, p.act);
        const size_t off = yoff[i] + ((size_t)py * Wo + px) * p.Cout + co;
        if (p.skip) {
          const uint2 rv = *reinterpret_cast<const uint2*>(p.skip + off);
          v0 += bits16_to_f32<DT>(rv.x & 0xffffu);
          v1 += bits16_to_f32<DT>(rv.x >> 16);
          v2 += bits16_to_f32<DT>(rv.y & 0xffffu);
          v3 += bits16_to_f32<DT>(rv.y >> 16);
        }
        *reinterpret_cast<uint2*>(p.y + off) = make_uint2(pack2_16<DT>(v0, v1), pack2_16<DT>(v2, v3));
      }
    }
    __syncthreads();  // the next class writes `red` again
  }
}

static bool convt_channels_ok(int Cin, int Cout) {
  return Cin >= 8 && Cout >= 8 && !(Cin % 8) && !(Cout % 8) && Cin <= (1 << 20) && Cout <= (1 << 20);
}

}  // namespace ssdk

using namespace ssdk;

extern "C" size_t ssdk_convt_desc_bytes(void) { return sizeof(ssdk_convt_desc); }

extern "C" size_t ssdk_convt_pack_bytes(int Cin, int Cout) {
  if (!convt_channels_ok(Cin, Cout)) return 0;
  size_t total = 0;
  for (int cls = 0; cls < 4; ++cls) {
    const int taps = (1 + (cls >> 1)) * (1 + (cls & 1));
    total += ssdk_weight_frag_bytes(Cout, 32 * ((taps * Cin + 31) / 32));
  }
  return total;
}

extern "C" int ssdk_convt3x3s2(const ssdk_convt_desc* d, void* stream) {
  if (!d) {
    set_error("convt3x3s2: null descriptor");
    return SSDK_E_BADARG;
  }
  if (d->dtype != SSDK_BF16 && d->dtype != SSDK_F16) {
    set_error("convt3x3s2: dtype must be bf16 or f16");
    return SSDK_E_BADARG;
  }
  if (d->N < 1 || d->N > 65535 || d->H < 1 || d->W < 1 || !convt_channels_ok(d->Cin, d->Cout)) {
    set_error("convt3x3s2: bad geometry N=%d H=%d W=%d Cin=%d Cout=%d (1 <= N <= 65535, H, W >= 1, Cin and Cout multiples of 8)",
              d->N, d->H, d->W, d->Cin, d->Cout);
    return SSDK_E_BADARG;
  }
  if (d->act < SSDK_ACT_NONE || d->act > SSDK_ACT_SIGMOID) {
    set_error("convt3x3s2: unknown activation %d", d->act);
    return SSDK_E_BADARG;
  }
  const long long M = (long long)d->N * d->H * d->W;
  if (M > 0x7fffffffLL - 1024 || (long long)d->H * d->W > 0x3fffffffLL) {
    set_error("convt3x3s2: more than 2^31 - 1 input pixels");
    return SSDK_E_BADARG;
  }
  const size_t pack_elems = ssdk_convt_pack_bytes(d->Cin, d->Cout) / 2;
  if (pack_elems > 0xffffffffull) {
    set_error("convt3x3s2: the weight images of Cin=%d Cout=%d exceed 2^32 elements", d->Cin, d->Cout);
    return SSDK_E_BADARG;
  }
  if (!d->x || !d->w_pack || !d->y) {
    set_error("convt3x3s2: null pointer (x, w_pack and y are required; bias and skip may be NULL)");
    return SSDK_E_BADARG;
  }
  if (((uintptr_t)d->x | (uintptr_t)d->w_pack | (uintptr_t)d->y | (uintptr_t)d->skip | (uintptr_t)d->bias) & 15) {
    set_error("convt3x3s2: x, w_pack, y, skip and bias must be 16-byte aligned");
    return SSDK_E_BADARG;
  }
  ConvtParams p;
  p.x = (const u16*)d->x;
  p.w = (const u16*)d->w_pack;
  p.bias = d->bias;
  p.skip = (const u16*)d->skip;
  p.y = (u16*)d->y;
  p.M = (int)M, p.H = d->H, p.W = d->W, p.Cin = d->Cin, p.Cout = d->Cout, p.act = d->act;
  p.cblocks = (d->Cout + 15) / 16;
  size_t off = 0;
  for (int cls = 0; cls < 4; ++cls) {
    const int taps = (1 + (cls >> 1)) * (1 + (cls & 1));
    p.ks[cls] = (taps * d->Cin + 31) / 32;
    p.woff[cls] = (unsigned)off;
    off += (size_t)p.cblocks * 16 * 32 * p.ks[cls];
  }
  // PT = 2 (32 pixels per workgroup: the weights are re-read once per 32 pixels) where that still gives 256 workgroups; else
  // 16 pixels, and while the grid is short of 256 the classes go to blockIdx.z and the channel blocks from 4 to 2 to 1
  const long long wg_target = 256;
  const bool big = ((M + 31) / 32) * ((p.cblocks + kConvtCB - 1) / kConvtCB) >= wg_target;
  const long long frags = big ? (M + 31) / 32 : (M + 15) / 16;
  p.cpc = kConvtCB;
  p.clsplit = 0;
  if (!big && frags * ((p.cblocks + p.cpc - 1) / p.cpc) < wg_target) {
    p.clsplit = 1;
    const long long live = (d->H > 1 ? 2 : 1) * (d->W > 1 ? 2 : 1);  // classes that have pixels
    while (p.cpc > 1 && frags * live * ((p.cblocks + p.cpc - 1) / p.cpc) < wg_target) p.cpc /= 2;
  }
  const dim3 grid((unsigned)frags, (unsigned)((p.cblocks + p.cpc - 1) / p.cpc), p.clsplit ? 4u : 1u);
  hipStream_t st = (hipStream_t)stream;
  if (d->dtype == SSDK_BF16) {
    if (big) hipLaunchKernelGGL((convt3x3s2_kernel<SSDK_BF16, 2>), grid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL((convt3x3s2_kernel<SSDK_BF16, 1>), grid, dim3(256), 0, st, p);
  } else {
    if (big) hipLaunchKernelGGL((convt3x3s2_kernel<SSDK_F16, 2>), grid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL((convt3x3s2_kernel<SSDK_F16, 1>), grid, dim3(256), 0, st, p);
  }
  return check_launch("convt3x3s2_kernel");
}
