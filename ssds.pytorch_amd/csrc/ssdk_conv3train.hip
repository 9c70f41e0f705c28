// ssdk_conv3train.hip -- the DENSE 3x3 convolution of the TRAINING step on gfx950: forward (+ bias), input gradient, weight gradient.
//
// Reference: the towers, smoothing and head convolutions of SSDFPN / SSDBiFPN (ssds/modeling/ssds/fpn.py, bifpn.py), the 3x3 of the
// ResNet bottlenecks (nets/resnet.py) and the extras, inside the DDP step.  pad 1, stride 1 | 2, Cin a multiple of 16 (16 .. 4096),
// Cout a multiple of 4 (4 .. 4096), independent of each other.  Tensors are bf16 | fp16, NCHW contiguous in and out (the layout of the
// 1x1, grouped 3x3 and BatchNorm kernels around the layer), fp32 accumulation on mfma16<DT>.  No BatchNorm fold, no activation.
// The one-group case ssdk_gconvtrain.hip cannot reach (gw <= 256, Cin == Cout there).
//
//   prepare   conv3_train_prepare_kernel: the fp32 master weight [Cout, Cin, 3, 3] -> two 16-bit dense images (include/ssdk.h, "dense
//             3x3 image"): the forward image and the input-gradient image (transposed, taps flipped).  Replaces autocast's cast.
//   forward / input gradient   conv3_train_conv_kernel<DT, S, T>: an implicit GEMM.  A workgroup (4 waves) owns a patch of 2 FT
//             fragments of 16 output pixels (a fragment is 16 / TW rows x TW columns, TW = 16 | 8 | 4 by the map's width, so that
//             narrow maps put several rows into one fragment) x 64 output channels, and loops over the input channels in chunks of 32.
//             The halo of a chunk lives in LDS as four planes [8-channel group][pixel][8 channels] (a lane's A operand is one
//             ds_read_b128; the plane pitch is a multiple of 256 B, + 16 B at stride 2, which keeps the four lane groups of the read
//             on different banks), double-buffered: the next chunk's global loads are in flight while the matrix cores work on this
//             one, one barrier per chunk.  The accumulators persist over the whole K = 9 Cin.  Operand roles as
//             gconv_train_conv_kernel: A = pixels, B = weights streamed from the image, so a lane's four accumulator values are four
//             consecutive pixels of ONE channel, an 8-byte store along W.  The bias is added in fp32 before the single rounding.
//             A wave is (FT fragments) x (2 blocks of 16 channels); FT = 4 at stride 1, 2 at stride 2.  (Four blocks per wave, a
//             128-channel tile, compile to 84 + 96 registers, 2 waves per SIMD, and halve the LDS reads per MFMA: to be tried
//             once the kernel can be timed.)
//             The last chunk of a Cin that is no multiple of 32 (912), and the channels that pad Cout to 16 in the input-gradient
//             image (36, 720), are zeros in LDS and masked weight loads.
//             T (input gradient at stride 2) is a real transposed convolution by input-pixel parity: an input pixel (2a + py, 2b + px)
//             sees the (1 + py)(1 + px) taps whose output pixel exists, 9 taps per 2 x 2 pixels, no zero-dilated dy.  A wave keeps the
//             four parity classes of its fragments and interleaves the two column parities into one 16-byte store.
//             Stride-1 input gradient = the forward kernel on the input-gradient image with Cin and Cout swapped.
//             The halo is staged with 2-byte loads (64 lanes on 64 consecutive pixels of a channel row), eight channels packed in
//             registers into one ds_write_b128; the 16-byte row loads + register transpose of ssdk_pwtrain.hip are not used yet.
//   weight gradient   conv3_train_wgrad_kernel<DT, S, CKL>: dW[co][ci][tap] = sum over pixels dy[co][p] x[ci][p + tap] contracts over
//             pixels, contiguous along W in both operands.  A workgroup owns a 64 x 64 (co, ci) tile, all nine taps, and a range of
//             output rows; a wave a 32 x 32 quarter (36 accumulators).  A k-step is 32 pixels (4 >> CKL rows x (1 << CKL) groups of
//             eight): the dy rows and the three x rows behind them are copied into LDS as they lie in memory (no transpose), shared
//             by the four waves; the three kx shifts come from one row window (v_alignbit at stride 1, v_perm even / odd pick at
//             stride 2).  The next step's global loads are issued before the MFMAs of this one.  The fp32 partial tiles go to
//             caller-owned workspace [split][tile][9][64][64]; conv3_train_wgrad_reduce_kernel adds them in split order: no float
//             atomics, bit-reproducible.
//
// The device templates, parameter blocks and launch plans live in ssdk_conv3train_kernels.h, shared with ssdk_convttrain.hip (the adjoint
// layer: the transposed 3x3 / stride 2 of the Shelf decoder, which adds an epilogue to the stride-2 input gradient and a bias sum to the
// stride-2 weight pass as template parameters that are off here).  This file keeps the prepare and reduce kernels, the launchers of its
// own instances -- c3_prepare, c3_conv and c3_wgrad_reduce are called from there too -- and the entry points.
//
// Compiler figures for gfx950 (-Rpass-analysis=kernel-resource-usage; bf16 / fp16 within 3 VGPRs; no scratch in any instance; the LDS
// of the conv kernel is dynamic, 2 buffers x 4 planes; VGPRs + AGPRs, LDS per workgroup, waves per SIMD):
//   conv, forward / stride-1 input gradient  <S = 1>  70 + 48, 24.0 KiB (26.0 at TW = 4), 4
//   conv, forward stride 2                   <S = 2>  80 + 24, 38.1 KiB, 4
//   conv, stride-2 input gradient            <T>      84 + 68, 12.0 KiB, 3
//   wgrad stride 1, CKL = 2 / 1 / 0: 130 / 141 / 162 + 144, 18.8 / 20.3 / 23.3 KiB, 1 wave per SIMD
//   wgrad stride 2, CKL = 2 / 1 / 0: 207 / 234 / 237 + 144, 30.8 / 32.3 / 35.3 KiB, 1 wave per SIMD
//   prepare 12, reduce 12 VGPRs, no LDS, 8
#include "ssdk_conv3train_kernels.h"

namespace ssdk {

template <int DT>
__global__ __launch_bounds__(256) void conv3_train_prepare_kernel(const C3PrepParams p) {
  const u32 idx = blockIdx.x * 256u + threadIdx.x;
  const int which = (int)blockIdx.y;
  u16* out = p.img[which];
  if (!out || idx >= p.total[which]) return;
  // image element [row block][k-step][k % 32 / 8][row % 16][k % 8], k = tap * Cp + channel
  const int e8 = (int)(idx & 7u), r16 = (int)((idx >> 3) & 15u), c4 = (int)((idx >> 7) & 3u);
  const int blk = (int)(idx >> 9), KS = p.KS[which], Cp = p.Cp[which];
  const int ks = blk % KS, rb = blk / KS;
  const int row = rb * 16 + r16, k = ks * 32 + c4 * 8 + e8, tap = k / Cp, c = k - tap * Cp;
  float v = 0.f;
  if (which == 0) {  // rows: output channels, channels: input channels
    if (row < p.Co && tap < 9 && c < p.Ci) v = p.w[((size_t)row * p.Ci + c) * 9 + tap];
  } else {  // rows: input channels, channels: output channels, taps flipped
    if (row < p.Ci && tap < 9 && c < p.Co) v = p.w[((size_t)c * p.Ci + row) * 9 + (8 - tap)];
  }
  out[idx] = (u16)f32_to_bits16<DT>(v);
}

int c3_prepare(const float* w32, void* w_fwd, void* w_dgrad, int Cin, int Cout, int dtype, hipStream_t stream) {
  C3PrepParams p;
  p.w = w32;
  p.img[0] = (u16*)w_fwd;
  p.img[1] = (u16*)w_dgrad;
  p.Ci = Cin;
  p.Co = Cout;
  p.Cp[0] = Cin;
  p.Cp[1] = c3_up(Cout, 16);
  p.KS[0] = (9 * p.Cp[0] + 31) / 32;
  p.KS[1] = (9 * p.Cp[1] + 31) / 32;
  const size_t t0 = (size_t)((Cout + 15) / 16) * p.KS[0] * 512, t1 = (size_t)(Cin / 16) * p.KS[1] * 512;
  p.total[0] = (u32)t0;
  p.total[1] = (u32)t1;
  const size_t total = t0 > t1 ? t0 : t1;
  const dim3 grid((unsigned)((total + 255) / 256), 2);
  if (dtype == SSDK_BF16) hipLaunchKernelGGL((conv3_train_prepare_kernel<SSDK_BF16>), grid, dim3(256), 0, stream, p);
  else hipLaunchKernelGGL((conv3_train_prepare_kernel<SSDK_F16>), grid, dim3(256), 0, stream, p);
  return check_launch("conv3_train_prepare_kernel");
}

template <int DT, int S, bool T>
static void c3_conv_launch(const C3ConvParams& p, long grid, size_t lds, hipStream_t stream) {
  hipLaunchKernelGGL((conv3_train_conv_kernel<DT, S, T>), dim3((unsigned)grid), dim3(256), lds, stream, p);
}

int c3_conv(const char* what, const void* x, const void* wf, const float* bias, void* y, int N, int Ci, int Co, int H, int W, int Ho,
            int Wo, int stride, bool transposed, int dtype, hipStream_t stream) {
  C3ConvParams p;
  long grid;
  size_t lds;
  if (int rc = c3_conv_plan(what, x, wf, bias, y, N, Ci, Co, H, W, Ho, Wo, stride, transposed, &p, &grid, &lds)) return rc;
  const int S = transposed ? 1 : stride;
  if (dtype == SSDK_BF16) {
    if (transposed) c3_conv_launch<SSDK_BF16, 1, true>(p, grid, lds, stream);
    else if (S == 1) c3_conv_launch<SSDK_BF16, 1, false>(p, grid, lds, stream);
    else c3_conv_launch<SSDK_BF16, 2, false>(p, grid, lds, stream);
  } else {
    if (transposed) c3_conv_launch<SSDK_F16, 1, true>(p, grid, lds, stream);
    else if (S == 1) c3_conv_launch<SSDK_F16, 1, false>(p, grid, lds, stream);
    else c3_conv_launch<SSDK_F16, 2, false>(p, grid, lds, stream);
  }
  return SSDK_OK;
}

// dw = the partial tiles added in split order; one thread per tile element
__global__ __launch_bounds__(256) void conv3_train_wgrad_reduce_kernel(const C3WgradParams p) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t per = (size_t)p.ntiles * (9 * 4096);
  if (i >= per) return;
  float s = 0.f;
  for (int q = 0; q < p.splits; ++q) s += p.part[(size_t)q * per + i];
  const int tile = (int)(i / (9 * 4096)), r = (int)(i % (9 * 4096));
  const int t = r >> 12, m = (r >> 6) & 63, nn = r & 63;
  const int co = (tile / p.tci) * 64 + m, ci = (tile % p.tci) * 64 + nn;
  if (co >= p.Co || ci >= p.Ci) return;
  p.dw[((size_t)co * p.Ci + ci) * 9 + t] = s;
}

void c3_wgrad_reduce(const C3WgradParams& p, hipStream_t stream) {
  const size_t per = (size_t)p.ntiles * (9 * 4096);
  hipLaunchKernelGGL(conv3_train_wgrad_reduce_kernel, dim3((unsigned)((per + 255) / 256)), dim3(256), 0, stream, p);
}

}  // namespace ssdk


using namespace ssdk;

extern "C" int ssdk_conv3x3_train_prepare(const float* w32, void* w_fwd, void* w_dgrad, int Cin, int Cout, int dtype, void* stream) {
  if (int rc = c3_check("conv3x3_train_prepare", 1, Cin, Cout, 1, 1, 1, dtype)) return rc;
  if (!w32 || (!w_fwd && !w_dgrad) || (((uintptr_t)w_fwd | (uintptr_t)w_dgrad) & 15u) || ((uintptr_t)w32 & 3u)) {
    set_error("conv3x3_train_prepare: null weights, no image asked for, or an image that is not 16-byte aligned");
    return SSDK_E_BADARG;
  }
  return c3_prepare(w32, w_fwd, w_dgrad, Cin, Cout, dtype, (hipStream_t)stream);
}

extern "C" int ssdk_conv3x3_train_forward(const void* x, const void* w_fwd, const float* bias, void* y, int N, int Cin, int Cout, int H, int W,
                                          int stride, int dtype, void* stream) {
  if (int rc = c3_check("conv3x3_train_forward", N, Cin, Cout, H, W, stride, dtype)) return rc;
  if (!x || !w_fwd || !y || ((uintptr_t)w_fwd & 15u) || (((uintptr_t)x | (uintptr_t)y) & 1u) || ((uintptr_t)bias & 3u)) {
    set_error("conv3x3_train_forward: null pointer, an image that is not 16-byte aligned, or a misaligned tensor / bias");
    return SSDK_E_BADARG;
  }
  const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
  if (int rc = c3_conv("conv3x3_train_forward", x, w_fwd, bias, y, N, Cin, Cout, H, W, Ho, Wo, stride, false, dtype, (hipStream_t)stream))
    return rc;
  return check_launch("conv3_train_fwd_kernel");
}

extern "C" int ssdk_conv3x3_train_dgrad(const void* dy, const void* w_dgrad, void* dx, int N, int Cin, int Cout, int H, int W, int stride,
                                        int dtype, void* stream) {
  if (int rc = c3_check("conv3x3_train_dgrad", N, Cin, Cout, H, W, stride, dtype)) return rc;
  if (!dy || !w_dgrad || !dx || ((uintptr_t)w_dgrad & 15u) || (((uintptr_t)dy | (uintptr_t)dx) & 1u)) {
    set_error("conv3x3_train_dgrad: null pointer, an image that is not 16-byte aligned, or a misaligned tensor");
    return SSDK_E_BADARG;
  }
  const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
  hipStream_t st = (hipStream_t)stream;
  int rc;
  if (stride == 1) rc = c3_conv("conv3x3_train_dgrad", dy, w_dgrad, nullptr, dx, N, Cout, Cin, H, W, H, W, 1, false, dtype, st);
  else rc = c3_conv("conv3x3_train_dgrad", dy, w_dgrad, nullptr, dx, N, Cout, Cin, Ho, Wo, H, W, 2, true, dtype, st);
  if (rc) return rc;
  return check_launch(stride == 1 ? "conv3_train_dgrad_kernel" : "conv3_train_dgrad_s2_kernel");
}

extern "C" size_t ssdk_conv3x3_train_wgrad_workspace_bytes(int N, int Cin, int Cout, int H, int W, int stride) {
  if (N < 1 || H < 1 || W < 1 || (stride != 1 && stride != 2) || !c3_shape_ok(Cin, Cout)) return 0;
  C3WgradParams p;
  c3_wgrad_plan(N, Cin, Cout, (H - 1) / stride + 1, (W - 1) / stride + 1, &p);
  return (size_t)p.splits * p.ntiles * (9 * 4096) * sizeof(float);
}

extern "C" int ssdk_conv3x3_train_wgrad(const void* x, const void* dy, float* dw, void* workspace, size_t workspace_bytes, int N, int Cin,
                                        int Cout, int H, int W, int stride, int dtype, void* stream) {
  if (int rc = c3_check("conv3x3_train_wgrad", N, Cin, Cout, H, W, stride, dtype)) return rc;
  const size_t need = ssdk_conv3x3_train_wgrad_workspace_bytes(N, Cin, Cout, H, W, stride);
  if (!x || !dy || !dw || !workspace || ((uintptr_t)workspace & 15u) || (((uintptr_t)x | (uintptr_t)dy) & 1u) || ((uintptr_t)dw & 3u) ||
      workspace_bytes < need) {
    set_error("conv3x3_train_wgrad: null pointer, or workspace too small / misaligned (%zu bytes given, %zu needed)", workspace_bytes, need);
    return SSDK_E_BADARG;
  }
  C3WgradParams p;
  memset(&p, 0, sizeof(p));
  p.x = (const u16*)x;
  p.dy = (const u16*)dy;
  p.dw = dw;
  p.part = (float*)workspace;
  p.N = N;
  p.Ci = Cin;
  p.Co = Cout;
  p.H = H;
  p.W = W;
  p.Ho = (H - 1) / stride + 1;
  p.Wo = (W - 1) / stride + 1;
  c3_wgrad_plan(N, Cin, Cout, p.Ho, p.Wo, &p);
  if (p.splits > 65535) {
    set_error("conv3x3_train_wgrad: too many pixel ranges (%d)", p.splits);
    return SSDK_E_BADARG;
  }
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)p.ntiles, (unsigned)p.splits);
#define SSDK_C3_W(DT, S)                                                                                    \
  do {                                                                                                      \
    if (p.ck_log2 == 2) hipLaunchKernelGGL((conv3_train_wgrad_kernel<DT, S, 2>), grid, dim3(256), 0, st, p); \
    else if (p.ck_log2 == 1) hipLaunchKernelGGL((conv3_train_wgrad_kernel<DT, S, 1>), grid, dim3(256), 0, st, p); \
    else hipLaunchKernelGGL((conv3_train_wgrad_kernel<DT, S, 0>), grid, dim3(256), 0, st, p);               \
  } while (0)
  if (dtype == SSDK_BF16) {
    if (stride == 1) SSDK_C3_W(SSDK_BF16, 1);
    else SSDK_C3_W(SSDK_BF16, 2);
  } else {
    if (stride == 1) SSDK_C3_W(SSDK_F16, 1);
    else SSDK_C3_W(SSDK_F16, 2);
  }
#undef SSDK_C3_W
  c3_wgrad_reduce(p, st);
  return check_launch("conv3_train_wgrad_kernel");
}
