// ssdk_convttrain.hip -- the TRANSPOSED 3x3 / stride 2 / pad 1 convolution of the SSDShelf TRAINING step on gfx950 (include/
// ssdk_convttrain.h): forward + bias + skip map, input gradient, weight + bias gradient.
//
// Reference: the decoder step of ShelfPyramid (ssds/modeling/ssds/shelf.py), nn.ConvTranspose2d(C_{i-1}, C_i, 3, stride 2, padding 1,
// bias)(x) + xx[i]: x [N, Cin, H, W] -> y [N, Cout, 2H-1, 2W-1], w [Cin, Cout, 3, 3].  Tensors are bf16 | fp16, NCHW contiguous.
//
// The layer is, operand for operand, the adjoint of the dense 3x3 / stride 2 / pad 1 convolution Cout -> Cin on the (2H-1) x (2W-1)
// map whose OIHW weight is w as it lies in memory (O = Cin, I = Cout).  So the three directions are the three kernels of
// ssdk_conv3train.hip with the roles turned round, and the device templates are shared (ssdk_conv3train_kernels.h):
//
//   prepare          that convolution's two dense images, one launch (c3_prepare): its input-gradient image (taps flipped) is what
//                    the forward here reads, its forward image what the input gradient here reads.
//   forward          conv3_train_conv_kernel<DT, 1, T, EPI> -- that convolution's input gradient "by input-pixel parity": an output
//                    pixel (2a + py, 2b + px) sees the (1 + py)(1 + px) taps whose input pixel exists, 9 taps per 2 x 2 pixels, no
//                    zero-inserted x and no border masking (2H - 1 rows: the odd row after the last input row does not exist).  A wave
//                    keeps the four parity classes of its fragments, so a lane ends with eight CONSECUTIVE pixels of one output row:
//                    the EPI instance (new here) adds the bias and the eight skip elements to the fp32 accumulators and rounds once.
//                    Rows of the odd-sided maps (17, 33, 65) start at any 2-byte address, so skip and y move element by element; the
//                    four lane groups of a wave cover 32 consecutive pixels of a row.
//   input gradient   that convolution's stride-2 forward on gy, launched through c3_conv: the very instance the dense layers use.
//   weight + bias gradient   conv3_train_wgrad_kernel<DT, 2, CKL, GB> with x and dy swapped: gw comes out as [Cin][Cout][3][3], the
//                    ConvTranspose2d layout.  The GB instance (new here) also sums every gy element it stages, per channel, counted
//                    once by stride-2 ownership: the bias gradient costs no pass of its own.  Partial sums per pixel range go to the
//                    workspace behind the weight partials; convt_train_gb_reduce_kernel adds them in range order.
//
// Every kernel instance is launched from one translation unit: the shared instances stay in ssdk_conv3train.hip, whose entry points
// compute bit for bit what they did.
//
// Compiler figures for gfx950 (-Rpass-analysis=kernel-resource-usage; no scratch in any instance): see DESIGN.md 4.5i.
#include "ssdk_conv3train_kernels.h"

#include "../../include/ssdk_convttrain.h"

namespace ssdk {

// gb[c] = the per-range sums added in range order; one thread per channel
__global__ __launch_bounds__(256) void convt_train_gb_reduce_kernel(const float* part, float* gb, int C, int pitch, int splits) {
  const int c = (int)(blockIdx.x * 256u + threadIdx.x);
  if (c >= C) return;
  float s = 0.f;
  for (int q = 0; q < splits; ++q) s += part[(size_t)q * pitch + c];
  gb[c] = s;
}

static int ct_check(const char* what, int N, int Cin, int Cout, int H, int W, int dtype) {
  const bool ch_ok = Cin >= 16 && Cin <= 4096 && (Cin % 16) == 0 && Cout >= 16 && Cout <= 4096 && (Cout % 16) == 0;
  if (N < 1 || H < 1 || W < 1 || (dtype != SSDK_BF16 && dtype != SSDK_F16) || !ch_ok) {
    set_error("%s: built for transposed 3x3, stride 2, pad 1, Cin and Cout multiples of 16 in 16..4096, bf16|f16 NCHW tensors "
              "(N=%d Cin=%d Cout=%d H=%d W=%d dtype=%d)", what, N, Cin, Cout, H, W, dtype);
    return SSDK_E_BADARG;
  }
  const size_t lim = (size_t)1 << 31;
  if ((size_t)H >= lim || (size_t)W >= lim || (size_t)H * W >= lim) {
    set_error("%s: tensor too large (N=%d Cin=%d Cout=%d H=%d W=%d)", what, N, Cin, Cout, H, W);
    return SSDK_E_BADARG;
  }
  const size_t Ho = 2 * (size_t)H - 1, Wo = 2 * (size_t)W - 1;
  if (Ho * Wo >= lim || (size_t)N * Cin * H * W >= lim || (size_t)N * Cout * (Ho * Wo) >= lim) {
    set_error("%s: tensor too large: 2^31 elements or more (N=%d Cin=%d Cout=%d H=%d W=%d)", what, N, Cin, Cout, H, W);
    return SSDK_E_BADARG;
  }
  return SSDK_OK;
}

template <int DT>
static void ct_fwd_launch(const C3ConvParams& p, long grid, size_t lds, hipStream_t stream) {
  hipLaunchKernelGGL((conv3_train_conv_kernel<DT, 1, true, true>), dim3((unsigned)grid), dim3(256), lds, stream, p);
}

}  // namespace ssdk

using namespace ssdk;

extern "C" int ssdk_convt_train_prepare(const float* w32, void* w_fwd, void* w_dgrad, int Cin, int Cout, int dtype, void* stream) {
  if (int rc = ct_check("convt_train_prepare", 1, Cin, Cout, 1, 1, dtype)) return rc;
  if (!w32 || (!w_fwd && !w_dgrad) || (((uintptr_t)w_fwd | (uintptr_t)w_dgrad) & 15u) || ((uintptr_t)w32 & 3u)) {
    set_error("convt_train_prepare: null weights, no image asked for, or an image that is not 16-byte aligned");
    return SSDK_E_BADARG;
  }
  // the convolution Cout -> Cin: its forward image is this layer's input-gradient image, its input-gradient image this layer's forward's
  if (int rc = c3_prepare(w32, w_dgrad, w_fwd, Cout, Cin, dtype, (hipStream_t)stream)) return rc;
  return check_launch("convt_train_prepare_kernel");
}

extern "C" int ssdk_convt_train_forward(const void* x, const void* w_fwd, const float* bias, const void* skip, void* y, int N, int Cin,
                                        int Cout, int H, int W, int dtype, void* stream) {
  if (int rc = ct_check("convt_train_forward", N, Cin, Cout, H, W, dtype)) return rc;
  if (!x || !w_fwd || !y || ((uintptr_t)w_fwd & 15u) || (((uintptr_t)x | (uintptr_t)y | (uintptr_t)skip) & 1u) || ((uintptr_t)bias & 3u)) {
    set_error("convt_train_forward: null pointer, an image that is not 16-byte aligned, or a misaligned tensor / bias");
    return SSDK_E_BADARG;
  }
  C3ConvParams p;
  long grid;
  size_t lds;
  if (int rc = c3_conv_plan("convt_train_forward", x, w_fwd, bias, y, N, Cin, Cout, H, W, 2 * H - 1, 2 * W - 1, 2, true, &p, &grid, &lds))
    return rc;
  p.skip = (const u16*)skip;
  if (dtype == SSDK_BF16) ct_fwd_launch<SSDK_BF16>(p, grid, lds, (hipStream_t)stream);
  else ct_fwd_launch<SSDK_F16>(p, grid, lds, (hipStream_t)stream);
  return check_launch("convt_train_fwd_kernel");
}

extern "C" int ssdk_convt_train_dgrad(const void* gy, const void* w_dgrad, void* gx, int N, int Cin, int Cout, int H, int W, int dtype,
                                      void* stream) {
  if (int rc = ct_check("convt_train_dgrad", N, Cin, Cout, H, W, dtype)) return rc;
  if (!gy || !w_dgrad || !gx || ((uintptr_t)w_dgrad & 15u) || (((uintptr_t)gy | (uintptr_t)gx) & 1u)) {
    set_error("convt_train_dgrad: null pointer, an image that is not 16-byte aligned, or a misaligned tensor");
    return SSDK_E_BADARG;
  }
  if (int rc = c3_conv("convt_train_dgrad", gy, w_dgrad, nullptr, gx, N, Cout, Cin, 2 * H - 1, 2 * W - 1, H, W, 2, false, dtype,
                       (hipStream_t)stream))
    return rc;
  return check_launch("convt_train_dgrad_kernel");
}

// the weight-gradient plan of the convolution Cout -> Cin on the (2H-1) x (2W-1) map
static void ct_wgrad_plan(int N, int Cin, int Cout, int H, int W, C3WgradParams* p) {
  memset(p, 0, sizeof(*p));
  p->N = N;
  p->Ci = Cout;
  p->Co = Cin;
  p->H = 2 * H - 1;
  p->W = 2 * W - 1;
  p->Ho = H;
  p->Wo = W;
  c3_wgrad_plan(N, p->Ci, p->Co, p->Ho, p->Wo, p);
}

extern "C" size_t ssdk_convt_train_wgrad_workspace_bytes(int N, int Cin, int Cout, int H, int W) {
  if (ct_check("convt_train_wgrad_workspace_bytes", N, Cin, Cout, H, W, SSDK_BF16)) return 0;
  C3WgradParams p;
  ct_wgrad_plan(N, Cin, Cout, H, W, &p);
  return ((size_t)p.splits * p.ntiles * (9 * 4096) + (size_t)p.splits * p.tci * 64) * sizeof(float);
}

extern "C" int ssdk_convt_train_wgrad(const void* x, const void* gy, float* gw, float* gb, void* workspace, size_t workspace_bytes, int N,
                                      int Cin, int Cout, int H, int W, int dtype, void* stream) {
  if (int rc = ct_check("convt_train_wgrad", N, Cin, Cout, H, W, dtype)) return rc;
  const size_t need = ssdk_convt_train_wgrad_workspace_bytes(N, Cin, Cout, H, W);
  if (!x || !gy || !gw || !workspace || ((uintptr_t)workspace & 15u) || (((uintptr_t)x | (uintptr_t)gy) & 1u) ||
      (((uintptr_t)gw | (uintptr_t)gb) & 3u) || workspace_bytes < need) {
    set_error("convt_train_wgrad: null pointer, or workspace too small / misaligned (%zu bytes given, %zu needed)", workspace_bytes, need);
    return SSDK_E_BADARG;
  }
  C3WgradParams p;
  ct_wgrad_plan(N, Cin, Cout, H, W, &p);
  if (p.splits > 65535) {
    set_error("convt_train_wgrad: too many pixel ranges (%d)", p.splits);
    return SSDK_E_BADARG;
  }
  p.x = (const u16*)gy;  // the convolution's input is this layer's output gradient,
  p.dy = (const u16*)x;  // its output gradient this layer's input
  p.dw = gw;
  p.part = (float*)workspace;
  p.gbpart = gb ? p.part + (size_t)p.splits * p.ntiles * (9 * 4096) : nullptr;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)p.ntiles, (unsigned)p.splits);
#define SSDK_CT_W(DT)                                                                                                \
  do {                                                                                                               \
    if (p.ck_log2 == 2) hipLaunchKernelGGL((conv3_train_wgrad_kernel<DT, 2, 2, true>), grid, dim3(256), 0, st, p);      \
    else if (p.ck_log2 == 1) hipLaunchKernelGGL((conv3_train_wgrad_kernel<DT, 2, 1, true>), grid, dim3(256), 0, st, p); \
    else hipLaunchKernelGGL((conv3_train_wgrad_kernel<DT, 2, 0, true>), grid, dim3(256), 0, st, p);                     \
  } while (0)
  if (dtype == SSDK_BF16) SSDK_CT_W(SSDK_BF16);
  else SSDK_CT_W(SSDK_F16);
#undef SSDK_CT_W
  c3_wgrad_reduce(p, st);
  if (gb)
    hipLaunchKernelGGL(convt_train_gb_reduce_kernel, dim3((unsigned)((Cout + 255) / 256)), dim3(256), 0, st, p.gbpart, gb, Cout, 64 * p.tci,
                       p.splits);
  return check_launch("convt_train_wgrad_kernel");
}
