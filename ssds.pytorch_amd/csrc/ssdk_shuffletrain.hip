// ssdk_shuffletrain.hip -- the ShuffleNetV2 TRAINING step on the NCHW tensors themselves (include/ssdk_shuffletrain.h):
//
//   ssdk_pws_forward   y[b] = a x[b] where x and / or y is a channel SLICE of a wider tensor (own image stride) and K, M are any
//                      values >= 8: the forward of a stride-1 unit's first 1x1 reads x[:, Cb:] where it lies (no chunk copy), and
//                      its input gradient is written into the last Cb channels of the unit's gradient buffer.  The branch widths
//                      of the backbone are 58 / 116 / 232 (x1) and 122 / 244 / 488 (x2): K tails of 2 and 4.
//   ssdk_pws_wgrad     dW = sum_b dy[b] x[b]^T with x such a slice
//   ssdk_pws_prepare   fp32 master weights -> the 16-bit matrix and its transpose, rows zero-padded to a multiple of 8
//   ssdk_shuffle_join_fwd / _bwd   y[2i] = left[i], y[2i + 1] = right[i] and its gradient: what chunk + cat + channel_shuffle do
//                      in three passes (~5 C HW 2 bytes) as one copy (2 C HW 2 bytes)
//
// Reference: torchvision's shufflenetv2.InvertedResidual as the reference's nets/shufflenet.py runs it in the training step
// (x.chunk(2, 1), torch.cat, channel_shuffle; 1x1 convolutions through nn.Conv2d).
//
// The GEMM kernels are those of ssdk_pwtrain.hip (ssdk_pwtrain_kernels.h) instantiated with SL = true: image strides for x and y, a
// leading dimension for a, and the K tail -- a lane's channels >= K are NEVER loaded (in a slice they are the next image's, behind
// the last image they lie outside the allocation) and the A fragments are masked to K columns, so the k-steps past K multiply
// zeros by zeros.  The weight-gradient kernels already guard rows >= Cin / Cout; they take the image stride of x.
#include "ssdk_pwtrain_kernels.h"

#include "../../include/ssdk_shuffletrain.h"

namespace ssdk {

template <int DT>
__global__ __launch_bounds__(256) void pws_prepare_kernel(const float* w32, u16* w16, u16* wt16, u32 cout, u32 cin, u32 kp, u32 mp) {
  const u32 i = blockIdx.x * 256u + threadIdx.x, n1 = cout * kp;
  if (i < n1) {
    const u32 co = i / kp, k = i - co * kp;
    w16[i] = k < cin ? (u16)f32_to_bits16<DT>(w32[(size_t)co * cin + k]) : (u16)0;
  } else if (i - n1 < cin * mp) {
    const u32 j = i - n1, ci = j / mp, m = j - ci * mp;
    wt16[j] = m < cout ? (u16)f32_to_bits16<DT>(w32[(size_t)m * cin + ci]) : (u16)0;
  }
}

struct JoinParams {
  const u16* even;  // forward: left;  backward: gy
  const u16* odd;   // forward: right
  u16* y;           // forward: y;     backward: unused
  u16* geven;       // backward: gleft or null
  u16* godd;        // backward: gright
  size_t es;        // elements between two images of left / gleft
  u32 N, Cb, HW;
};

// one thread = 8 consecutive pixels of one plane of the INTERLEAVED tensor (16-byte runs at any 2-byte alignment; the last run of
// a plane element by element).  BWD: the interleaved tensor is the source.
template <bool BWD>
__global__ __launch_bounds__(256) void shuffle_join_kernel(const JoinParams p) {
  const u32 vpr = (p.HW + 7u) / 8u, C = 2u * p.Cb;
  const size_t total = (size_t)p.N * C * vpr;
  for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < total; i += (size_t)gridDim.x * 256u) {
    const u32 v = (u32)(i % vpr), c = (u32)((i / vpr) % C), n = (u32)(i / ((size_t)vpr * C));
    const u32 p0 = v * 8u, h = c >> 1;
    const int nvalid = (int)p.HW - (int)p0;
    const size_t full = ((size_t)n * C + c) * p.HW + p0;
    const size_t left = (size_t)n * p.es + (size_t)h * p.HW + p0, right = ((size_t)n * p.Cb + h) * p.HW + p0;
    if constexpr (!BWD) {
      const u16* src = (c & 1u) ? p.odd + right : p.even + left;
      pw_store8<true>(p.y + full, pw_load8<true>(src, nvalid), nvalid);
    } else {
      u16* dst = (c & 1u) ? p.godd + right : (p.geven ? p.geven + left : nullptr);
      if (dst) pw_store8<true>(dst, pw_load8<true>(p.even + full, nvalid), nvalid);
    }
  }
}

}  // namespace ssdk

using namespace ssdk;

static bool pws_dtype(int dtype) { return dtype == SSDK_BF16 || dtype == SSDK_F16; }
static const size_t PWS_LIMIT = (size_t)1 << 32;

extern "C" int ssdk_pws_prepare(const float* w32, void* w16, void* wt16, int Cout, int Cin, int dtype, void* stream) {
  if (!w32 || !w16 || !wt16 || Cout < 1 || Cin < 1 || !pws_dtype(dtype) || (size_t)(Cout + 8) * (size_t)(Cin + 8) >= ((size_t)1 << 31)) {
    set_error("ssdk_pws_prepare: bad argument");
    return SSDK_E_BADARG;
  }
  const u32 kp = ((u32)Cin + 7u) / 8u * 8u, mp = ((u32)Cout + 7u) / 8u * 8u;
  const u32 n = (u32)Cout * kp + (u32)Cin * mp;
  if (dtype == SSDK_BF16)
    hipLaunchKernelGGL(pws_prepare_kernel<SSDK_BF16>, dim3((n + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, w32, (u16*)w16,
                       (u16*)wt16, (u32)Cout, (u32)Cin, kp, mp);
  else
    hipLaunchKernelGGL(pws_prepare_kernel<SSDK_F16>, dim3((n + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, w32, (u16*)w16,
                       (u16*)wt16, (u32)Cout, (u32)Cin, kp, mp);
  return check_launch("pws_prepare_kernel");
}

extern "C" size_t ssdk_pws_stats_workspace_bytes(int B, int K, int M, int HW) {
  if (B < 1 || K < 8 || M < 8 || HW < 1) return 0;
  PwtParams p;
  const PwtPlan pl = pw_gemm_plan(p, B, K, M, HW, true);
  const size_t rows = (size_t)pl.gx * 4;
  return (rows + (rows + 63) / 64) * (size_t)M * 2 * sizeof(float);
}

extern "C" int ssdk_pws_forward(const void* x, size_t x_image_stride, const void* a, int lda, const float* bias, void* y,
                                size_t y_image_stride, float* sums, void* workspace, size_t workspace_bytes, int B, int K, int M, int HW,
                                int dtype, void* stream) {
  if (!x || !a || !y || B < 1 || K < 8 || M < 8 || HW < 1 || !pws_dtype(dtype)) {
    set_error("ssdk_pws_forward: bad argument (16-bit tensors, K and M at least 8)");
    return SSDK_E_BADARG;
  }
  if (lda < K || (lda % 8) || (((uintptr_t)a) & 15)) {
    set_error("ssdk_pws_forward: the matrix needs lda >= K, lda a multiple of 8 and 16-byte alignment");
    return SSDK_E_BADARG;
  }
  if ((((uintptr_t)x) | ((uintptr_t)y)) & 1) {
    set_error("ssdk_pws_forward: misaligned tensor");
    return SSDK_E_BADARG;
  }
  if (x_image_stride < (size_t)K * (size_t)HW || y_image_stride < (size_t)M * (size_t)HW) {
    set_error("ssdk_pws_forward: an image stride is smaller than the slice");
    return SSDK_E_BADARG;
  }
  if (x_image_stride >= PWS_LIMIT || y_image_stride >= PWS_LIMIT || (size_t)B * x_image_stride >= PWS_LIMIT ||
      (size_t)B * y_image_stride >= PWS_LIMIT) {
    set_error("ssdk_pws_forward: tensor too large");
    return SSDK_E_BADARG;
  }
  hipStream_t st = (hipStream_t)stream;
  if (!sums)
    return pw_gemm_launch<true>(x, a, bias, y, B, K, M, HW, dtype, st, nullptr, nullptr, x_image_stride, y_image_stride, (unsigned)lda);
  if (!workspace || (((uintptr_t)workspace) & 15) || (((uintptr_t)sums) & 3)) {
    set_error("ssdk_pws_forward: sums need a 16-byte aligned workspace");
    return SSDK_E_BADARG;
  }
  if (workspace_bytes < ssdk_pws_stats_workspace_bytes(B, K, M, HW)) {
    set_error("ssdk_pws_forward: workspace too small");
    return SSDK_E_WORKSPACE;
  }
  unsigned rows = 0;
  int rc = pw_gemm_launch<true>(x, a, bias, y, B, K, M, HW, dtype, st, (float*)workspace, &rows, x_image_stride, y_image_stride,
                                (unsigned)lda);
  if (rc) return rc;
  const u32 n = (u32)M * 2u;
  return reduce_rows_fixed_order((const float*)workspace, (float*)workspace + (size_t)rows * n, sums, n, rows, st);
}

extern "C" size_t ssdk_pws_wgrad_workspace_bytes(int B, int Cout, int Cin, int HW) {
  if (B < 1 || Cout < 1 || Cin < 1 || HW < 1) return 0;
  PwgParams p;
  int mfw, nfw;
  pw_wgrad_plan(B, Cout, Cin, HW, &p, &mfw, &nfw);
  return ((size_t)p.splits + (size_t)((p.splits + 63u) / 64u)) * (size_t)Cout * (size_t)Cin * sizeof(float);
}

extern "C" int ssdk_pws_wgrad(const void* dy, const void* x, size_t x_image_stride, float* dw, void* workspace, size_t workspace_bytes,
                              int B, int Cout, int Cin, int HW, int dtype, void* stream) {
  if (!dy || !x || !dw || !workspace || B < 1 || Cout < 1 || Cin < 1 || HW < 1 || !pws_dtype(dtype) ||
      ((((uintptr_t)dy) | ((uintptr_t)x)) & 1) || ((((uintptr_t)dw) | ((uintptr_t)workspace)) & 3)) {
    set_error("ssdk_pws_wgrad: bad argument");
    return SSDK_E_BADARG;
  }
  if (x_image_stride < (size_t)Cin * (size_t)HW) {
    set_error("ssdk_pws_wgrad: the image stride is smaller than the slice");
    return SSDK_E_BADARG;
  }
  if (x_image_stride >= PWS_LIMIT || (size_t)B * x_image_stride >= PWS_LIMIT || (size_t)B * (size_t)Cout * (size_t)HW >= PWS_LIMIT ||
      (size_t)Cout * (size_t)Cin >= ((size_t)1 << 31)) {
    set_error("ssdk_pws_wgrad: tensor too large");
    return SSDK_E_BADARG;
  }
  return pw_wgrad_run(dy, x, x_image_stride, dw, workspace, workspace_bytes, B, Cout, Cin, HW, dtype, (hipStream_t)stream, "ssdk_pws_wgrad");
}

static int join_check(const void* a, const void* b, const void* c, size_t stride, bool strided, int N, int Cb, int HW, int dtype,
                      const char* what) {
  if (!a || !b || N < 1 || Cb < 1 || HW < 1 || !pws_dtype(dtype) || ((((uintptr_t)a) | ((uintptr_t)b) | ((uintptr_t)c)) & 1)) {
    set_error("%s: bad argument (16-bit tensors)", what);
    return SSDK_E_BADARG;
  }
  if (strided && stride < (size_t)Cb * (size_t)HW) {
    set_error("%s: the image stride is smaller than the slice", what);
    return SSDK_E_BADARG;
  }
  if ((size_t)N * 2 * (size_t)Cb * (size_t)HW >= PWS_LIMIT || (strided && (stride >= PWS_LIMIT || (size_t)N * stride >= PWS_LIMIT))) {
    set_error("%s: tensor too large", what);
    return SSDK_E_BADARG;
  }
  return SSDK_OK;
}

static unsigned join_grid(int N, int Cb, int HW) {
  const size_t total = (size_t)N * 2 * (size_t)Cb * (size_t)((HW + 7) / 8);
  const size_t wgs = (total + 255) / 256;
  return (unsigned)(wgs < 8192 ? wgs : 8192);  // (32 workgroups per CU: a grid-stride copy)
}

extern "C" int ssdk_shuffle_join_fwd(const void* left, size_t left_image_stride, const void* right, void* y, int N, int Cb, int HW,
                                     int dtype, void* stream) {
  if (!y) {
    set_error("ssdk_shuffle_join_fwd: bad argument (null output)");
    return SSDK_E_BADARG;
  }
  int rc = join_check(left, right, y, left_image_stride, true, N, Cb, HW, dtype, "ssdk_shuffle_join_fwd");
  if (rc) return rc;
  JoinParams p;
  p.even = (const u16*)left;
  p.odd = (const u16*)right;
  p.y = (u16*)y;
  p.geven = p.godd = nullptr;
  p.es = left_image_stride;
  p.N = (u32)N;
  p.Cb = (u32)Cb;
  p.HW = (u32)HW;
  hipLaunchKernelGGL(shuffle_join_kernel<false>, dim3(join_grid(N, Cb, HW)), dim3(256), 0, (hipStream_t)stream, p);
  return check_launch("shuffle_join_kernel");
}

extern "C" int ssdk_shuffle_join_bwd(const void* gy, void* gleft, size_t gleft_image_stride, void* gright, int N, int Cb, int HW,
                                     int dtype, void* stream) {
  int rc = join_check(gy, gright, gleft, gleft_image_stride, gleft != nullptr, N, Cb, HW, dtype, "ssdk_shuffle_join_bwd");
  if (rc) return rc;
  JoinParams p;
  p.even = (const u16*)gy;
  p.odd = nullptr;
  p.y = nullptr;
  p.geven = (u16*)gleft;
  p.godd = (u16*)gright;
  p.es = gleft ? gleft_image_stride : 0;
  p.N = (u32)N;
  p.Cb = (u32)Cb;
  p.HW = (u32)HW;
  hipLaunchKernelGGL(shuffle_join_kernel<true>, dim3(join_grid(N, Cb, HW)), dim3(256), 0, (hipStream_t)stream, p);
  return check_launch("shuffle_join_kernel (backward)");
}
