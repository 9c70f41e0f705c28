// ssdk_densetrain.hip -- the DenseNet dense block of the TRAINING step on ONE feature buffer F [N][Ctot][HW] and one gradient buffer G
// (include/ssdk_densetrain.h):
//
//   ssdk_dense_train_place        t -> a channel slice of F, + (sum, sum of squares) per channel of what was stored: channel c of the
//                                 block holds the same data for every later layer, so the batch statistics of all their norm1 layers
//                                 are computed ONCE, when the channel is written; norm1 of layer j is a finalize over a prefix of the
//                                 block's [Ctot][2] sums (ssdk_bn_act_train_stats with `sums`)
//   ssdk_dense_train_pw_forward   m = W1 op(F[:, :K]),  op(x) = round(max(fmaf(a, x, b), 0)): norm1 + relu1 applied while the 1x1 stages
//                                 its operand; relu(norm1(x)) -- Cin_j channels per layer, quadratic in the depth of a block -- is never
//                                 written.  The kernels of ssdk_pws_forward (ssdk_pwtrain_kernels.h) instantiated with AF = true.
//   ssdk_dense_train_pw_wgrad     dW1 = sum_b dm[b] op(x[b])^T, the kernels of ssdk_pws_wgrad with AF = true
//   ssdk_dense_train_bn1_reduce   (sum g, sum g xhat) per channel of norm1's backward, g = (W1^T dm) masked by the ReLU
//   ssdk_dense_train_bn1_apply    G[:, :K] += norm1's input gradient (read, add in fp32, round once)
//
// Reference: torchvision's densenet._DenseLayer / _DenseBlock as the reference's nets/densenet.py runs them in the training step
// (torch.cat of all earlier features, nn.BatchNorm2d over the concatenation, per layer).
//
// The three memory-bound kernels read and write planes as runs of 8 elements (16 bytes at any 2-byte alignment: a slice starts
// K * HW * 2 bytes into its tensor) and the last run of a plane element by element (pw_load8 / pw_store8 with TAIL).  No lane
// touches a channel >= C of a slice or a pixel >= HW of a plane.
#include "ssdk_pwtrain_kernels.h"

#include "../../include/ssdk_densetrain.h"

namespace ssdk {

struct DenseRedParams {
  const u16* t;       // place: the source [N][C][HW];  bn1: s [N][C][HW]
  const u16* x;       // bn1: the prefix of F
  u16* y;             // place: the slice of F;  bn1_apply: the prefix of G
  size_t xs, ys;      // image strides of x / y
  const float* coef;  // [C][4]
  const float* mean;
  const float* invstd;
  const float* weight;
  const float* red;   // bn1_apply: [C][2]
  float* partial;     // [C][S][2]
  u32 N, C, HW, S;
};

// images n = s, s + S, ... of a channel go to workgroup (c, s): S such that the chip sees ~2048 workgroups, at most one per image
static u32 dense_split(int N, int C) {
  u32 s = (2048u + (u32)C - 1u) / (u32)C;
  if (s > (u32)N) s = (u32)N;
  if (s > 64u) s = 64u;
  return s < 1u ? 1u : s;
}

// fixed order: the lane's own chain, the xor butterfly over the wave, the four waves in order
__device__ __forceinline__ void dense_block_sum2(float& a, float& b, float (*red)[2]) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    a += __shfl_xor(a, d, 64);
    b += __shfl_xor(b, d, 64);
  }
  const u32 lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  if (lane == 0u) {
    red[wave][0] = a;
    red[wave][1] = b;
  }
  __syncthreads();
  a = ((red[0][0] + red[1][0]) + red[2][0]) + red[3][0];
  b = ((red[0][1] + red[1][1]) + red[2][1]) + red[3][1];
}

// MODE 0 (place): copy + (sum v, sum v^2).  MODE 1 (bn1_reduce): (sum g, sum g xhat).
// Workgroup (c, s); its items are (image, run of 8 pixels) pairs, item i = tid, tid + 256, ... in that order per thread.
template <int DT, int MODE>
__global__ __launch_bounds__(256) void dense_reduce_kernel(const DenseRedParams p) {
  __shared__ float red[4][2];
  const u32 c = blockIdx.x, s = blockIdx.y;
  const u32 vpr = (p.HW + 7u) / 8u;
  const u32 nimg = (p.N - s + p.S - 1u) / p.S;  // images of this workgroup (s < S <= N)
  const u32 items = nimg * vpr;
  float ca = 0.f, cb = 0.f, mean = 0.f, istd = 0.f;
  if constexpr (MODE == 1) {
    ca = p.coef[4u * c];
    cb = p.coef[4u * c + 1u];
    mean = p.mean[c];
    istd = p.invstd[c];
  }
  float a = 0.f, b = 0.f;
  for (u32 i = threadIdx.x; i < items; i += 256u) {
    const u32 n = s + p.S * (i / vpr), p0 = (i % vpr) * 8u;
    const int nvalid = (int)p.HW - (int)p0;
    const u32x4 tv = pw_load8<true>(p.t + ((size_t)n * p.C + c) * p.HW + p0, nvalid);
    u32x4 xv = tv;
    if constexpr (MODE == 0) pw_store8<true>(p.y + (size_t)n * p.ys + (size_t)c * p.HW + p0, tv, nvalid);
    else xv = pw_load8<true>(p.x + (size_t)n * p.xs + (size_t)c * p.HW + p0, nvalid);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      if (e < nvalid) {
        const float tf = bits16_to_f32<DT>((e & 1) ? (tv[e >> 1] >> 16) : (tv[e >> 1] & 0xffffu));
        if constexpr (MODE == 0) {
          a += tf;
          b += tf * tf;
        } else {
          const float xf = bits16_to_f32<DT>((e & 1) ? (xv[e >> 1] >> 16) : (xv[e >> 1] & 0xffffu));
          const float g = __builtin_fmaf(ca, xf, cb) > 0.f ? tf : 0.f;
          const float xh = (xf - mean) * istd;
          a += g;
          b += g * xh;
        }
      }
    }
  }
  dense_block_sum2(a, b, red);
  if (threadIdx.x == 0u) {
    p.partial[((size_t)c * p.S + s) * 2u + 0u] = a;
    p.partial[((size_t)c * p.S + s) * 2u + 1u] = b;
  }
}

// out[c] = the S partials of channel c added in index order
__global__ __launch_bounds__(64) void dense_finalize_kernel(const float* partial, float* out, u32 C, u32 S) {
  const u32 c = blockIdx.x * 64u + threadIdx.x;
  if (c >= C) return;
  float a = partial[(size_t)c * S * 2u], b = partial[(size_t)c * S * 2u + 1u];
  for (u32 s = 1; s < S; ++s) {
    a += partial[((size_t)c * S + s) * 2u];
    b += partial[((size_t)c * S + s) * 2u + 1u];
  }
  out[2u * c] = a;
  out[2u * c + 1u] = b;
}

// one thread = 8 consecutive pixels of one plane of the prefix, grid-stride
template <int DT>
__global__ __launch_bounds__(256) void dense_bn1_apply_kernel(const DenseRedParams p) {
  const u32 vpr = (p.HW + 7u) / 8u;
  const size_t total = (size_t)p.N * p.C * vpr;
  const float cnt = (float)p.N * (float)p.HW;
  for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < total; i += (size_t)gridDim.x * 256u) {
    const u32 v = (u32)(i % vpr), c = (u32)((i / vpr) % p.C), n = (u32)(i / ((size_t)vpr * p.C));
    const u32 p0 = v * 8u;
    const int nvalid = (int)p.HW - (int)p0;
    const float ca = p.coef[4u * c], cb = p.coef[4u * c + 1u], mean = p.mean[c], istd = p.invstd[c];
    const float scale = p.weight[c] * istd, kb = p.red[2u * c] / cnt, kg = p.red[2u * c + 1u] / cnt;
    const u32x4 sv = pw_load8<true>(p.t + ((size_t)n * p.C + c) * p.HW + p0, nvalid);
    const u32x4 xv = pw_load8<true>(p.x + (size_t)n * p.xs + (size_t)c * p.HW + p0, nvalid);
    u16* gp = p.y + (size_t)n * p.ys + (size_t)c * p.HW + p0;
    const u32x4 gv = pw_load8<true>(gp, nvalid);
    float o[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const u32 sh = (e & 1) ? 16u : 0u;
      const float sf = bits16_to_f32<DT>((sv[e >> 1] >> sh) & 0xffffu), xf = bits16_to_f32<DT>((xv[e >> 1] >> sh) & 0xffffu);
      const float gf = bits16_to_f32<DT>((gv[e >> 1] >> sh) & 0xffffu);
      const float g = __builtin_fmaf(ca, xf, cb) > 0.f ? sf : 0.f;
      const float xh = (xf - mean) * istd;
      o[e] = gf + scale * ((g - kb) - xh * kg);
    }
    const u32x4 ov = {pack2_16<DT>(o[0], o[1]), pack2_16<DT>(o[2], o[3]), pack2_16<DT>(o[4], o[5]), pack2_16<DT>(o[6], o[7])};
    pw_store8<true>(gp, ov, nvalid);
  }
}

}  // namespace ssdk

using namespace ssdk;

static bool dn_dtype(int dtype) { return dtype == SSDK_BF16 || dtype == SSDK_F16; }
static const size_t DN_LIMIT = (size_t)1 << 32;

// a C-channel tensor of N images, contiguous or `stride` apart: sizes the kernels index with 32 bits
static bool dn_fits(int N, int C, int HW, size_t stride) {
  return (size_t)C * (size_t)HW <= stride && stride < DN_LIMIT && (size_t)N * stride < DN_LIMIT;
}

static size_t dn_red_bytes(int N, int C) { return (size_t)C * dense_split(N, C) * 2 * sizeof(float); }

extern "C" size_t ssdk_dense_train_place_workspace_bytes(int N, int C, int HW) {
  if (N < 1 || C < 1 || HW < 1) return 0;
  return dn_red_bytes(N, C);
}

extern "C" size_t ssdk_dense_train_bn1_workspace_bytes(int N, int K, int HW) {
  if (N < 1 || K < 1 || HW < 1) return 0;
  return dn_red_bytes(N, K);
}

extern "C" int ssdk_dense_train_place(const void* t, void* y, size_t y_image_stride, float* sums, void* workspace, size_t workspace_bytes,
                                      int N, int C, int HW, int dtype, void* stream) {
  if (!t || !y || !sums || !workspace || N < 1 || C < 1 || HW < 1 || !dn_dtype(dtype) || ((((uintptr_t)t) | ((uintptr_t)y)) & 1) ||
      (((uintptr_t)sums) & 3) || (((uintptr_t)workspace) & 15) || (size_t)C >= ((size_t)1 << 16)) {
    set_error("ssdk_dense_train_place: bad argument (16-bit tensors, a 16-byte aligned workspace)");
    return SSDK_E_BADARG;
  }
  if (y_image_stride < (size_t)C * (size_t)HW) {
    set_error("ssdk_dense_train_place: the image stride is smaller than the slice");
    return SSDK_E_BADARG;
  }
  if (!dn_fits(N, C, HW, y_image_stride)) {
    set_error("ssdk_dense_train_place: tensor too large");
    return SSDK_E_BADARG;
  }
  if (workspace_bytes < dn_red_bytes(N, C)) {
    set_error("ssdk_dense_train_place: workspace too small");
    return SSDK_E_WORKSPACE;
  }
  DenseRedParams p = {};
  p.t = (const u16*)t;
  p.y = (u16*)y;
  p.ys = y_image_stride;
  p.partial = (float*)workspace;
  p.N = (u32)N;
  p.C = (u32)C;
  p.HW = (u32)HW;
  p.S = dense_split(N, C);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)C, p.S);
  if (dtype == SSDK_BF16) hipLaunchKernelGGL((dense_reduce_kernel<SSDK_BF16, 0>), grid, dim3(256), 0, st, p);
  else hipLaunchKernelGGL((dense_reduce_kernel<SSDK_F16, 0>), grid, dim3(256), 0, st, p);
  int rc = check_launch("dense_reduce_kernel (place)");
  if (rc) return rc;
  hipLaunchKernelGGL(dense_finalize_kernel, dim3(((unsigned)C + 63u) / 64u), dim3(64), 0, st, (const float*)workspace, sums, p.C, p.S);
  return check_launch("dense_finalize_kernel");
}

// the checks the two GEMM entries share
static int dn_pw_check(const char* what, const void* x, size_t xs, const float* coef, const void* other, int B, int K, int M, int HW,
                       int dtype) {
  if (!x || !coef || !other || B < 1 || K < 8 || M < 8 || HW < 1 || !dn_dtype(dtype)) {
    set_error("%s: bad argument (16-bit tensors, K and M at least 8)", what);
    return SSDK_E_BADARG;
  }
  if (((((uintptr_t)x) | ((uintptr_t)other)) & 1) || (((uintptr_t)coef) & 15)) {
    set_error("%s: misaligned tensor or coef", what);
    return SSDK_E_BADARG;
  }
  if (xs < (size_t)K * (size_t)HW) {
    set_error("%s: the image stride is smaller than the slice", what);
    return SSDK_E_BADARG;
  }
  if (!dn_fits(B, K, HW, xs) || (size_t)B * (size_t)M * (size_t)HW >= DN_LIMIT || (size_t)M * (size_t)(K + 8) >= ((size_t)1 << 31)) {
    set_error("%s: tensor too large", what);
    return SSDK_E_BADARG;
  }
  return SSDK_OK;
}

extern "C" int ssdk_dense_train_pw_forward(const void* x, size_t x_image_stride, const float* coef, const void* a, int lda, void* m,
                                           float* sums, void* workspace, size_t workspace_bytes, int B, int K, int M, int HW, int dtype,
                                           void* stream) {
  int rc = dn_pw_check("ssdk_dense_train_pw_forward", x, x_image_stride, coef, m, B, K, M, HW, dtype);
  if (rc) return rc;
  if (!a || lda < K || (lda % 8) || (((uintptr_t)a) & 15)) {
    set_error("ssdk_dense_train_pw_forward: the matrix needs lda >= K, lda a multiple of 8 and 16-byte alignment");
    return SSDK_E_BADARG;
  }
  hipStream_t st = (hipStream_t)stream;
  const size_t ms = (size_t)M * (size_t)HW;
  if (!sums)
    return pw_gemm_launch<true, true>(x, a, nullptr, m, B, K, M, HW, dtype, st, nullptr, nullptr, x_image_stride, ms, (unsigned)lda, coef);
  if (!workspace || (((uintptr_t)workspace) & 15) || (((uintptr_t)sums) & 3)) {
    set_error("ssdk_dense_train_pw_forward: sums need a 16-byte aligned workspace");
    return SSDK_E_BADARG;
  }
  PwtParams pp;
  const PwtPlan pl = pw_gemm_plan(pp, B, K, M, HW, true);
  const size_t prow = (size_t)pl.gx * 4;
  if (workspace_bytes < (prow + (prow + 63) / 64) * (size_t)M * 2 * sizeof(float)) {
    set_error("ssdk_dense_train_pw_forward: workspace too small");
    return SSDK_E_WORKSPACE;
  }
  unsigned rows = 0;
  rc = pw_gemm_launch<true, true>(x, a, nullptr, m, B, K, M, HW, dtype, st, (float*)workspace, &rows, x_image_stride, ms, (unsigned)lda,
                                  coef);
  if (rc) return rc;
  const u32 n = (u32)M * 2u;
  return reduce_rows_fixed_order((const float*)workspace, (float*)workspace + (size_t)rows * n, sums, n, rows, st);
}

extern "C" int ssdk_dense_train_pw_wgrad(const void* dm, const void* x, size_t x_image_stride, const float* coef, float* dw,
                                         void* workspace, size_t workspace_bytes, int B, int M, int K, int HW, int dtype, void* stream) {
  int rc = dn_pw_check("ssdk_dense_train_pw_wgrad", x, x_image_stride, coef, dm, B, K, M, HW, dtype);
  if (rc) return rc;
  if (!dw || !workspace || ((((uintptr_t)dw) | ((uintptr_t)workspace)) & 3)) {
    set_error("ssdk_dense_train_pw_wgrad: bad argument (null or misaligned dw / workspace)");
    return SSDK_E_BADARG;
  }
  return pw_wgrad_run<true>(dm, x, x_image_stride, dw, workspace, workspace_bytes, B, M, K, HW, dtype, (hipStream_t)stream,
                            "ssdk_dense_train_pw_wgrad", coef);
}

// the checks the two bn1 entries share
static int dn_bn1_check(const char* what, const void* s, const void* x, size_t xs, const float* coef, const float* mean,
                        const float* invstd, const void* out, int N, int K, int HW, int dtype) {
  if (!s || !x || !coef || !mean || !invstd || !out || N < 1 || K < 1 || HW < 1 || !dn_dtype(dtype) ||
      ((((uintptr_t)s) | ((uintptr_t)x)) & 1) || ((((uintptr_t)coef) | ((uintptr_t)mean) | ((uintptr_t)invstd)) & 3) ||
      (size_t)K >= ((size_t)1 << 16)) {
    set_error("%s: bad argument (16-bit tensors)", what);
    return SSDK_E_BADARG;
  }
  if (xs < (size_t)K * (size_t)HW) {
    set_error("%s: the image stride is smaller than the slice", what);
    return SSDK_E_BADARG;
  }
  if (!dn_fits(N, K, HW, xs)) {
    set_error("%s: tensor too large", what);
    return SSDK_E_BADARG;
  }
  return SSDK_OK;
}

extern "C" int ssdk_dense_train_bn1_reduce(const void* s, const void* x, size_t x_image_stride, const float* coef, const float* save_mean,
                                           const float* save_invstd, float* red, void* workspace, size_t workspace_bytes, int N, int K,
                                           int HW, int dtype, void* stream) {
  int rc = dn_bn1_check("ssdk_dense_train_bn1_reduce", s, x, x_image_stride, coef, save_mean, save_invstd, red, N, K, HW, dtype);
  if (rc) return rc;
  if (!workspace || (((uintptr_t)workspace) & 15) || (((uintptr_t)red) & 3)) {
    set_error("ssdk_dense_train_bn1_reduce: bad argument (a 16-byte aligned workspace)");
    return SSDK_E_BADARG;
  }
  if (workspace_bytes < dn_red_bytes(N, K)) {
    set_error("ssdk_dense_train_bn1_reduce: workspace too small");
    return SSDK_E_WORKSPACE;
  }
  DenseRedParams p = {};
  p.t = (const u16*)s;
  p.x = (const u16*)x;
  p.xs = x_image_stride;
  p.coef = coef;
  p.mean = save_mean;
  p.invstd = save_invstd;
  p.partial = (float*)workspace;
  p.N = (u32)N;
  p.C = (u32)K;
  p.HW = (u32)HW;
  p.S = dense_split(N, K);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)K, p.S);
  if (dtype == SSDK_BF16) hipLaunchKernelGGL((dense_reduce_kernel<SSDK_BF16, 1>), grid, dim3(256), 0, st, p);
  else hipLaunchKernelGGL((dense_reduce_kernel<SSDK_F16, 1>), grid, dim3(256), 0, st, p);
  rc = check_launch("dense_reduce_kernel (bn1)");
  if (rc) return rc;
  hipLaunchKernelGGL(dense_finalize_kernel, dim3(((unsigned)K + 63u) / 64u), dim3(64), 0, st, (const float*)workspace, red, p.C, p.S);
  return check_launch("dense_finalize_kernel");
}

extern "C" int ssdk_dense_train_bn1_apply(const void* s, const void* x, size_t x_image_stride, const float* coef, const float* save_mean,
                                          const float* save_invstd, const float* weight, const float* red, void* g, size_t g_image_stride,
                                          int N, int K, int HW, int dtype, void* stream) {
  int rc = dn_bn1_check("ssdk_dense_train_bn1_apply", s, x, x_image_stride, coef, save_mean, save_invstd, g, N, K, HW, dtype);
  if (rc) return rc;
  if (!weight || !red || ((((uintptr_t)weight) | ((uintptr_t)red)) & 3) || (((uintptr_t)g) & 1)) {
    set_error("ssdk_dense_train_bn1_apply: bad argument (null or misaligned weight / red / g)");
    return SSDK_E_BADARG;
  }
  if (g_image_stride < (size_t)K * (size_t)HW) {
    set_error("ssdk_dense_train_bn1_apply: the image stride is smaller than the slice");
    return SSDK_E_BADARG;
  }
  if (!dn_fits(N, K, HW, g_image_stride)) {
    set_error("ssdk_dense_train_bn1_apply: tensor too large");
    return SSDK_E_BADARG;
  }
  DenseRedParams p = {};
  p.t = (const u16*)s;
  p.x = (const u16*)x;
  p.xs = x_image_stride;
  p.y = (u16*)g;
  p.ys = g_image_stride;
  p.coef = coef;
  p.mean = save_mean;
  p.invstd = save_invstd;
  p.weight = weight;
  p.red = red;
  p.N = (u32)N;
  p.C = (u32)K;
  p.HW = (u32)HW;
  const size_t total = (size_t)N * (size_t)K * (size_t)((HW + 7) / 8);
  const size_t wgs = (total + 255) / 256;
  const unsigned grid = (unsigned)(wgs < 8192 ? wgs : 8192);  // (32 workgroups per CU: a grid-stride pass)
  if (dtype == SSDK_BF16) hipLaunchKernelGGL((dense_bn1_apply_kernel<SSDK_BF16>), dim3(grid), dim3(256), 0, (hipStream_t)stream, p);
  else hipLaunchKernelGGL((dense_bn1_apply_kernel<SSDK_F16>), dim3(grid), dim3(256), 0, (hipStream_t)stream, p);
  return check_launch("dense_bn1_apply_kernel");
}
