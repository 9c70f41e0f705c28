// ssdk_cattrain.hip -- the two YOLO-only operations of the TRAINING step on gfx950, forward and backward, on the 16-bit NCHW tensors
// the step keeps (include/ssdk_cattrain.h):
//     cat    y = a || R(b) along the channels, R = SAME | UP2 (nearest x2); the upsampled tensor is never written
//     spp    y = x || maxpool5(x) || maxpool9(x) || maxpool13(x), stride 1, the padding never wins
// Every forward output carries the bits of an input element.  The backward passes write every gradient element exactly once, add in
// fp32 in a fixed order and round once: no atomics, no workspace, bit-reproducible.
//
// cat: a work item is 8 output columns of one output row (forward) or of one row pair (backward: the pair holds the complete 2x2
// blocks an UP2 source sums, ((g00 + g01) + g10) + g11, the rule of ssdk_neck_fuse_bwd).  Eight columns are one 16-byte access when
// the row segment is 16-byte aligned, four 4-byte accesses when it is 4-byte aligned and 2-byte accesses otherwise.
//
// spp: one workgroup per (n, c) plane, staged ONCE in LDS (H, W <= SSDK_SPP_TRAIN_MAX_SIDE).  Per window size the separable form:
// a row pass (maximum of the clipped row segment, and in the backward its first column), then a column pass over the row results.
// The backward recomputes the arg-max of every window from x -- torch's rule: the first maximum in row-major order of the clipped
// window under NUMERIC comparison (-0 == +0), a NaN is a maximum -- as the first row that reaches the overall maximum and the first
// column of that row's maximum, keeps it as a 16-bit plane index in LDS, and then GATHERS: pixel p adds gy_k[q] over the window
// positions q in row-major order whose arg-max is p, for k = 5, 9, 13 in that order, on top of gy_0[p].  LDS per workgroup:
// forward 4 HW bytes, backward 9 HW bytes (2 x, 1 first column, 2 arg-max, 4 fp32 sum): 36 KiB at 64 x 64, 2.25 KiB at 16 x 16.
#include "ssdk_conv_common.h"

#include "../../include/ssdk_cattrain.h"

namespace ssdk {

constexpr int kCatThreads = 256;
constexpr int kSppSide = SSDK_SPP_TRAIN_MAX_SIDE;

// ---- 8 / 4 consecutive 16-bit elements as raw bits, nv of them valid (nv <= 0: nothing is touched; invalid ones read as 0) ----
__device__ __forceinline__ void ldraw8(const u16* p, int nv, u16 (&v)[8]) {
  if (nv >= 8 && ((uintptr_t)p & 15u) == 0) {
    const u32x4 q = *reinterpret_cast<const u32x4*>(p);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      v[2 * e] = (u16)(q[e] & 0xffffu);
      v[2 * e + 1] = (u16)(q[e] >> 16);
    }
  } else if (nv >= 8 && ((uintptr_t)p & 3u) == 0) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const u32 w = reinterpret_cast<const u32*>(p)[e];
      v[2 * e] = (u16)(w & 0xffffu);
      v[2 * e + 1] = (u16)(w >> 16);
    }
  } else {
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = e < nv ? p[e] : (u16)0;
  }
}

__device__ __forceinline__ void straw8(u16* p, int nv, const u16 (&v)[8]) {
  if (nv >= 8 && ((uintptr_t)p & 15u) == 0) {
    u32x4 q;
#pragma unroll
    for (int e = 0; e < 4; ++e) q[e] = (u32)v[2 * e] | ((u32)v[2 * e + 1] << 16);
    *reinterpret_cast<u32x4*>(p) = q;
  } else if (nv >= 8 && ((uintptr_t)p & 3u) == 0) {
#pragma unroll
    for (int e = 0; e < 4; ++e) reinterpret_cast<u32*>(p)[e] = (u32)v[2 * e] | ((u32)v[2 * e + 1] << 16);
  } else {
#pragma unroll
    for (int e = 0; e < 8; ++e)
      if (e < nv) p[e] = v[e];
  }
}

__device__ __forceinline__ void ldraw4(const u16* p, int nv, u16 (&v)[4]) {
  if (nv >= 4 && ((uintptr_t)p & 3u) == 0) {
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const u32 w = reinterpret_cast<const u32*>(p)[e];
      v[2 * e] = (u16)(w & 0xffffu);
      v[2 * e + 1] = (u16)(w >> 16);
    }
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = e < nv ? p[e] : (u16)0;
  }
}

__device__ __forceinline__ void straw4(u16* p, int nv, const u16 (&v)[4]) {
  if (nv >= 4 && ((uintptr_t)p & 3u) == 0) {
#pragma unroll
    for (int e = 0; e < 2; ++e) reinterpret_cast<u32*>(p)[e] = (u32)v[2 * e] | ((u32)v[2 * e + 1] << 16);
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (e < nv) p[e] = v[e];
  }
}

struct CatTrainParams {
  const u16* a;
  const u16* b;
  const u16* gy;
  u16* y;
  u16* ga;
  u16* gb;
  int N, C1, C2, H, W, mode;
  int R, S;    // rows (forward) or row pairs (backward) of a plane, ceil(W / 8) column segments
  long items;  // N * (C1 + C2) * R * S
};

// item t -> image n, output channel co, row (pair) r, first column x0
__device__ __forceinline__ void cat_item(const CatTrainParams& q, long t, int& n, int& co, int& r, int& x0) {
  x0 = (int)(t % q.S) * 8;
  t /= q.S;
  r = (int)(t % q.R);
  t /= q.R;
  co = (int)(t % (q.C1 + q.C2));
  n = (int)(t / (q.C1 + q.C2));
}

__global__ __launch_bounds__(kCatThreads) void cat_train_fwd_kernel(const CatTrainParams q) {
  const long t = (long)blockIdx.x * kCatThreads + threadIdx.x;
  if (t >= q.items) return;
  int n, co, y, x0;
  cat_item(q, t, n, co, y, x0);
  const int nv = min(8, q.W - x0);
  u16 v[8];
  if (co < q.C1) {
    ldraw8(q.a + (((long)n * q.C1 + co) * q.H + y) * q.W + x0, nv, v);
  } else if (q.mode == SSDK_FUSE_SAME) {
    ldraw8(q.b + (((long)n * q.C2 + (co - q.C1)) * q.H + y) * q.W + x0, nv, v);
  } else {  // UP2: H, W even, so nv is even
    u16 s[4];
    ldraw4(q.b + (((long)n * q.C2 + (co - q.C1)) * (q.H >> 1) + (y >> 1)) * (q.W >> 1) + (x0 >> 1), nv >> 1, s);
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = s[e >> 1];
  }
  straw8(q.y + (((long)n * (q.C1 + q.C2) + co) * q.H + y) * q.W + x0, nv, v);
}

template <int DT>
__global__ __launch_bounds__(kCatThreads) void cat_train_bwd_kernel(const CatTrainParams q) {
  const long t = (long)blockIdx.x * kCatThreads + threadIdx.x;
  if (t >= q.items) return;
  int n, co, yy, x0;
  cat_item(q, t, n, co, yy, x0);
  const bool first = co < q.C1;
  if (first ? q.ga == nullptr : q.gb == nullptr) return;
  const int nv = min(8, q.W - x0);
  const u16* g = q.gy + (((long)n * (q.C1 + q.C2) + co) * q.H + 2 * yy) * q.W + x0;
  if (first || q.mode == SSDK_FUSE_SAME) {
    u16* o = first ? q.ga + (((long)n * q.C1 + co) * q.H + 2 * yy) * q.W + x0
                   : q.gb + (((long)n * q.C2 + (co - q.C1)) * q.H + 2 * yy) * q.W + x0;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      if (2 * yy + r >= q.H) break;
      u16 v[8];
      ldraw8(g + (long)r * q.W, nv, v);
      straw8(o + (long)r * q.W, nv, v);
    }
    return;
  }
  // UP2: H, W even -> both rows exist and nv is even
  u16 r0[8], r1[8], o[4];
  ldraw8(g, nv, r0);
  ldraw8(g + q.W, nv, r1);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float s = ((bits16_to_f32<DT>((u32)r0[2 * j]) + bits16_to_f32<DT>((u32)r0[2 * j + 1])) + bits16_to_f32<DT>((u32)r1[2 * j])) +
                    bits16_to_f32<DT>((u32)r1[2 * j + 1]);
    o[j] = (u16)f32_to_bits16<DT>(s);
  }
  straw4(q.gb + (((long)n * q.C2 + (co - q.C1)) * (q.H >> 1) + yy) * (q.W >> 1) + (x0 >> 1), nv >> 1, o);
}

// ---- SPP ---------------------------------------------------------------------------------------------------------------------------
struct SppTrainParams {
  const u16* x;
  const u16* gy;
  u16* y;
  u16* gx;
  int C, H, W;
};

// a later element replaces the running maximum when it is greater or a NaN (a NaN maximum is never replaced by a number)
__device__ __forceinline__ bool spp_takes(float u, float m) { return u > m || u != u; }

// forward: LDS  xs [HW] u16 | rm [HW] u16 (row maxima of the current window size)
template <int DT>
__global__ __launch_bounds__(kCatThreads) void spp_train_fwd_kernel(const SppTrainParams q) {
  extern __shared__ u16 spp_lds[];
  const int H = q.H, W = q.W, HW = H * W;
  u16* xs = spp_lds;
  u16* rm = spp_lds + HW;
  const long plane = blockIdx.x;  // n * C + c
  const long n = plane / q.C, c = plane % q.C;
  const u16* x = q.x + plane * HW;
  u16* y0 = q.y + (n * 4 * q.C + c) * HW;
  for (int i = threadIdx.x; i < HW; i += kCatThreads) {
    const u16 v = x[i];
    xs[i] = v;
    y0[i] = v;
  }
  __syncthreads();
#pragma unroll 1
  for (int ki = 1; ki <= 3; ++ki) {
    const int h = 2 * ki;  // half window: 2, 4, 6
    for (int i = threadIdx.x; i < HW; i += kCatThreads) {
      const int r = i / W, cx = i - r * W;
      const int lo = max(cx - h, 0), hi = min(cx + h, W - 1);
      u16 mb = xs[r * W + lo];
      float m = bits16_to_f32<DT>((u32)mb);
      for (int j = lo + 1; j <= hi; ++j) {
        const u16 ub = xs[r * W + j];
        const float u = bits16_to_f32<DT>((u32)ub);
        if (spp_takes(u, m)) {
          m = u;
          mb = ub;
        }
      }
      rm[i] = mb;
    }
    __syncthreads();
    u16* yk = y0 + (long)ki * q.C * HW;
    for (int i = threadIdx.x; i < HW; i += kCatThreads) {
      const int r = i / W, cx = i - r * W;
      const int lo = max(r - h, 0), hi = min(r + h, H - 1);
      u16 mb = rm[lo * W + cx];
      float m = bits16_to_f32<DT>((u32)mb);
      for (int j = lo + 1; j <= hi; ++j) {
        const u16 ub = rm[j * W + cx];
        const float u = bits16_to_f32<DT>((u32)ub);
        if (spp_takes(u, m)) {
          m = u;
          mb = ub;
        }
      }
      yk[i] = mb;
    }
    __syncthreads();  // rm is rewritten by the next window size
  }
}

// backward: LDS  acc [HW] fp32 | xs [HW] u16 | arg [HW] u16 | fc [HW] u8 (first column of the row maximum)
template <int DT>
__global__ __launch_bounds__(kCatThreads) void spp_train_bwd_kernel(const SppTrainParams q) {
  extern __shared__ float spp_acc[];
  const int H = q.H, W = q.W, HW = H * W;
  float* acc = spp_acc;
  u16* xs = reinterpret_cast<u16*>(spp_acc + HW);
  u16* arg = xs + HW;
  unsigned char* fc = reinterpret_cast<unsigned char*>(arg + HW);
  const long plane = blockIdx.x;
  const long n = plane / q.C, c = plane % q.C;
  const u16* x = q.x + plane * HW;
  const u16* g0 = q.gy + (n * 4 * q.C + c) * HW;
  for (int i = threadIdx.x; i < HW; i += kCatThreads) {
    xs[i] = x[i];
    acc[i] = bits16_to_f32<DT>((u32)g0[i]);  // (only this thread touches acc[i])
  }
  __syncthreads();
#pragma unroll 1
  for (int ki = 1; ki <= 3; ++ki) {
    const int h = 2 * ki;
    // row pass: first column of the maximum of row r over columns [cx - h, cx + h] clipped
    for (int i = threadIdx.x; i < HW; i += kCatThreads) {
      const int r = i / W, cx = i - r * W;
      const int lo = max(cx - h, 0), hi = min(cx + h, W - 1);
      float m = bits16_to_f32<DT>((u32)xs[r * W + lo]);
      int best = lo;
      for (int j = lo + 1; j <= hi; ++j) {
        const float u = bits16_to_f32<DT>((u32)xs[r * W + j]);
        if (spp_takes(u, m)) {
          m = u;
          best = j;
        }
      }
      fc[i] = (unsigned char)best;
    }
    __syncthreads();
    // column pass: the first row whose maximum is the window's -> plane index of the arg-max of window i
    for (int i = threadIdx.x; i < HW; i += kCatThreads) {
      const int r = i / W, cx = i - r * W;
      const int lo = max(r - h, 0), hi = min(r + h, H - 1);
      int best = lo * W + fc[lo * W + cx];
      float m = bits16_to_f32<DT>((u32)xs[best]);
      for (int j = lo + 1; j <= hi; ++j) {
        const int cand = j * W + fc[j * W + cx];
        const float u = bits16_to_f32<DT>((u32)xs[cand]);
        if (spp_takes(u, m)) {
          m = u;
          best = cand;
        }
      }
      arg[i] = (u16)best;
    }
    __syncthreads();
    // gather: the windows that can reach pixel i are those centred within h of it, in row-major order
    const u16* gk = g0 + (long)ki * q.C * HW;
    for (int i = threadIdx.x; i < HW; i += kCatThreads) {
      const int r = i / W, cx = i - r * W;
      const int r0 = max(r - h, 0), r1 = min(r + h, H - 1), c0 = max(cx - h, 0), c1 = min(cx + h, W - 1);
      float s = acc[i];
      for (int qr = r0; qr <= r1; ++qr)
        for (int qc = c0; qc <= c1; ++qc) {
          const int qi = qr * W + qc;
          if ((int)arg[qi] == i) s += bits16_to_f32<DT>((u32)gk[qi]);
        }
      acc[i] = s;
    }
    __syncthreads();  // fc and arg are rewritten by the next window size
  }
  u16* gx = q.gx + plane * HW;
  for (int i = threadIdx.x; i < HW; i += kCatThreads) gx[i] = (u16)f32_to_bits16<DT>(acc[i]);
}

static int cat_train_check(const char* who, int N, int C1, int C2, int H, int W, int mode, int dtype, CatTrainParams* q) {
  if (dtype != SSDK_BF16 && dtype != SSDK_F16) {
    set_error("%s: dtype must be bf16 or f16", who);
    return SSDK_E_BADARG;
  }
  if (N < 1 || C1 < 1 || C2 < 1 || H < 1 || W < 1 || (long)C1 + C2 >= (1L << 31) || (long)N * ((long)C1 + C2) >= (1L << 31) ||
      (long)N * ((long)C1 + C2) * H >= (1L << 31) || (long)N * ((long)C1 + C2) * H * W >= (1L << 31)) {
    set_error("%s: bad geometry N=%d C1=%d C2=%d H=%d W=%d (each >= 1, below 2^31 elements)", who, N, C1, C2, H, W);
    return SSDK_E_BADARG;
  }
  if (mode != SSDK_FUSE_SAME && mode != SSDK_FUSE_UP2) {
    set_error("%s: mode %d is neither SSDK_FUSE_SAME nor SSDK_FUSE_UP2", who, mode);
    return SSDK_E_BADARG;
  }
  if (mode == SSDK_FUSE_UP2 && ((H | W) & 1)) {
    set_error("%s: an upsampled source needs even output dims (%dx%d)", who, H, W);
    return SSDK_E_BADARG;
  }
  memset(q, 0, sizeof(*q));
  q->N = N;
  q->C1 = C1;
  q->C2 = C2;
  q->H = H;
  q->W = W;
  q->mode = mode;
  q->S = (W + 7) / 8;
  return SSDK_OK;
}

static int spp_train_check(const char* who, const void* p0, const void* p1, const void* p2, int N, int C, int H, int W, int dtype) {
  if (dtype != SSDK_BF16 && dtype != SSDK_F16) {
    set_error("%s: dtype must be bf16 or f16", who);
    return SSDK_E_BADARG;
  }
  if (N < 1 || C < 1 || H < 1 || W < 1 || (long)N * C >= (1L << 29) || (long)N * C * H >= (1L << 29) || (long)N * C * H * W >= (1L << 29)) {
    set_error("%s: bad geometry N=%d C=%d H=%d W=%d (each >= 1, the 4 C channel output below 2^31 elements)", who, N, C, H, W);
    return SSDK_E_BADARG;
  }
  if (H > kSppSide || W > kSppSide) {
    set_error("%s: a %dx%d plane does not fit the LDS staging (H, W <= SSDK_SPP_TRAIN_MAX_SIDE = %d)", who, H, W, kSppSide);
    return SSDK_E_BADARG;
  }
  if (!p0 || !p1 || !p2 || (((uintptr_t)p0 | (uintptr_t)p1 | (uintptr_t)p2) & 1u)) {
    set_error("%s: null or misaligned pointer", who);
    return SSDK_E_BADARG;
  }
  return SSDK_OK;
}

}  // namespace ssdk

using namespace ssdk;

extern "C" int ssdk_cat_train_fwd(const void* a, const void* b, void* y, int N, int C1, int C2, int H, int W, int mode, int dtype,
                                  void* stream) {
  CatTrainParams q;
  if (int rc = cat_train_check("cat_train_fwd", N, C1, C2, H, W, mode, dtype, &q)) return rc;
  if (!a || !b || !y || (((uintptr_t)a | (uintptr_t)b | (uintptr_t)y) & 1u)) {
    set_error("cat_train_fwd: null or misaligned pointer (a, b and y are mandatory)");
    return SSDK_E_BADARG;
  }
  q.a = (const u16*)a;
  q.b = (const u16*)b;
  q.y = (u16*)y;
  q.R = H;
  q.items = (long)N * (C1 + C2) * q.R * q.S;
  const dim3 grid((unsigned)((q.items + kCatThreads - 1) / kCatThreads));
  hipLaunchKernelGGL(cat_train_fwd_kernel, grid, dim3(kCatThreads), 0, (hipStream_t)stream, q);
  return check_launch("cat_train_fwd_kernel");
}

extern "C" int ssdk_cat_train_bwd(const void* gy, void* ga, void* gb, int N, int C1, int C2, int H, int W, int mode, int dtype,
                                  void* stream) {
  CatTrainParams q;
  if (int rc = cat_train_check("cat_train_bwd", N, C1, C2, H, W, mode, dtype, &q)) return rc;
  if (!gy || (((uintptr_t)gy | (uintptr_t)ga | (uintptr_t)gb) & 1u)) {
    set_error("cat_train_bwd: null gy or a misaligned pointer (ga and gb may each be NULL)");
    return SSDK_E_BADARG;
  }
  if (!ga && !gb) return SSDK_OK;
  q.gy = (const u16*)gy;
  q.ga = (u16*)ga;
  q.gb = (u16*)gb;
  q.R = (H + 1) / 2;
  q.items = (long)N * (C1 + C2) * q.R * q.S;
  const dim3 grid((unsigned)((q.items + kCatThreads - 1) / kCatThreads));
  if (dtype == SSDK_BF16) hipLaunchKernelGGL((cat_train_bwd_kernel<SSDK_BF16>), grid, dim3(kCatThreads), 0, (hipStream_t)stream, q);
  else hipLaunchKernelGGL((cat_train_bwd_kernel<SSDK_F16>), grid, dim3(kCatThreads), 0, (hipStream_t)stream, q);
  return check_launch("cat_train_bwd_kernel");
}

extern "C" int ssdk_spp_train_fwd(const void* x, void* y, int N, int C, int H, int W, int dtype, void* stream) {
  if (int rc = spp_train_check("spp_train_fwd", x, y, y, N, C, H, W, dtype)) return rc;
  SppTrainParams q;
  memset(&q, 0, sizeof(q));
  q.x = (const u16*)x;
  q.y = (u16*)y;
  q.C = C;
  q.H = H;
  q.W = W;
  const size_t lds = (size_t)H * W * 4;
  const dim3 grid((unsigned)(N * C));
  if (dtype == SSDK_BF16) hipLaunchKernelGGL((spp_train_fwd_kernel<SSDK_BF16>), grid, dim3(kCatThreads), lds, (hipStream_t)stream, q);
  else hipLaunchKernelGGL((spp_train_fwd_kernel<SSDK_F16>), grid, dim3(kCatThreads), lds, (hipStream_t)stream, q);
  return check_launch("spp_train_fwd_kernel");
}

extern "C" int ssdk_spp_train_bwd(const void* x, const void* gy, void* gx, int N, int C, int H, int W, int dtype, void* stream) {
  if (int rc = spp_train_check("spp_train_bwd", x, gy, gx, N, C, H, W, dtype)) return rc;
  SppTrainParams q;
  memset(&q, 0, sizeof(q));
  q.x = (const u16*)x;
  q.gy = (const u16*)gy;
  q.gx = (u16*)gx;
  q.C = C;
  q.H = H;
  q.W = W;
  const size_t lds = (size_t)H * W * 9;
  const dim3 grid((unsigned)(N * C));
  if (dtype == SSDK_BF16) hipLaunchKernelGGL((spp_train_bwd_kernel<SSDK_BF16>), grid, dim3(kCatThreads), lds, (hipStream_t)stream, q);
  else hipLaunchKernelGGL((spp_train_bwd_kernel<SSDK_F16>), grid, dim3(kCatThreads), lds, (hipStream_t)stream, q);
  return check_launch("spp_train_bwd_kernel");
}
