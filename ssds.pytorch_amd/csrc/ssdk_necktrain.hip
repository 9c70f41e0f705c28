// ssdk_necktrain.hip -- the memory-bound neck operations of the FPN / BiFPN TRAINING step on gfx950, forward and backward, on the
// 16-bit NCHW tensors the step keeps:
//     fusion     y = w0 a + w1 R_b(b) [+ w2 R_c(c)],  R = SAME | UP2 (nearest x2) | POOL2 (max_pool2d(kernel 2), floor mode)
//                (BiFPNModule's weighted fusions; with a NULL weight pointer the FPN top-down upsample-add)
//     max-pool   3x3 / stride 2 / pad 1 (the ResNet stem's)
// The fusion weights are read from DEVICE memory (fp32 pointer + element stride: a column of the fast-normalised [K, L] tensor),
// so nothing synchronises with the host.  fp32 arithmetic, one rounding per output element.  The backward passes recompute the
// arg-max of every pooling window from the saved source (first maximum in row-major window order, a NaN is a maximum: torch's
// rule); no index tensor exists.
//
// Work item of the fusion kernels: 2 output rows x 8 output columns of one (n, c) plane.  The two rows share the UP2 source row
// and hold the complete 2x2 block whose gradients an UP2 source sums; under POOL2 the item owns the 4 x 16 source elements below
// it (+ the odd row / column floor mode drops, which get zeros), so every gradient element is written exactly once.  Eight
// columns are one 16-byte access when the row segment is 16-byte aligned, four 4-byte accesses when it is 4-byte aligned and
// scalar 2-byte accesses otherwise (rows of odd W, the last partial segment).
//
// Weight gradient gw[k] = sum gy R_k(x_k): fixed order, no atomics.  An item adds its <= 16 products in order; a thread adds its
// items into an inner accumulator that is flushed into an outer one every 64 items; xor-shuffle tree over the wave; the four
// waves in order; one fp32 partial triple per workgroup into the caller's workspace; a second one-workgroup launch adds the
// partials (<= 16 per thread in index order, then the same trees) and writes the whole [K, L] gradient.  The longest chain of
// dependent additions a term passes through is 16 + 64 + 33 + 6 + 4 + 16 + 6 + 4 = 149 at the largest supported tensor
// (neckfuse.WSUM_DEPTH).
#include "ssdk_conv_common.h"

namespace ssdk {

constexpr int kNeckThreads = 256;
constexpr int kNeckMaxBlocks = 4096;  // partial triples of the weight gradient: <= 16 per thread of the final launch
constexpr int kNeckInner = 64;        // items per flush of a thread's inner accumulator

// ---- 8 / 4 consecutive 16-bit elements <-> fp32, nv of them valid (nv <= 0: nothing is touched) ----------------------------
template <int DT>
__device__ __forceinline__ void ld8(const u16* p, int nv, float (&v)[8], float fill) {
  if (nv >= 8 && ((uintptr_t)p & 15u) == 0) {
    const u32x4 q = *reinterpret_cast<const u32x4*>(p);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const u32 w = q[e];
      v[2 * e] = bits16_to_f32<DT>(w & 0xffffu);
      v[2 * e + 1] = bits16_to_f32<DT>(w >> 16);
    }
  } else if (nv >= 8 && ((uintptr_t)p & 3u) == 0) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const u32 w = reinterpret_cast<const u32*>(p)[e];
      v[2 * e] = bits16_to_f32<DT>(w & 0xffffu);
      v[2 * e + 1] = bits16_to_f32<DT>(w >> 16);
    }
  } else {
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = e < nv ? bits16_to_f32<DT>((u32)p[e]) : fill;
  }
}

template <int DT>
__device__ __forceinline__ void st8(u16* p, int nv, const float (&v)[8]) {
  if (nv >= 8 && ((uintptr_t)p & 15u) == 0) {
    u32x4 q;
#pragma unroll
    for (int e = 0; e < 4; ++e) q[e] = pack2_16<DT>(v[2 * e], v[2 * e + 1]);
    *reinterpret_cast<u32x4*>(p) = q;
  } else if (nv >= 8 && ((uintptr_t)p & 3u) == 0) {
#pragma unroll
    for (int e = 0; e < 4; ++e) reinterpret_cast<u32*>(p)[e] = pack2_16<DT>(v[2 * e], v[2 * e + 1]);
  } else {
#pragma unroll
    for (int e = 0; e < 8; ++e)
      if (e < nv) p[e] = (u16)f32_to_bits16<DT>(v[e]);
  }
}

template <int DT>
__device__ __forceinline__ void ld4(const u16* p, int nv, float (&v)[4]) {
  if (nv >= 4 && ((uintptr_t)p & 3u) == 0) {
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const u32 w = reinterpret_cast<const u32*>(p)[e];
      v[2 * e] = bits16_to_f32<DT>(w & 0xffffu);
      v[2 * e + 1] = bits16_to_f32<DT>(w >> 16);
    }
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = e < nv ? bits16_to_f32<DT>((u32)p[e]) : 0.f;
  }
}

template <int DT>
__device__ __forceinline__ void st4(u16* p, int nv, const float (&v)[4]) {
  if (nv >= 4 && ((uintptr_t)p & 3u) == 0) {
#pragma unroll
    for (int e = 0; e < 2; ++e) reinterpret_cast<u32*>(p)[e] = pack2_16<DT>(v[2 * e], v[2 * e + 1]);
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (e < nv) p[e] = (u16)f32_to_bits16<DT>(v[e]);
  }
}

// max of a 2x2 window in row-major order: a later element replaces the running maximum when it is greater or a NaN
__device__ __forceinline__ void win2(float v00, float v01, float v10, float v11, float& m, int& arg) {
  m = v00;
  arg = 0;
  if (v01 > m || v01 != v01) {
    m = v01;
    arg = 1;
  }
  if (v10 > m || v10 != v10) {
    m = v10;
    arg = 2;
  }
  if (v11 > m || v11 != v11) {
    m = v11;
    arg = 3;
  }
}

struct NeckParams {
  const u16* a;
  const u16* b;
  const u16* c;
  const u16* gy;
  u16* y;
  u16* ga;
  u16* gb;
  u16* gc;
  const float* w;  // device fp32 weights, element k at w[k * wstride]; NULL: every weight is 1
  float* part;     // [blocks][3] partial weight gradients (backward with gw)
  int wstride;
  int nsrc;  // 2 | 3
  int mode_b, mode_c;
  int hb, wb, hc, wc;  // source dims of b / c
  int P, H, W;         // P = N * C planes of H x W outputs
  int HT, S;           // ceil(H / 2) row pairs, ceil(W / 8) column segments
  long items;          // P * HT * S
};

// R(src) on the 8 output columns x0 .. x0 + 7 of output row y (nv valid; the others come back as 0); arg: POOL2 window arg-max
template <int DT>
__device__ __forceinline__ void neck_source_row(const u16* src, int mode, int hs, int ws, long p, int y, int x0, int nv, int H, int W,
                                                float (&v)[8], int (&arg)[8]) {
  if (mode == SSDK_FUSE_SAME) {
    ld8<DT>(src + (p * H + y) * W + x0, nv, v, 0.f);
  } else if (mode == SSDK_FUSE_UP2) {
    float s[4];
    ld4<DT>(src + (p * (H >> 1) + (y >> 1)) * (W >> 1) + (x0 >> 1), nv >> 1, s);
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = s[e >> 1];
  } else {
    float r0[16], r1[16];
    const u16* q = src + (p * hs + 2 * y) * ws + 2 * x0;
    float t[8];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      ld8<DT>(q + 8 * h, 2 * nv - 8 * h, t, 0.f);
#pragma unroll
      for (int e = 0; e < 8; ++e) r0[8 * h + e] = t[e];
      ld8<DT>(q + ws + 8 * h, 2 * nv - 8 * h, t, 0.f);
#pragma unroll
      for (int e = 0; e < 8; ++e) r1[8 * h + e] = t[e];
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) win2(r0[2 * e], r0[2 * e + 1], r1[2 * e], r1[2 * e + 1], v[e], arg[e]);
  }
}

__device__ __forceinline__ void neck_item(const NeckParams& q, long t, long& p, int& yy, int& x0) {
  x0 = (int)(t % q.S) * 8;
  const long r = t / q.S;
  yy = (int)(r % q.HT);
  p = r / q.HT;
}

template <int DT>
__global__ __launch_bounds__(kNeckThreads) void neck_fuse_fwd_kernel(const NeckParams q) {
  float w0 = 1.f, w1 = 1.f, w2 = 1.f;
  if (q.w) {
    w0 = q.w[0];
    w1 = q.w[q.wstride];
    if (q.nsrc == 3) w2 = q.w[2 * (long)q.wstride];
  }
  const long step = (long)gridDim.x * kNeckThreads;
  for (long t = (long)blockIdx.x * kNeckThreads + threadIdx.x; t < q.items; t += step) {
    long p;
    int yy, x0;
    neck_item(q, t, p, yy, x0);
    const int nv = min(8, q.W - x0);
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const int y = 2 * yy + r;
      if (y >= q.H) break;
      float v[8], acc[8];
      int arg[8];
      ld8<DT>(q.a + (p * q.H + y) * q.W + x0, nv, v, 0.f);
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] = w0 * v[e];
      neck_source_row<DT>(q.b, q.mode_b, q.hb, q.wb, p, y, x0, nv, q.H, q.W, v, arg);
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] += w1 * v[e];
      if (q.nsrc == 3) {
        neck_source_row<DT>(q.c, q.mode_c, q.hc, q.wc, p, y, x0, nv, q.H, q.W, v, arg);
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] += w2 * v[e];
      }
      st8<DT>(q.y + (p * q.H + y) * q.W + x0, nv, acc);
    }
  }
}

// gradient of one source over an item (g: gy of the two rows, zeros where invalid) -> its gradient tensor (gout, may be NULL) and
// the item's share of sum gy R(src) (when want_sum)
template <int DT>
__device__ __forceinline__ float neck_source_bwd(const u16* src, u16* gout, int mode, int hs, int ws, float w, bool want_sum, long p, int yy,
                                                 int x0, int nv, int H, int W, const float (&g)[2][8]) {
  float s = 0.f;
  if (mode == SSDK_FUSE_UP2) {  // H, W even: both rows exist, nv is even
    const long off = (p * (H >> 1) + yy) * (W >> 1) + (x0 >> 1);
    if (want_sum) {
      float sv[4];
      ld4<DT>(src + off, nv >> 1, sv);
#pragma unroll
      for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int e = 0; e < 8; ++e) s += g[r][e] * sv[e >> 1];
    }
    if (gout) {
      float o[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = w * (((g[0][2 * j] + g[0][2 * j + 1]) + g[1][2 * j]) + g[1][2 * j + 1]);
      st4<DT>(gout + off, nv >> 1, o);
    }
    return s;
  }
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const int y = 2 * yy + r;
    if (y >= H) break;
    float v[8];
    int arg[8];
    if (mode == SSDK_FUSE_SAME) {
      if (want_sum) {
        ld8<DT>(src + (p * H + y) * W + x0, nv, v, 0.f);
#pragma unroll
        for (int e = 0; e < 8; ++e) s += g[r][e] * v[e];
      }
      if (gout) {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = w * g[r][e];
        st8<DT>(gout + (p * H + y) * W + x0, nv, v);
      }
    } else {  // POOL2
      neck_source_row<DT>(src, mode, hs, ws, p, y, x0, nv, H, W, v, arg);
      if (want_sum) {
#pragma unroll
        for (int e = 0; e < 8; ++e) s += g[r][e] * v[e];
      }
      if (gout) {
        const bool last_seg = x0 + 8 >= W, odd_col = (ws & 1) != 0;
        u16* o = gout + (p * hs + 2 * y) * ws + 2 * x0;
        float z[8];
#pragma unroll
        for (int dy = 0; dy < 2; ++dy) {
#pragma unroll
          for (int h = 0; h < 2; ++h) {
#pragma unroll
            for (int e = 0; e < 8; ++e) z[e] = arg[4 * h + (e >> 1)] == 2 * dy + (e & 1) ? w * g[r][4 * h + (e >> 1)] : 0.f;
            st8<DT>(o + (long)dy * ws + 8 * h, 2 * nv - 8 * h, z);
          }
          if (last_seg && odd_col) o[(long)dy * ws + (ws - 1 - 2 * x0)] = 0;  // the column floor mode drops
        }
        if (y == H - 1 && (hs & 1)) {  // the row floor mode drops
#pragma unroll
          for (int e = 0; e < 8; ++e) z[e] = 0.f;
          st8<DT>(o + 2L * ws, 2 * nv, z);
          st8<DT>(o + 2L * ws + 8, 2 * nv - 8, z);
          if (last_seg && odd_col) o[2L * ws + (ws - 1 - 2 * x0)] = 0;
        }
      }
    }
  }
  return s;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
  return v;
}

// sums of the workgroup's per-thread triples, in thread 0: xor tree over each wave, then the four waves in order
__device__ __forceinline__ void block_sum3(float (&s)[3], float (*lds)[3]) {
#pragma unroll
  for (int k = 0; k < 3; ++k) s[k] = wave_sum(s[k]);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < 3; ++k) lds[wave][k] = s[k];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      float t = 0.f;
#pragma unroll
      for (int v = 0; v < kNeckThreads / 64; ++v) t += lds[v][k];
      s[k] = t;
    }
  }
}

template <int DT>
__global__ __launch_bounds__(kNeckThreads) void neck_fuse_bwd_kernel(const NeckParams q) {
  __shared__ float lds[kNeckThreads / 64][3];
  float w0 = 1.f, w1 = 1.f, w2 = 1.f;
  if (q.w) {
    w0 = q.w[0];
    w1 = q.w[q.wstride];
    if (q.nsrc == 3) w2 = q.w[2 * (long)q.wstride];
  }
  const bool want_sum = q.part != nullptr;
  float inner[3] = {0.f, 0.f, 0.f}, outer[3] = {0.f, 0.f, 0.f};
  int run = 0;
  const long step = (long)gridDim.x * kNeckThreads;
  for (long t = (long)blockIdx.x * kNeckThreads + threadIdx.x; t < q.items; t += step) {
    long p;
    int yy, x0;
    neck_item(q, t, p, yy, x0);
    const int nv = min(8, q.W - x0);
    float g[2][8];
#pragma unroll
    for (int r = 0; r < 2; ++r) ld8<DT>(q.gy + (p * q.H + 2 * yy + r) * q.W + x0, 2 * yy + r < q.H ? nv : 0, g[r], 0.f);
    float s[3] = {0.f, 0.f, 0.f};
    if (q.ga || want_sum) {
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        const int y = 2 * yy + r;
        if (y >= q.H) break;
        float v[8];
        if (want_sum) {
          ld8<DT>(q.a + (p * q.H + y) * q.W + x0, nv, v, 0.f);
#pragma unroll
          for (int e = 0; e < 8; ++e) s[0] += g[r][e] * v[e];
        }
        if (q.ga) {
#pragma unroll
          for (int e = 0; e < 8; ++e) v[e] = w0 * g[r][e];
          st8<DT>(q.ga + (p * q.H + y) * q.W + x0, nv, v);
        }
      }
    }
    if (q.gb || want_sum) s[1] = neck_source_bwd<DT>(q.b, q.gb, q.mode_b, q.hb, q.wb, w1, want_sum, p, yy, x0, nv, q.H, q.W, g);
    if (q.nsrc == 3 && (q.gc || want_sum))
      s[2] = neck_source_bwd<DT>(q.c, q.gc, q.mode_c, q.hc, q.wc, w2, want_sum, p, yy, x0, nv, q.H, q.W, g);
    if (want_sum) {
#pragma unroll
      for (int k = 0; k < 3; ++k) inner[k] += s[k];
      if (++run == kNeckInner) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          outer[k] += inner[k];
          inner[k] = 0.f;
        }
        run = 0;
      }
    }
  }
  if (want_sum) {  // (workgroup-uniform)
#pragma unroll
    for (int k = 0; k < 3; ++k) outer[k] += inner[k];
    block_sum3(outer, lds);
    if (threadIdx.x == 0) {
#pragma unroll
      for (int k = 0; k < 3; ++k) q.part[(long)blockIdx.x * 3 + k] = outer[k];
    }
  }
}

// one workgroup: partial triples -> gw [K][L], the sums in column `col`, zeros elsewhere
__global__ __launch_bounds__(kNeckThreads) void neck_fuse_gw_kernel(const float* part, int nparts, float* gw, int K, int L, int col) {
  __shared__ float lds[kNeckThreads / 64][3];
  __shared__ float total[3];
  const int chunk = (nparts + kNeckThreads - 1) / kNeckThreads;
  float s[3] = {0.f, 0.f, 0.f};
  for (int i = threadIdx.x * chunk; i < min(nparts, ((int)threadIdx.x + 1) * chunk); ++i) {
#pragma unroll
    for (int k = 0; k < 3; ++k) s[k] += part[(long)i * 3 + k];
  }
  block_sum3(s, lds);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < 3; ++k) total[k] = s[k];
  }
  __syncthreads();
  for (int i = threadIdx.x; i < K * L; i += kNeckThreads) gw[i] = (i % L) == col ? total[i / L] : 0.f;
}

// ---- max-pool 3x3 / stride 2 / pad 1 on NCHW planes ------------------------------------------------------------------------
struct PoolTrainParams {
  const u16* x;
  const u16* gy;
  u16* y;
  u16* gx;
  int P, H, W, Ho, Wo;
  int R, S;  // forward: Ho rows, ceil(Wo / 8) segments; backward: ceil(H / 2) row pairs, ceil(W / 8) segments
  long items;
};

// forward item: 8 outputs of one output row = input rows 2 oy - 1 .. 2 oy + 1, columns 2 ox0 - 1 .. 2 ox0 + 15
template <int DT>
__global__ __launch_bounds__(kNeckThreads) void maxpool_train_fwd_kernel(const PoolTrainParams q) {
  const float ninf = -__builtin_inff();
  const long step = (long)gridDim.x * kNeckThreads;
  for (long t = (long)blockIdx.x * kNeckThreads + threadIdx.x; t < q.items; t += step) {
    const int ox0 = (int)(t % q.S) * 8;
    const long r = t / q.S;
    const int oy = (int)(r % q.R);
    const long p = r / q.R;
    float m[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) m[e] = ninf;
#pragma unroll
    for (int dy = 0; dy < 3; ++dy) {
      const int iy = 2 * oy - 1 + dy;
      if (iy < 0 || iy >= q.H) continue;
      const u16* row = q.x + (p * q.H + iy) * q.W + 2 * ox0;
      float v[17], tmp[8];
      v[0] = ox0 > 0 ? bits16_to_f32<DT>((u32)row[-1]) : ninf;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        ld8<DT>(row + 8 * h, q.W - 2 * ox0 - 8 * h, tmp, ninf);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[1 + 8 * h + e] = tmp[e];
      }
#pragma unroll
      for (int e = 0; e < 8; ++e)
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
          const float u = v[2 * e + dx];
          m[e] = (u > m[e] || u != u) ? u : m[e];
        }
    }
    st8<DT>(q.y + (p * q.Ho + oy) * q.Wo + ox0, q.Wo - ox0, m);
  }
}

// backward item: gx rows 2k, 2k + 1 x columns c0 .. c0 + 7 gathered from the windows that can reach them: window rows k (input rows
// 2k - 1 .. 2k + 1) and k + 1 (2k + 1 .. 2k + 3), window columns c0 / 2 .. c0 / 2 + 4 (input columns c0 - 1 .. c0 + 9).  The
// arg-max of each is recomputed (first maximum over the window's in-range elements, a NaN is a maximum), and a pixel that wins
// several windows adds their gy in window order.
template <int DT>
__global__ __launch_bounds__(kNeckThreads) void maxpool_train_bwd_kernel(const PoolTrainParams q) {
  const float ninf = -__builtin_inff();
  const long step = (long)gridDim.x * kNeckThreads;
  for (long t = (long)blockIdx.x * kNeckThreads + threadIdx.x; t < q.items; t += step) {
    const int c0 = (int)(t % q.S) * 8;
    const long rr = t / q.S;
    const int k = (int)(rr % q.R);
    const long p = rr / q.R;
    const int j0 = c0 >> 1;
    float acc[2][8];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[r][e] = 0.f;
    bool cv[11];
#pragma unroll
    for (int i = 0; i < 11; ++i) cv[i] = c0 - 1 + i >= 0 && c0 - 1 + i < q.W;
#pragma unroll
    for (int wr = 0; wr < 2; ++wr) {
      const int oy = k + wr;
      if (oy >= q.Ho) break;
      float v[3][11];
      bool rv[3];
#pragma unroll
      for (int dy = 0; dy < 3; ++dy) {
        const int iy = 2 * oy - 1 + dy;
        rv[dy] = iy >= 0 && iy < q.H;
        const u16* row = q.x + (p * q.H + iy) * q.W + c0;  // (only dereferenced where rv && cv)
        float tmp[8];
        ld8<DT>(row, rv[dy] ? q.W - c0 : 0, tmp, ninf);
        v[dy][0] = (rv[dy] && cv[0]) ? bits16_to_f32<DT>((u32)row[-1]) : ninf;
#pragma unroll
        for (int e = 0; e < 8; ++e) v[dy][1 + e] = tmp[e];
        v[dy][9] = (rv[dy] && cv[9]) ? bits16_to_f32<DT>((u32)row[8]) : ninf;
        v[dy][10] = (rv[dy] && cv[10]) ? bits16_to_f32<DT>((u32)row[9]) : ninf;
      }
#pragma unroll
      for (int j = 0; j < 5; ++j) {
        const int ox = j0 + j;
        if (ox >= q.Wo) break;
        const float g = bits16_to_f32<DT>((u32)q.gy[(p * q.Ho + oy) * q.Wo + ox]);
        float m = ninf;
        int arg = -1;
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
          for (int dx = 0; dx < 3; ++dx) {
            const float u = v[dy][2 * j + dx];
            if (rv[dy] && cv[2 * j + dx] && (arg < 0 || u > m || u != u)) {
              m = u;
              arg = 3 * dy + dx;
            }
          }
        // window row wr = 0 reaches tile rows 0 (dy 1) and 1 (dy 2); wr = 1 reaches tile row 1 (dy 0); tile column 2j + dx - 1
#pragma unroll
        for (int dy = 0; dy < 3; ++dy) {
          const int tr = wr == 0 ? dy - 1 : (dy == 0 ? 1 : -1);
          if (tr < 0) continue;
#pragma unroll
          for (int dx = 0; dx < 3; ++dx) {
            const int tc = 2 * j + dx - 1;
            if (tc < 0 || tc > 7) continue;
            acc[tr][tc] += arg == 3 * dy + dx ? g : 0.f;
          }
        }
      }
    }
#pragma unroll
    for (int r = 0; r < 2; ++r)
      if (2 * k + r < q.H) st8<DT>(q.gx + (p * q.H + 2 * k + r) * q.W + c0, q.W - c0, acc[r]);
  }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------
static bool neck_source_dims(int mode, int H, int W, int given_h, int given_w, int* hs, int* ws) {
  if (mode == SSDK_FUSE_POOL2) {
    *hs = given_h;
    *ws = given_w;
    return given_h / 2 == H && given_w / 2 == W;
  }
  *hs = mode == SSDK_FUSE_UP2 ? H / 2 : H;
  *ws = mode == SSDK_FUSE_UP2 ? W / 2 : W;
  return true;
}

// geometry shared by forward and backward; nothing touches the device
static int neck_check(const char* who, int nsrc, int N, int C, int H, int W, int mode_b, int hb, int wb, int mode_c, int hc, int wc, int dtype,
                      NeckParams* q) {
  if (dtype != SSDK_BF16 && dtype != SSDK_F16) {
    set_error("%s: dtype must be bf16 or f16", who);
    return SSDK_E_BADARG;
  }
  if (N < 1 || C < 1 || H < 1 || W < 1 || (long)N * C * H * W >= (1L << 31)) {
    set_error("%s: bad geometry N=%d C=%d H=%d W=%d (each >= 1, below 2^31 elements)", who, N, C, H, W);
    return SSDK_E_BADARG;
  }
  if ((nsrc != 2 && nsrc != 3) || mode_b < 0 || mode_b > 2 || (nsrc == 3 && (mode_c < 0 || mode_c > 2))) {
    set_error("%s: %d sources (2 | 3) or a mode out of range (%d / %d)", who, nsrc, mode_b, mode_c);
    return SSDK_E_BADARG;
  }
  if ((mode_b == SSDK_FUSE_UP2 || (nsrc == 3 && mode_c == SSDK_FUSE_UP2)) && ((H | W) & 1)) {
    set_error("%s: an upsampled source needs even output dims (%dx%d)", who, H, W);
    return SSDK_E_BADARG;
  }
  memset(q, 0, sizeof(*q));
  if (!neck_source_dims(mode_b, H, W, hb, wb, &q->hb, &q->wb) || (nsrc == 3 && !neck_source_dims(mode_c, H, W, hc, wc, &q->hc, &q->wc))) {
    set_error("%s: pooled source dims (%dx%d / %dx%d) do not reduce to the output %dx%d", who, hb, wb, hc, wc, H, W);
    return SSDK_E_BADARG;
  }
  q->nsrc = nsrc;
  q->mode_b = mode_b;
  q->mode_c = mode_c;
  q->P = N * C;
  q->H = H;
  q->W = W;
  q->HT = (H + 1) / 2;
  q->S = (W + 7) / 8;
  q->items = (long)q->P * q->HT * q->S;
  return SSDK_OK;
}

static unsigned neck_blocks(long items) {
  const long b = (items + kNeckThreads - 1) / kNeckThreads;
  return (unsigned)(b < kNeckMaxBlocks ? b : kNeckMaxBlocks);
}

}  // namespace ssdk

using namespace ssdk;

extern "C" int ssdk_neck_fuse_fwd(const void* a, const void* b, const void* c, const float* w, int w_stride, void* y, int N, int C, int H,
                                  int W, int mode_b, int hb, int wb, int mode_c, int hc, int wc, int dtype, void* stream) {
  NeckParams q;
  if (int rc = neck_check("neck_fuse_fwd", c ? 3 : 2, N, C, H, W, mode_b, hb, wb, mode_c, hc, wc, dtype, &q)) return rc;
  if (!a || !b || !y || (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)y) & 1u) || ((uintptr_t)w & 3u) || (w && w_stride < 1)) {
    set_error("neck_fuse_fwd: null pointer (a, b and y are mandatory), a misaligned tensor or weight pointer, or a weight stride < 1");
    return SSDK_E_BADARG;
  }
  q.a = (const u16*)a;
  q.b = (const u16*)b;
  q.c = (const u16*)c;
  q.y = (u16*)y;
  q.w = w;
  q.wstride = w_stride;
  const dim3 grid((unsigned)((q.items + kNeckThreads - 1) / kNeckThreads));
  if (dtype == SSDK_BF16) hipLaunchKernelGGL((neck_fuse_fwd_kernel<SSDK_BF16>), grid, dim3(kNeckThreads), 0, (hipStream_t)stream, q);
  else hipLaunchKernelGGL((neck_fuse_fwd_kernel<SSDK_F16>), grid, dim3(kNeckThreads), 0, (hipStream_t)stream, q);
  return check_launch("neck_fuse_fwd_kernel");
}

extern "C" size_t ssdk_neck_fuse_bwd_workspace_bytes(int N, int C, int H, int W) {
  if (N < 1 || C < 1 || H < 1 || W < 1 || (long)N * C * H * W >= (1L << 31)) return 0;
  const long items = (long)N * C * ((H + 1) / 2) * ((W + 7) / 8);
  return (size_t)neck_blocks(items) * 3 * sizeof(float);
}

extern "C" int ssdk_neck_fuse_bwd(const void* gy, const void* a, const void* b, const void* c, int nsrc, const float* w, int w_stride, void* ga,
                                  void* gb, void* gc, float* gw, int gw_cols, int gw_col, void* workspace, size_t workspace_bytes, int N,
                                  int C, int H, int W, int mode_b, int hb, int wb, int mode_c, int hc, int wc, int dtype, void* stream) {
  NeckParams q;
  if (int rc = neck_check("neck_fuse_bwd", nsrc, N, C, H, W, mode_b, hb, wb, mode_c, hc, wc, dtype, &q)) return rc;
  if (!gy || (((uintptr_t)gy | (uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)ga | (uintptr_t)gb | (uintptr_t)gc) & 1u) ||
      (((uintptr_t)w | (uintptr_t)gw) & 3u) || (w && w_stride < 1)) {
    set_error("neck_fuse_bwd: null gy, a misaligned tensor, weight or weight-gradient pointer, or a weight stride < 1");
    return SSDK_E_BADARG;
  }
  if (!w && (ga || gw)) {
    set_error("neck_fuse_bwd: without weights ga is gy itself and there is no weight gradient: pass ga = gw = NULL");
    return SSDK_E_BADARG;
  }
  if (nsrc == 2 && (c || gc)) {
    set_error("neck_fuse_bwd: c / gc given with two sources");
    return SSDK_E_BADARG;
  }
  // a source is read for the weight gradient and for the arg-max of a pooled gradient
  if ((gw && (!a || !b || (nsrc == 3 && !c))) || (gb && mode_b == SSDK_FUSE_POOL2 && !b) || (gc && mode_c == SSDK_FUSE_POOL2 && !c)) {
    set_error("neck_fuse_bwd: null source (every source with gw; a pooled source with its gradient)");
    return SSDK_E_BADARG;
  }
  const size_t need = ssdk_neck_fuse_bwd_workspace_bytes(N, C, H, W);
  if (gw && (gw_cols < 1 || gw_col < 0 || gw_col >= gw_cols || !workspace || ((uintptr_t)workspace & 3u) || workspace_bytes < need)) {
    set_error("neck_fuse_bwd: gw column %d of %d, or workspace null / misaligned / too small (%zu bytes given, %zu needed)", gw_col, gw_cols,
              workspace_bytes, need);
    return SSDK_E_BADARG;
  }
  if (!ga && !gb && !gc && !gw) return SSDK_OK;
  q.gy = (const u16*)gy;
  q.a = (const u16*)a;
  q.b = (const u16*)b;
  q.c = (const u16*)c;
  q.ga = (u16*)ga;
  q.gb = (u16*)gb;
  q.gc = (u16*)gc;
  q.w = w;
  q.wstride = w_stride;
  q.part = gw ? (float*)workspace : nullptr;
  const unsigned blocks = neck_blocks(q.items);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == SSDK_BF16) hipLaunchKernelGGL((neck_fuse_bwd_kernel<SSDK_BF16>), dim3(blocks), dim3(kNeckThreads), 0, st, q);
  else hipLaunchKernelGGL((neck_fuse_bwd_kernel<SSDK_F16>), dim3(blocks), dim3(kNeckThreads), 0, st, q);
  if (int rc = check_launch("neck_fuse_bwd_kernel")) return rc;
  if (gw) {
    hipLaunchKernelGGL(neck_fuse_gw_kernel, dim3(1), dim3(kNeckThreads), 0, st, q.part, (int)blocks, gw, nsrc, gw_cols, gw_col);
    return check_launch("neck_fuse_bwd_kernel+neck_fuse_gw_kernel");
  }
  return SSDK_OK;
}

static int pool_train_check(const char* who, const void* p0, const void* p1, const void* p2, int N, int C, int H, int W, int dtype) {
  if (dtype != SSDK_BF16 && dtype != SSDK_F16) {
    set_error("%s: dtype must be bf16 or f16", who);
    return SSDK_E_BADARG;
  }
  if (N < 1 || C < 1 || H < 1 || W < 1 || (long)N * C * H * W >= (1L << 31)) {
    set_error("%s: bad geometry N=%d C=%d H=%d W=%d (each >= 1, below 2^31 elements)", who, N, C, H, W);
    return SSDK_E_BADARG;
  }
  if (!p0 || !p1 || !p2 || (((uintptr_t)p0 | (uintptr_t)p1 | (uintptr_t)p2) & 1u)) {
    set_error("%s: null or misaligned pointer", who);
    return SSDK_E_BADARG;
  }
  return SSDK_OK;
}

extern "C" int ssdk_maxpool3x3s2_train_fwd(const void* x, void* y, int N, int C, int H, int W, int dtype, void* stream) {
  if (int rc = pool_train_check("maxpool3x3s2_train_fwd", x, y, y, N, C, H, W, dtype)) return rc;
  PoolTrainParams q;
  memset(&q, 0, sizeof(q));
  q.x = (const u16*)x;
  q.y = (u16*)y;
  q.P = N * C;
  q.H = H;
  q.W = W;
  q.Ho = (H - 1) / 2 + 1;
  q.Wo = (W - 1) / 2 + 1;
  q.R = q.Ho;
  q.S = (q.Wo + 7) / 8;
  q.items = (long)q.P * q.R * q.S;
  const dim3 grid((unsigned)((q.items + kNeckThreads - 1) / kNeckThreads));
  if (dtype == SSDK_BF16) hipLaunchKernelGGL((maxpool_train_fwd_kernel<SSDK_BF16>), grid, dim3(kNeckThreads), 0, (hipStream_t)stream, q);
  else hipLaunchKernelGGL((maxpool_train_fwd_kernel<SSDK_F16>), grid, dim3(kNeckThreads), 0, (hipStream_t)stream, q);
  return check_launch("maxpool_train_fwd_kernel");
}

extern "C" int ssdk_maxpool3x3s2_train_bwd(const void* x, const void* gy, void* gx, int N, int C, int H, int W, int dtype, void* stream) {
  if (int rc = pool_train_check("maxpool3x3s2_train_bwd", x, gy, gx, N, C, H, W, dtype)) return rc;
  PoolTrainParams q;
  memset(&q, 0, sizeof(q));
  q.x = (const u16*)x;
  q.gy = (const u16*)gy;
  q.gx = (u16*)gx;
  q.P = N * C;
  q.H = H;
  q.W = W;
  q.Ho = (H - 1) / 2 + 1;
  q.Wo = (W - 1) / 2 + 1;
  q.R = (H + 1) / 2;
  q.S = (W + 7) / 8;
  q.items = (long)q.P * q.R * q.S;
  const dim3 grid((unsigned)((q.items + kNeckThreads - 1) / kNeckThreads));
  if (dtype == SSDK_BF16) hipLaunchKernelGGL((maxpool_train_bwd_kernel<SSDK_BF16>), grid, dim3(kNeckThreads), 0, (hipStream_t)stream, q);
  else hipLaunchKernelGGL((maxpool_train_bwd_kernel<SSDK_F16>), grid, dim3(kNeckThreads), 0, (hipStream_t)stream, q);
  return check_launch("maxpool_train_bwd_kernel");
}
