// ssdk_map.h -- what the two average-precision translation units share (ssdk_map.hip: one IoU threshold, the reference's rule;
// ssdk_apsweep.hip: up to 16 thresholds in one launch, the reference's rule or the COCO rule): the launch shape, the IoU of a
// detection with a staged ground-truth box and the right-to-left walk over a class's sorted records.  One definition each, so
// that the sweep at T = 1 cannot drift from the bits of ssdk_map_match / ssdk_map_average_precision.
#pragma once
#include "ssdk_common.h"

namespace ssdk {

constexpr int kMapThreads = 256;
constexpr int kMapPer = 8;  // detections per thread: D <= kMapThreads * kMapPer

// IoU in fp32 in the reference's operation order (evaluation_metrics.py:16-26, no +1 on the widths); g = ltrb of a box.
__device__ __forceinline__ float map_iou(float x1, float y1, float x2, float y2, float area_a, const float* g) {
  const float lx = fmaxf(x1, g[0]), ly = fmaxf(y1, g[1]);  // :20-21
  const float rx = fminf(x2, g[2]), ry = fminf(y2, g[3]);
  const float inter = (lx < rx && ly < ry) ? (rx - lx) * (ry - ly) : 0.f;  // :23
  const float area_b = (g[2] - g[0]) * (g[3] - g[1]);                      // :25
  return inter / (area_a + area_b - inter);                                // :26
}

// One wave over the n records of a class, sorted by score descending: precision tp / rank in fp64 at every rank, its running
// maximum from the right (the envelope), summed over the true positives as  weight(k) * envelope  where k counts the true
// positives up to and including this one.  is_tp(j) reads the flag of record j of the class.  Every lane returns the sum.
template <class IsTp, class Weight>
__device__ __forceinline__ double map_envelope_sum(long long n, u32 lane, IsTp is_tp, Weight weight) {
  long long T = 0;
  for (long long j = 0; j < n; j += 64) {
    const bool t = (j + lane < n) && is_tp(j + lane);
    T += __popcll(__ballot(t));
  }
  double carry = 0.0, acc = 0.0;
  long long tp_ge = 0;  // true positives at ranks >= the current chunk
  for (long long j = ((n - 1) / 64) * 64; j >= 0 && n > 0; j -= 64) {
    const bool in = j + lane < n;
    const bool t = in && is_tp(j + lane);
    const u64 m = __ballot(t);
    tp_ge += __popcll(m);
    const long long tpj = (T - tp_ge) + (long long)__popcll(m & ((lane == 63u) ? ~0ull : ((2ull << lane) - 1ull)));
    // :136-137  prec = tp / max(tp + fp, eps) with tp + fp = rank + 1
    double pr = in ? (double)tpj / (double)(j + lane + 1) : 0.0;
    pr = pr > carry ? pr : carry;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {  // suffix maximum across the wave (:104-106)
      const double o = __shfl_down(pr, d);
      if (lane + d < 64u) pr = pr > o ? pr : o;
    }
    carry = __shfl(pr, 0);
    if (t) acc += weight(tpj) * pr;
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) acc += __shfl_xor(acc, d);
  return acc;
}

// :108-111  the VOC area: recall moves exactly at the true positives, by 1 / npos each
struct MapVocWeight {
  double dnp;
  __device__ __forceinline__ double operator()(long long tpj) const { return (double)tpj / dnp - (double)(tpj - 1) / dnp; }
};

}  // namespace ssdk
