// ssdk_map.h -- what the two average-precision translation units share (ssdk_map.hip: one IoU threshold, the reference's rule;
// ssdk_apsweep.hip: up to 16 thresholds in one launch, the reference's rule or the COCO rule; ssdk_cocoeval.hip: the COCO rule with
// area ranges, crowd boxes and maxDets): the launch shape, the IoU of a
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
// `counts(j)` says which records take part at all: a record that does not (COCO: ignored, or beyond maxDets) is neither a true
// nor a false positive, so the rank of a record is the number of counting records up to and including it.
template <class IsTp, class Counts, class Weight>
__device__ __forceinline__ double map_envelope_sum(long long n, u32 lane, IsTp is_tp, Counts counts, Weight weight) {
  long long T = 0, N = 0;
  for (long long j = 0; j < n; j += 64) {
    const bool c = (j + lane < n) && counts(j + lane);
    const bool t = c && is_tp(j + lane);
    T += __popcll(__ballot(t));
    N += __popcll(__ballot(c));
  }
  double carry = 0.0, acc = 0.0;
  long long tp_ge = 0, n_ge = 0;  // true positives / counting records at ranks >= the current chunk
  for (long long j = ((n - 1) / 64) * 64; j >= 0 && n > 0; j -= 64) {
    const bool c = (j + lane < n) && counts(j + lane);
    const bool t = c && is_tp(j + lane);
    const u64 m = __ballot(t), mc = __ballot(c);
    tp_ge += __popcll(m);
    n_ge += __popcll(mc);
    const u64 upto = (lane == 63u) ? ~0ull : ((2ull << lane) - 1ull);
    const long long tpj = (T - tp_ge) + (long long)__popcll(m & upto);
    const long long nj = (N - n_ge) + (long long)__popcll(mc & upto);
    // :136-137  prec = tp / max(tp + fp, eps) with tp + fp = the record's rank
    double pr = c ? (double)tpj / (double)nj : 0.0;
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

// every record counts: its rank is its position
template <class IsTp, class Weight>
__device__ __forceinline__ double map_envelope_sum(long long n, u32 lane, IsTp is_tp, Weight weight) {
  return map_envelope_sum(n, lane, is_tp, [](long long) { return true; }, weight);
}

// :108-111  the VOC area: recall moves exactly at the true positives, by 1 / npos each
struct MapVocWeight {
  double dnp;
  __device__ __forceinline__ double operator()(long long tpj) const { return (double)tpj / dnp - (double)(tpj - 1) / dnp; }
};

// how many of the 101 recall points r_k = k * 0.01 (r_100 = 1.0: numpy.linspace(0, 1, 101)) are <= x, compared in fp64
__device__ __forceinline__ int coco_points_le(double x) {
  int k = (int)(x * 100.0) + 2;
  if (k > 100) k = 100;
  while (k >= 0 && (k == 100 ? 1.0 : (double)k * 0.01) > x) --k;
  return k + 1;
}

// 101-point interpolation as a sum over the true positives: the k-th one is the first rank whose recall is k / npos, so it answers
// the recall points in ((k - 1) / npos, k / npos]; the first also answers r_0 = 0, whose envelope value is the same (precision is 0
// before the first true positive).  The sum is divided by 101 afterwards.
struct MapCocoWeight {
  double dnp;
  __device__ __forceinline__ double operator()(long long tpj) const {
    const int hi = coco_points_le((double)tpj / dnp);
    const int lo = tpj == 1 ? 0 : coco_points_le((double)(tpj - 1) / dnp);
    return (double)(hi - lo);
  }
};

}  // namespace ssdk
