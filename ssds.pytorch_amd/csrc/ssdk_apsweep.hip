// ssdk_apsweep.hip -- average precision over a sweep of IoU thresholds on gfx950 (include/ssdk_apsweep.h): the bookkeeping of
// AP@[.50:.95].  ssdk_map.hip answers one threshold with the reference's rule; ten thresholds there are ten launches per batch and
// ten sorts per epoch, and the COCO rule (greedy, a box is taken once per threshold) cannot be expressed with it at all.
//
//  apsweep_reference_kernel  one workgroup per image, the rule of map_match_kernel at every threshold: a detection's box (same
//                            class, highest IoU, first maximum) does not depend on the threshold, so the IoUs are computed once;
//                            per (threshold, box) one LDS atomicMin slot finds the detection of lowest index that reaches it.
//  apsweep_coco_kernel       one workgroup per image.  Phase 1: which detections count (score, class range, the first max_dets of
//                            them by index) from wave ballots.  Phase 2: the distinct ground-truth classes of the image ("leaders":
//                            a class without ground truth has false positives only, which is what the mask starts as).  Phase 3:
//                            the chains -- those of different (class, threshold) pairs are independent, those of one pair are
//                            sequential: a wave takes a class, walks its detections in index order, its lanes hold the IoUs of one
//                            detection against up to 4 x 64 boxes (each computed once, not once per threshold), and every lane keeps
//                            the taken-set of its boxes as one bit per threshold.  Per threshold one wave-wide maximum of
//                            (IoU bits, box index) picks the box: highest IoU, then highest index.
//  apsweep_ap_kernel         grid (class, threshold), one wave each over the sorted records: the walk of map_ap_kernel
//                            (ssdk_map.h) with the VOC weight or the 101-point weight.
//
// Nothing here is a float atomic, and no result depends on which wave runs first: the bits are reproducible.
#include "ssdk_map.h"

#include "../../include/ssdk_apsweep.h"

namespace ssdk {

constexpr int kSweepSlots = kMapThreads * kMapPer;  // 2048 detection slots of an image
constexpr int kSweepChunks = kSweepSlots / 64;      // 32 wave-sized chunks of them
constexpr int kSweepGtChunks = SSDK_MAX_GT / 64;    // 4 wave-sized chunks of ground-truth boxes
static_assert(SSDK_MAX_GT == 256 && kMapThreads == SSDK_MAX_GT, "one thread per ground-truth box; 4 x 64 boxes per lane set");

struct SweepParams {
  const float* scores;   // [B, D]
  const float* boxes;    // [B, D, 4] ltrb
  const float* classes;  // [B, D]
  const float* targets;  // [B, G, 5] ltrb + label (label < 0: padding)
  int D, G, C, T, max_dets;
  float conf_thr;
  float thr[SSDK_APSWEEP_MAX_T];
  long long* keys;  // [B, D]
  int* mask;        // [B, D]
  int* npos;        // [C], accumulated
};

// ground truth of image b into LDS, its boxes counted per class (integer atomics), the thresholds next to it
__device__ __forceinline__ void sweep_stage(const SweepParams& p, int b, int tid, float (*gt)[5], float* thr) {
  for (int g = tid; g < p.G; g += kMapThreads) {
    const float* t = p.targets + ((size_t)b * p.G + g) * 5;
#pragma unroll
    for (int k = 0; k < 5; ++k) gt[g][k] = t[k];
    const float lab = t[4];
    if (lab >= 0.f && lab < (float)p.C) atomicAdd(&p.npos[(int)lab], 1);  // evaluation_metrics.py:36,56
  }
  if (tid < SSDK_APSWEEP_MAX_T) {
    float v = 2.f;  // (never reached: an IoU is at most 1)
#pragma unroll
    for (int k = 0; k < SSDK_APSWEEP_MAX_T; ++k)
      if (k == tid && k < p.T) v = p.thr[k];
    thr[tid] = v;
  }
}

__device__ __forceinline__ long long sweep_key(u32 cls, float s) {
  // ascending key order = (class ascending, score descending); slots of equal key keep their arrival order under a stable sort
  return (long long)(((u64)cls << 32) | (u64)(~ord_f32(s)));
}

__global__ __launch_bounds__(kMapThreads) void apsweep_reference_kernel(const SweepParams p) {
  __shared__ float gt[SSDK_MAX_GT][5];
  __shared__ float thr[SSDK_APSWEEP_MAX_T];
  __shared__ int first[SSDK_APSWEEP_MAX_T][SSDK_MAX_GT];
  const int tid = (int)threadIdx.x, b = (int)blockIdx.x;
  sweep_stage(p, b, tid, gt, thr);
  for (int t = 0; t < p.T; ++t)
    for (int g = tid; g < p.G; g += kMapThreads) first[t][g] = 0x7fffffff;
  __syncthreads();

  int best_g[kMapPer], reach[kMapPer];  // the detection's box and how many thresholds its IoU reaches (they ascend)
#pragma unroll
  for (int r = 0; r < kMapPer; ++r) {
    best_g[r] = -1;
    reach[r] = 0;
    const int i = tid + r * kMapThreads;
    if (i >= p.D) continue;
    const size_t o = (size_t)b * p.D + i;
    const float s = p.scores[o];
    if (!(s > p.conf_thr)) continue;  // evaluation_metrics.py:29-31
    const float c = p.classes[o];
    const float x1 = p.boxes[o * 4 + 0], y1 = p.boxes[o * 4 + 1], x2 = p.boxes[o * 4 + 2], y2 = p.boxes[o * 4 + 3];
    const float area_a = (x2 - x1) * (y2 - y1);  // evaluation_metrics.py:24
    float best = 0.f;
    int bg = -1;
    for (int g = 0; g < p.G; ++g) {
      if (gt[g][4] != c) continue;  // evaluation_metrics.py:33
      const float iou = map_iou(x1, y1, x2, y2, area_a, gt[g]);  // :20-26
      if (bg < 0 || iou > best) {  // :49 argmax, first maximum
        best = iou;
        bg = g;
      }
    }
    if (bg < 0) continue;
    int nt = 0;
    while (nt < p.T && best >= thr[nt]) {  // :54 at every threshold
      atomicMin(&first[nt][bg], i);
      ++nt;
    }
    if (nt > 0) {
      best_g[r] = bg;
      reach[r] = nt;
    }
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < kMapPer; ++r) {
    const int i = tid + r * kMapThreads;
    if (i >= p.D) continue;
    const size_t o = (size_t)b * p.D + i;
    const float s = p.scores[o];
    const float c = p.classes[o];
    const bool valid = (s > p.conf_thr) && c >= 0.f && c < (float)p.C;
    p.keys[o] = sweep_key(valid ? (u32)c : (u32)p.C, s);
    int m = 0;
    for (int t = 0; t < reach[r]; ++t)
      if (first[t][best_g[r]] == i) m |= 1 << t;  // :54-56
    p.mask[o] = m;
  }
}

__global__ __launch_bounds__(kMapThreads) void apsweep_coco_kernel(const SweepParams p) {
  __shared__ float gt[SSDK_MAX_GT][5];
  __shared__ float thr[SSDK_APSWEEP_MAX_T];
  __shared__ int mask[kSweepSlots];    // the true-positive bits of every slot: 0 unless a chain says otherwise
  __shared__ u64 keep[kSweepChunks];   // bit l of keep[j]: detection 64 j + l counts
  __shared__ int cnt[kSweepChunks];    // valid detections per chunk
  __shared__ int lead[SSDK_MAX_GT];    // the first box of every class that has ground truth in this image
  __shared__ int wave_leads[kMapThreads / 64];
  const int tid = (int)threadIdx.x, b = (int)blockIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const u64 below = (1ull << lane) - 1ull;  // the lanes before this one
  sweep_stage(p, b, tid, gt, thr);

  // ---- phase 1: the detections that count.  Slot i = 256 r + tid is lane `lane` of chunk 4 r + wave.
  bool valid[kMapPer];
#pragma unroll
  for (int r = 0; r < kMapPer; ++r) {
    const int i = tid + r * kMapThreads;
    valid[r] = false;
    if (i < p.D) {
      const size_t o = (size_t)b * p.D + i;
      const float s = p.scores[o], c = p.classes[o];
      valid[r] = (s > p.conf_thr) && c >= 0.f && c < (float)p.C;
    }
    const u64 m = __ballot(valid[r]);
    if (lane == 0) cnt[r * 4 + wave] = __popcll(m);
    mask[i] = 0;
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < kMapPer; ++r) {  // only the first max_dets valid detections of the image, by index
    const int chunk = r * 4 + wave;
    int rank = 0;
    for (int j = 0; j < chunk; ++j) rank += cnt[j];
    const u64 m = __ballot(valid[r]);
    rank += __popcll(m & below);
    const u64 k = __ballot(valid[r] && rank < p.max_dets);
    if (lane == 0) keep[chunk] = k;
  }

  // ---- phase 2: leaders.  Thread g looks at box g (G <= 256 = the workgroup).
  bool leader = false;
  if (tid < p.G) {
    const float lab = gt[tid][4];
    leader = lab >= 0.f && lab < (float)p.C;
    for (int g = 0; g < tid && leader; ++g) leader = gt[g][4] != lab;
  }
  const u64 lm = __ballot(leader);
  if (lane == 0) wave_leads[wave] = __popcll(lm);
  __syncthreads();
  int nlead = 0, at = 0;
#pragma unroll
  for (int w = 0; w < kMapThreads / 64; ++w) {
    if (w < wave) at += wave_leads[w];
    nlead += wave_leads[w];
  }
  if (leader) lead[at + __popcll(lm & below)] = tid;
  __syncthreads();

  // ---- phase 3: the chains, a class per wave
  const int nchunk = (p.D + 63) >> 6, ngt = (p.G + 63) >> 6;
  for (int li = wave; li < nlead; li += kMapThreads / 64) {
    const float c = gt[lead[li]][4];
    bool mine_gt[kSweepGtChunks];
    u32 taken[kSweepGtChunks];  // bit t: this lane's box of chunk k is taken at threshold t
#pragma unroll
    for (int k = 0; k < kSweepGtChunks; ++k) {
      const int g = k * 64 + lane;
      mine_gt[k] = g < p.G && gt[g][4] == c;
      taken[k] = 0;
    }
    for (int j = 0; j < nchunk; ++j) {
      const int i = j * 64 + lane;
      bool mine = ((keep[j] >> lane) & 1ull) != 0;  // (a kept slot is inside D)
      float x1 = 0.f, y1 = 0.f, x2 = 0.f, y2 = 0.f;
      if (mine) {
        const size_t o = (size_t)b * p.D + i;
        mine = p.classes[o] == c;
        if (mine) {
          x1 = p.boxes[o * 4 + 0];
          y1 = p.boxes[o * 4 + 1];
          x2 = p.boxes[o * 4 + 2];
          y2 = p.boxes[o * 4 + 3];
        }
      }
      u64 todo = __ballot(mine);
      while (todo) {  // the class's detections of this chunk, in index order (wave-uniform)
        const int src = __ffsll((long long)todo) - 1;
        todo &= todo - 1ull;
        const float ax1 = __shfl(x1, src), ay1 = __shfl(y1, src), ax2 = __shfl(x2, src), ay2 = __shfl(y2, src);
        const float area_a = (ax2 - ax1) * (ay2 - ay1);
        float iou[kSweepGtChunks];
#pragma unroll
        for (int k = 0; k < kSweepGtChunks; ++k) {
          iou[k] = -1.f;
          if (k < ngt && mine_gt[k]) iou[k] = map_iou(ax1, ay1, ax2, ay2, area_a, gt[k * 64 + lane]);  // (k < ngt: wave-uniform)
        }
        int bits = 0;
        for (int t = 0; t < p.T; ++t) {
          const float th = thr[t];
          bool reaches = false;
          u64 key = 0;  // (IoU bits, box index) of this lane's best free box: an IoU >= th > 0 has non-zero, monotone bits
#pragma unroll
          for (int k = 0; k < kSweepGtChunks; ++k) {
            if (!(iou[k] >= th)) continue;  // (a NaN IoU of two empty boxes reaches nothing)
            reaches = true;
            if ((taken[k] >> t) & 1u) continue;
            const u64 kk = ((u64)__builtin_bit_cast(u32, iou[k]) << 32) | (u64)(u32)(k * 64 + lane);
            key = kk > key ? kk : key;
          }
          if (__ballot(reaches) == 0) break;  // the thresholds ascend: nothing reaches a later one either
          const u64 have = __ballot(key != 0);
          if (have == 0) continue;
          if (have & (have - 1ull)) {
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) {
              const u64 other = __shfl_xor(key, d);
              key = other > key ? other : key;
            }
          } else {  // one lane has a free box (the usual case: a detection overlaps one box of its class): no reduction
            key = __shfl(key, __ffsll((long long)have) - 1);
          }
          const int g = (int)(u32)key;  // highest IoU, then highest index
          if (lane == (g & 63)) {
#pragma unroll
            for (int k = 0; k < kSweepGtChunks; ++k)
              if (k == (g >> 6)) taken[k] |= 1u << t;
          }
          bits |= 1 << t;
        }
        if (lane == 0) mask[j * 64 + src] = bits;
      }
    }
  }
  __syncthreads();

#pragma unroll
  for (int r = 0; r < kMapPer; ++r) {
    const int i = tid + r * kMapThreads;
    if (i >= p.D) continue;
    const size_t o = (size_t)b * p.D + i;
    const bool kept = ((keep[r * 4 + wave] >> lane) & 1ull) != 0;
    p.keys[o] = sweep_key(kept ? (u32)p.classes[o] : (u32)p.C, p.scores[o]);
    p.mask[o] = mask[i];
  }
}

// records sorted by key; seg[c] .. seg[c+1] is class c.  ap[t * C + c] = NaN when the class has no ground truth, 0 when it has no
// detections.
__global__ __launch_bounds__(64) void apsweep_ap_kernel(const int* mask, const long long* seg, const int* npos, int C, int rule,
                                                        double* ap) {
  const int c = (int)blockIdx.x, t = (int)blockIdx.y;
  const u32 lane = threadIdx.x;
  const long long s0 = seg[c], n = seg[c + 1] - seg[c];
  const int np = npos[c];
  double* out = ap + (size_t)t * C + c;
  if (np == 0) {
    if (lane == 0) *out = __builtin_nan("");
    return;
  }
  const int* m = mask + s0;
  auto is_tp = [m, t](long long j) { return ((m[j] >> t) & 1) != 0; };
  double acc;
  if (rule == SSDK_AP_RULE_REFERENCE)
    acc = map_envelope_sum(n, lane, is_tp, MapVocWeight{(double)np});
  else
    acc = map_envelope_sum(n, lane, is_tp, MapCocoWeight{(double)np}) / 101.0;
  if (lane == 0) *out = acc;
}

}  // namespace ssdk

extern "C" int ssdk_apsweep_match(const float* scores, const float* boxes, const float* classes, int B, int D,
                                  const float* targets, int G, int num_classes, float conf_threshold,
                                  const float* iou_thresholds, int T, int rule, int max_dets, long long* keys, int* tp_mask,
                                  int* npos, void* stream) {
  using namespace ssdk;
  if (!scores || !boxes || !classes || !targets || !iou_thresholds || !keys || !tp_mask || !npos) {
    set_error("apsweep_match: null pointer");
    return SSDK_E_BADARG;
  }
  if (B < 1 || D < 1 || D > kSweepSlots || G < 0 || G > SSDK_MAX_GT || num_classes < 1) {
    set_error("apsweep_match: bad dims B=%d D=%d (<=%d) G=%d (<=%d) classes=%d", B, D, kSweepSlots, G, SSDK_MAX_GT, num_classes);
    return SSDK_E_BADARG;
  }
  if (T < 1 || T > SSDK_APSWEEP_MAX_T) {
    set_error("apsweep_match: T=%d IoU thresholds (1 .. %d)", T, SSDK_APSWEEP_MAX_T);
    return SSDK_E_BADARG;
  }
  for (int t = 0; t < T; ++t) {
    const float v = iou_thresholds[t];
    if (!(v > 0.f && v <= 1.f) || (t > 0 && !(v > iou_thresholds[t - 1]))) {
      set_error("apsweep_match: iou_thresholds[%d] = %g: the thresholds must lie in (0, 1] and ascend strictly", t, (double)v);
      return SSDK_E_BADARG;
    }
  }
  if (rule != SSDK_AP_RULE_REFERENCE && rule != SSDK_AP_RULE_COCO) {
    set_error("apsweep_match: unknown rule %d (SSDK_AP_RULE_REFERENCE | SSDK_AP_RULE_COCO)", rule);
    return SSDK_E_BADARG;
  }
  if (max_dets < 1) {
    set_error("apsweep_match: max_dets=%d (>= 1)", max_dets);
    return SSDK_E_BADARG;
  }
  SweepParams p;
  p.scores = scores;
  p.boxes = boxes;
  p.classes = classes;
  p.targets = targets;
  p.D = D;
  p.G = G;
  p.C = num_classes;
  p.T = T;
  p.max_dets = max_dets;
  p.conf_thr = conf_threshold;
  for (int t = 0; t < SSDK_APSWEEP_MAX_T; ++t) p.thr[t] = t < T ? iou_thresholds[t] : 2.f;
  p.keys = keys;
  p.mask = tp_mask;
  p.npos = npos;
  if (rule == SSDK_AP_RULE_REFERENCE) {
    hipLaunchKernelGGL(apsweep_reference_kernel, dim3((unsigned)B), dim3(kMapThreads), 0, (hipStream_t)stream, p);
    return check_launch("apsweep_reference_kernel");
  }
  hipLaunchKernelGGL(apsweep_coco_kernel, dim3((unsigned)B), dim3(kMapThreads), 0, (hipStream_t)stream, p);
  return check_launch("apsweep_coco_kernel");
}

extern "C" int ssdk_apsweep_average_precision(const int* tp_mask_sorted, const long long* seg_offsets, const int* npos,
                                              int num_classes, int T, int rule, double* ap, void* stream) {
  using namespace ssdk;
  if (!tp_mask_sorted || !seg_offsets || !npos || !ap) {
    set_error("apsweep_average_precision: null pointer");
    return SSDK_E_BADARG;
  }
  if (num_classes < 1 || T < 1 || T > SSDK_APSWEEP_MAX_T) {
    set_error("apsweep_average_precision: classes=%d T=%d (1 .. %d)", num_classes, T, SSDK_APSWEEP_MAX_T);
    return SSDK_E_BADARG;
  }
  if (rule != SSDK_AP_RULE_REFERENCE && rule != SSDK_AP_RULE_COCO) {
    set_error("apsweep_average_precision: unknown rule %d (SSDK_AP_RULE_REFERENCE | SSDK_AP_RULE_COCO)", rule);
    return SSDK_E_BADARG;
  }
  hipLaunchKernelGGL(apsweep_ap_kernel, dim3((unsigned)num_classes, (unsigned)T), dim3(64), 0, (hipStream_t)stream,
                     tp_mask_sorted, seg_offsets, npos, num_classes, rule, ap);
  return check_launch("apsweep_ap_kernel");
}
