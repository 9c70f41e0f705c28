// ssdk_cocoeval.hip -- the COCO detection summary on gfx950 (include/ssdk_cocoeval.h): pycocotools' evaluateImg and accumulate
// for boxes with area ranges, crowd (ignore) regions, maxDets per image and category, and recall.  ssdk_apsweep.hip answers one area
// range without ignore regions and cuts max_dets per image; the twelve numbers of the COCO table need the rest.
//
//  cocoeval_match_kernel       one workgroup per image.  Phase 1: which slots count, their class into LDS, and the flags of an
//                              unmatched detection (ignored at every threshold iff its own area is outside the range) -- what a class
//                              without ground truth keeps.  Phase 2: the distinct ground-truth classes of the image ("leaders"), as
//                              apsweep_coco_kernel finds them.  Phase 3: a wave takes a class and walks its detections in index order;
//                              its lanes hold the IoUs of one detection against up to 4 x 64 boxes (each computed once), every lane
//                              keeps the taken-set of its boxes as one bit per (area range, threshold).  Per (range, threshold) ONE
//                              wave-wide maximum of (not ignored, IoU bits, box index) picks the box: a non-ignored box before an
//                              ignored one (the `break` of pycocotools' loop over boxes sorted non-ignored first), then highest IoU,
//                              then highest index.  Phase 4: rank = the counted detections of the same class before the slot.
//  cocoeval_accumulate_kernel  grid (class, threshold, area range x maxDets), one wave each over the sorted records: the walk of
//                              ssdk_map.h over the records that count (rank < maxDets, not ignored) with the 101-point weight.
//
// Nothing here is a float atomic, and no result depends on which wave runs first: the bits are reproducible.
#include "ssdk_map.h"

#include "../../include/ssdk_cocoeval.h"

namespace ssdk {

constexpr int kCocoSlots = kMapThreads * kMapPer;  // 2048 detection slots of an image
constexpr int kCocoGtChunks = SSDK_MAX_GT / 64;    // 4 wave-sized chunks of ground-truth boxes
constexpr int kCocoWaves = kMapThreads / 64;
static_assert(SSDK_MAX_GT == 256 && kMapThreads == SSDK_MAX_GT, "one thread per ground-truth box; 4 x 64 boxes per lane set");
static_assert(SSDK_COCOEVAL_MAX_T == 16 && SSDK_COCOEVAL_MAX_A == 4, "a taken-set is 4 x 16 bits; a flag word is 16 + 16 bits");

struct CocoParams {
  const float* scores;      // [B, D]
  const float* boxes;       // [B, D, 4] ltrb
  const float* classes;     // [B, D]
  const float* targets;     // [B, G, 5] ltrb + label (label < 0: padding)
  const int* gt_crowd;      // [B, G] or null
  const float* gt_area;     // [B, G] or null
  const float* area_scale;  // [B] or null
  int D, G, C, T, A;
  float conf_thr;
  float thr[SSDK_COCOEVAL_MAX_T];
  float rng[2 * SSDK_COCOEVAL_MAX_A];  // lo, hi per area range
  long long* keys;                     // [B, D]
  int* rank;                           // [B, D]
  int* flags;                          // [B, D, A]
  int* npig;                           // [A, C], accumulated
};

struct CocoMaxDets {
  int v[SSDK_COCOEVAL_MAX_M];
};

__device__ __forceinline__ long long coco_key(u32 cls, float s) {
  // the key of ssdk_map_match / ssdk_apsweep_match: ascending key order = (class ascending, score descending)
  return (long long)(((u64)cls << 32) | (u64)(~ord_f32(s)));
}

// intersection / detection area: the "IoU" with a crowd region, the intersection in the operation order of map_iou
__device__ __forceinline__ float coco_crowd_iou(float x1, float y1, float x2, float y2, float area_a, const float* g) {
  const float lx = fmaxf(x1, g[0]), ly = fmaxf(y1, g[1]);
  const float rx = fminf(x2, g[2]), ry = fminf(y2, g[3]);
  const float inter = (lx < rx && ly < ry) ? (rx - lx) * (ry - ly) : 0.f;
  return inter / area_a;
}

__global__ __launch_bounds__(kMapThreads) void cocoeval_match_kernel(const CocoParams p) {
  __shared__ float gt[SSDK_MAX_GT][5];
  __shared__ float garea[SSDK_MAX_GT];
  __shared__ int gcrowd[SSDK_MAX_GT];
  __shared__ float thr[SSDK_COCOEVAL_MAX_T];
  __shared__ float rng[2 * SSDK_COCOEVAL_MAX_A];
  __shared__ float dcls[kCocoSlots];                      // the class of a slot that counts, NaN otherwise (equal to nothing)
  __shared__ int flags[kCocoSlots][SSDK_COCOEVAL_MAX_A];  // starts as "unmatched"; a chain overwrites its detections
  __shared__ int lead[SSDK_MAX_GT];                       // the first box of every class that has ground truth in this image
  __shared__ int wave_leads[kCocoWaves];
  const int tid = (int)threadIdx.x, b = (int)blockIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const u64 below = (1ull << lane) - 1ull;  // the lanes before this one
  const float scale = p.area_scale ? p.area_scale[b] : 1.f;
  const u32 tmask = (1u << p.T) - 1u;

  // ---- stage: ground truth, its area and crowd flag, the thresholds and the ranges
  for (int g = tid; g < p.G; g += kMapThreads) {
    const size_t og = (size_t)b * p.G + g;
    const float* t = p.targets + og * 5;
#pragma unroll
    for (int k = 0; k < 5; ++k) gt[g][k] = t[k];
    garea[g] = p.gt_area ? p.gt_area[og] : ((t[2] - t[0]) * (t[3] - t[1])) * scale;
    gcrowd[g] = p.gt_crowd ? (p.gt_crowd[og] != 0 ? 1 : 0) : 0;
  }
  if (tid < SSDK_COCOEVAL_MAX_T) {
    float v = 2.f;  // (never reached: an IoU is at most 1)
#pragma unroll
    for (int k = 0; k < SSDK_COCOEVAL_MAX_T; ++k)
      if (k == tid && k < p.T) v = p.thr[k];
    thr[tid] = v;
  }
  if (tid < 2 * SSDK_COCOEVAL_MAX_A) {
    float v = 0.f;
#pragma unroll
    for (int k = 0; k < 2 * SSDK_COCOEVAL_MAX_A; ++k)
      if (k == tid) v = p.rng[k];
    rng[tid] = v;
  }
  __syncthreads();

  // ---- phase 1: the slots that count.  Slot i = 256 r + tid.
#pragma unroll
  for (int r = 0; r < kMapPer; ++r) {
    const int i = tid + r * kMapThreads;
    if (i >= p.D) continue;
    const size_t o = (size_t)b * p.D + i;
    const float s = p.scores[o], c = p.classes[o];
    const bool valid = (s > p.conf_thr) && c >= 0.f && c < (float)p.C;
    dcls[i] = valid ? c : __builtin_nanf("");
    const float x1 = p.boxes[o * 4 + 0], y1 = p.boxes[o * 4 + 1], x2 = p.boxes[o * 4 + 2], y2 = p.boxes[o * 4 + 3];
    const float darea = ((x2 - x1) * (y2 - y1)) * scale;
#pragma unroll
    for (int a = 0; a < SSDK_COCOEVAL_MAX_A; ++a) {
      const bool out = a < p.A && (darea < rng[2 * a] || darea > rng[2 * a + 1]);
      flags[i][a] = (valid && out) ? (int)(tmask << 16) : 0;
    }
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
  for (int w = 0; w < kCocoWaves; ++w) {
    if (w < wave) at += wave_leads[w];
    nlead += wave_leads[w];
  }
  if (leader) lead[at + __popcll(lm & below)] = tid;
  __syncthreads();

  // ---- phase 3: the chains, a class per wave
  const int nchunk = (p.D + 63) >> 6, ngt = (p.G + 63) >> 6;
  for (int li = wave; li < nlead; li += kCocoWaves) {
    const float c = gt[lead[li]][4];
    bool mine_gt[kCocoGtChunks], crowd[kCocoGtChunks];
    u32 ign[kCocoGtChunks];    // bit a: this lane's box of chunk k is ignored in area range a
    u64 taken[kCocoGtChunks];  // bit 16 a + t: this lane's box of chunk k is taken at (range a, threshold t)
    int pos[SSDK_COCOEVAL_MAX_A] = {0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < kCocoGtChunks; ++k) {
      const int g = k * 64 + lane;
      mine_gt[k] = g < p.G && gt[g][4] == c;
      crowd[k] = mine_gt[k] && gcrowd[g] != 0;
      taken[k] = 0;
      ign[k] = 0;
      const float ar = mine_gt[k] ? garea[g] : 0.f;
#pragma unroll
      for (int a = 0; a < SSDK_COCOEVAL_MAX_A; ++a) {
        const bool ig = crowd[k] || ar < rng[2 * a] || ar > rng[2 * a + 1];
        if (ig) ign[k] |= 1u << a;
        pos[a] += __popcll(__ballot(mine_gt[k] && !ig));
      }
    }
    if (lane == 0) {
#pragma unroll
      for (int a = 0; a < SSDK_COCOEVAL_MAX_A; ++a)
        if (a < p.A && pos[a] > 0) atomicAdd(&p.npig[(size_t)a * p.C + (int)c], pos[a]);
    }
    for (int j = 0; j < nchunk; ++j) {
      const int i = j * 64 + lane;
      const bool mine = i < p.D && dcls[i] == c;
      float x1 = 0.f, y1 = 0.f, x2 = 0.f, y2 = 0.f;
      if (mine) {
        const size_t o = (size_t)b * p.D + i;
        x1 = p.boxes[o * 4 + 0];
        y1 = p.boxes[o * 4 + 1];
        x2 = p.boxes[o * 4 + 2];
        y2 = p.boxes[o * 4 + 3];
      }
      u64 todo = __ballot(mine);
      while (todo) {  // the class's detections of this chunk, in index order (wave-uniform)
        const int src = __ffsll((long long)todo) - 1;
        todo &= todo - 1ull;
        const float ax1 = __shfl(x1, src), ay1 = __shfl(y1, src), ax2 = __shfl(x2, src), ay2 = __shfl(y2, src);
        const float area_a = (ax2 - ax1) * (ay2 - ay1);
        float iou[kCocoGtChunks];
#pragma unroll
        for (int k = 0; k < kCocoGtChunks; ++k) {
          iou[k] = -1.f;
          if (k < ngt && mine_gt[k])  // (k < ngt: wave-uniform)
            iou[k] = crowd[k] ? coco_crowd_iou(ax1, ay1, ax2, ay2, area_a, gt[k * 64 + lane])
                              : map_iou(ax1, ay1, ax2, ay2, area_a, gt[k * 64 + lane]);
        }
        u32 mbits[SSDK_COCOEVAL_MAX_A] = {0, 0, 0, 0};  // matched at threshold t, per range
        u32 ibits[SSDK_COCOEVAL_MAX_A] = {0, 0, 0, 0};  // ... by an ignored box
        for (int t = 0; t < p.T; ++t) {
          const float th = thr[t];
          bool reaches = false;
#pragma unroll
          for (int k = 0; k < kCocoGtChunks; ++k) reaches = reaches || (iou[k] >= th);  // (a NaN IoU reaches nothing)
          if (__ballot(reaches) == 0) break;  // the thresholds ascend: nothing reaches a later one either
#pragma unroll
          for (int a = 0; a < SSDK_COCOEVAL_MAX_A; ++a) {
            if (a >= p.A) continue;
            // (not ignored, IoU bits, box index) of this lane's best candidate: an IoU >= th > 0 has non-zero, monotone bits below
            // 2^31, so bit 63 is free for "not ignored"
            u64 key = 0;
#pragma unroll
            for (int k = 0; k < kCocoGtChunks; ++k) {
              if (!(iou[k] >= th)) continue;
              if (((taken[k] >> (16 * a + t)) & 1ull) && !crowd[k]) continue;  // a crowd box can be taken again
              const u64 kk = (((ign[k] >> a) & 1u) ? 0ull : (1ull << 63)) | ((u64)__builtin_bit_cast(u32, iou[k]) << 32) |
                             (u64)(u32)(k * 64 + lane);
              key = kk > key ? kk : key;
            }
            const u64 have = __ballot(key != 0);
            if (have == 0) continue;
            if (have & (have - 1ull)) {
#pragma unroll
              for (int d = 32; d >= 1; d >>= 1) {
                const u64 other = __shfl_xor(key, d);
                key = other > key ? other : key;
              }
            } else {  // one lane has a candidate (the usual case): no reduction
              key = __shfl(key, __ffsll((long long)have) - 1);
            }
            const int g = (int)(u32)key;
            if (lane == (g & 63)) {
#pragma unroll
              for (int k = 0; k < kCocoGtChunks; ++k)
                if (k == (g >> 6)) taken[k] |= 1ull << (16 * a + t);
            }
            mbits[a] |= 1u << t;
            if (!(key >> 63)) ibits[a] |= 1u << t;  // the detection inherits the box's ignore flag
          }
        }
        if (lane == 0) {
#pragma unroll
          for (int a = 0; a < SSDK_COCOEVAL_MAX_A; ++a) {
            const u32 unmatched = (u32)flags[j * 64 + src][a] & ~(mbits[a] << 16);  // outside the range: ignored where unmatched
            flags[j * 64 + src][a] = (int)(mbits[a] | (ibits[a] << 16) | unmatched);
          }
        }
      }
    }
  }
  __syncthreads();

  // ---- phase 4: keys, ranks and flags of every slot
#pragma unroll
  for (int r = 0; r < kMapPer; ++r) {
    const int i = tid + r * kMapThreads;
    if (i >= p.D) continue;
    const size_t o = (size_t)b * p.D + i;
    const float c = dcls[i];
    const bool valid = c == c;
    int rank = 0;
    if (valid)
      for (int q = 0; q < i; ++q) rank += dcls[q] == c ? 1 : 0;
    p.keys[o] = coco_key(valid ? (u32)c : (u32)p.C, p.scores[o]);
    p.rank[o] = rank;
#pragma unroll
    for (int a = 0; a < SSDK_COCOEVAL_MAX_A; ++a)
      if (a < p.A) p.flags[o * p.A + a] = flags[i][a];
  }
}

// records sorted by key; seg[c] .. seg[c+1] is class c; flags [n, A], rank [n].  out index ((a * M + m) * T + t) * C + c.
__global__ __launch_bounds__(64) void cocoeval_accumulate_kernel(const int* flags, const int* rank, const long long* seg,
                                                                 const int* npig, int C, int T, int A, int M, const CocoMaxDets md,
                                                                 double* ap, double* recall) {
  const int c = (int)blockIdx.x, t = (int)blockIdx.y, a = (int)blockIdx.z / M, m = (int)blockIdx.z % M;
  const u32 lane = threadIdx.x;
  int maxd = 0;
#pragma unroll
  for (int k = 0; k < SSDK_COCOEVAL_MAX_M; ++k)
    if (k == m) maxd = md.v[k];
  const long long s0 = seg[c], n = seg[c + 1] - seg[c];
  const int np = npig[(size_t)a * C + c];
  const size_t out = (((size_t)a * M + m) * T + t) * C + c;
  if (np == 0) {
    if (lane == 0) {
      ap[out] = __builtin_nan("");
      recall[out] = __builtin_nan("");
    }
    return;
  }
  const int* f = flags + (size_t)s0 * A + a;
  const int* rk = rank + s0;
  auto counts = [f, rk, A, t, maxd](long long j) { return rk[j] < maxd && ((f[j * A] >> (16 + t)) & 1) == 0; };
  auto is_tp = [f, A, t](long long j) { return ((f[j * A] >> t) & 1) != 0; };
  const double acc = map_envelope_sum(n, lane, is_tp, counts, MapCocoWeight{(double)np}) / 101.0;
  long long tp = 0;
  for (long long j = 0; j < n; j += 64) {
    const bool hit = (j + lane < n) && counts(j + lane) && is_tp(j + lane);
    tp += __popcll(__ballot(hit));
  }
  if (lane == 0) {
    ap[out] = acc;
    recall[out] = (double)tp / (double)np;
  }
}

}  // namespace ssdk

extern "C" int ssdk_cocoeval_match(const float* scores, const float* boxes, const float* classes, int B, int D,
                                   const float* targets, int G, const int* gt_crowd, const float* gt_area,
                                   const float* area_scale, int num_classes, float conf_threshold, const float* iou_thresholds,
                                   int T, const float* area_ranges, int A, long long* keys, int* rank, int* flags, int* npig,
                                   void* stream) {
  using namespace ssdk;
  if (!scores || !boxes || !classes || !targets || !iou_thresholds || !area_ranges || !keys || !rank || !flags || !npig) {
    set_error("cocoeval_match: null pointer");
    return SSDK_E_BADARG;
  }
  if (B < 1 || D < 1 || D > kCocoSlots || G < 0 || G > SSDK_MAX_GT || num_classes < 1) {
    set_error("cocoeval_match: bad dims B=%d D=%d (<=%d) G=%d (<=%d) classes=%d", B, D, kCocoSlots, G, SSDK_MAX_GT, num_classes);
    return SSDK_E_BADARG;
  }
  if (T < 1 || T > SSDK_COCOEVAL_MAX_T) {
    set_error("cocoeval_match: T=%d IoU thresholds (1 .. %d)", T, SSDK_COCOEVAL_MAX_T);
    return SSDK_E_BADARG;
  }
  for (int t = 0; t < T; ++t) {
    const float v = iou_thresholds[t];
    if (!(v > 0.f && v <= 1.f) || (t > 0 && !(v > iou_thresholds[t - 1]))) {
      set_error("cocoeval_match: iou_thresholds[%d] = %g: the thresholds must lie in (0, 1] and ascend strictly", t, (double)v);
      return SSDK_E_BADARG;
    }
  }
  if (A < 1 || A > SSDK_COCOEVAL_MAX_A) {
    set_error("cocoeval_match: A=%d area ranges (1 .. %d)", A, SSDK_COCOEVAL_MAX_A);
    return SSDK_E_BADARG;
  }
  for (int a = 0; a < A; ++a) {
    const float lo = area_ranges[2 * a], hi = area_ranges[2 * a + 1];
    if (!(lo <= hi)) {
      set_error("cocoeval_match: area_ranges[%d] = (%g, %g): lo <= hi, neither NaN", a, (double)lo, (double)hi);
      return SSDK_E_BADARG;
    }
  }
  CocoParams p;
  p.scores = scores;
  p.boxes = boxes;
  p.classes = classes;
  p.targets = targets;
  p.gt_crowd = gt_crowd;
  p.gt_area = gt_area;
  p.area_scale = area_scale;
  p.D = D;
  p.G = G;
  p.C = num_classes;
  p.T = T;
  p.A = A;
  p.conf_thr = conf_threshold;
  for (int t = 0; t < SSDK_COCOEVAL_MAX_T; ++t) p.thr[t] = t < T ? iou_thresholds[t] : 2.f;
  for (int a = 0; a < SSDK_COCOEVAL_MAX_A; ++a) {
    p.rng[2 * a] = a < A ? area_ranges[2 * a] : 0.f;
    p.rng[2 * a + 1] = a < A ? area_ranges[2 * a + 1] : 0.f;
  }
  p.keys = keys;
  p.rank = rank;
  p.flags = flags;
  p.npig = npig;
  hipLaunchKernelGGL(cocoeval_match_kernel, dim3((unsigned)B), dim3(kMapThreads), 0, (hipStream_t)stream, p);
  return check_launch("cocoeval_match_kernel");
}

extern "C" int ssdk_cocoeval_accumulate(const int* flags_sorted, const int* rank_sorted, const long long* seg_offsets,
                                        const int* npig, int num_classes, int T, int A, const int* max_dets, int M, double* ap,
                                        double* recall, void* stream) {
  using namespace ssdk;
  if (!flags_sorted || !rank_sorted || !seg_offsets || !npig || !max_dets || !ap || !recall) {
    set_error("cocoeval_accumulate: null pointer");
    return SSDK_E_BADARG;
  }
  if (num_classes < 1 || T < 1 || T > SSDK_COCOEVAL_MAX_T || A < 1 || A > SSDK_COCOEVAL_MAX_A || M < 1 || M > SSDK_COCOEVAL_MAX_M) {
    set_error("cocoeval_accumulate: classes=%d T=%d (1 .. %d) A=%d (1 .. %d) M=%d (1 .. %d)", num_classes, T, SSDK_COCOEVAL_MAX_T, A,
              SSDK_COCOEVAL_MAX_A, M, SSDK_COCOEVAL_MAX_M);
    return SSDK_E_BADARG;
  }
  CocoMaxDets md;
  for (int m = 0; m < SSDK_COCOEVAL_MAX_M; ++m) md.v[m] = 0;
  for (int m = 0; m < M; ++m) {
    if (max_dets[m] < 1 || (m > 0 && max_dets[m] < max_dets[m - 1])) {
      set_error("cocoeval_accumulate: max_dets[%d] = %d: the values must be >= 1 and ascend", m, max_dets[m]);
      return SSDK_E_BADARG;
    }
    md.v[m] = max_dets[m];
  }
  hipLaunchKernelGGL(cocoeval_accumulate_kernel, dim3((unsigned)num_classes, (unsigned)T, (unsigned)(A * M)), dim3(64), 0,
                     (hipStream_t)stream, flags_sorted, rank_sorted, seg_offsets, npig, num_classes, T, A, M, md, ap, recall);
  return check_launch("cocoeval_accumulate_kernel");
}
