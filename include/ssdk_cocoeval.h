/*
 * ssdk_cocoeval.h -- C-ABI of the COCO detection summary (csrc/ssdk_cocoeval.hip), part of libssdk.so: pycocotools' evaluateImg
 * and accumulate for boxes -- area ranges, crowd (ignore) regions, maxDets per image and category, recall -- on the device.
 *
 * A header of its own next to ssdk.h, like ssdk_apsweep.h: the entry points of ssdk.h are a closed list under SSDK_VERSION 245,
 * and this addition changes neither.  Conventions (pointers, streams, return values, ssdk_last_error) are those of ssdk.h.
 *
 * The detections and targets are those of ssdk_apsweep_match (ssdk_apsweep.h): fp32 scores [B, D], boxes [B, D, 4] ltrb, classes
 * [B, D], each image's detections in descending score order, targets [B, G, 5] = ltrb + label with label < 0 as padding,
 * D <= 2048, G <= SSDK_MAX_GT.  Each call is ONE launch: no allocation, no workspace, no synchronisation, hipGraph-capturable.
 * The only atomics are integer ones (the ground-truth counts), so the results do not depend on scheduling and are
 * bit-reproducible.  Every argument error is SSDK_E_BADARG with a message, before any device call.
 */
#ifndef SSDK_COCOEVAL_H_
#define SSDK_COCOEVAL_H_

#include "ssdk.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the most IoU thresholds (one matched bit and one ignored bit each in a flag word), area ranges and maxDets values of a call */
#define SSDK_COCOEVAL_MAX_T 16
#define SSDK_COCOEVAL_MAX_A 4
#define SSDK_COCOEVAL_MAX_M 4

/* One launch per batch, one workgroup per image.
 *   iou_thresholds  HOST pointer: T <= 16 values, strictly ascending, in (0, 1]; copied into the kernel arguments.
 *   area_ranges     HOST pointer: A <= 4 pairs (lo, hi), both inclusive, lo <= hi, in source pixels.
 *   gt_crowd [B, G] int32, non-zero = crowd region; NULL: no crowd box.
 *   gt_area  [B, G] fp32, source pixels; NULL: the box area (r - l) * (b - t) times the image's area_scale.
 *   area_scale [B]  fp32, source pixels per network pixel; NULL: 1.  A detection's area is its box area times this value.
 *
 * Per image, class, area range a and threshold t independently the rule is pycocotools' evaluateImg.  A ground-truth box is
 * IGNORED at a if it is crowd or its area is < lo or > hi.  The class's detections are walked in order.  A detection looks at the
 * class's boxes that are not yet taken at (a, t) -- a crowd box can be taken any number of times -- and whose IoU is >= t: it takes
 * the non-ignored one of highest IoU if there is one, else the ignored one of highest IoU; among equal IoUs the box of HIGHEST
 * index (the `<` of pycocotools' loop over boxes sorted non-ignored first, stable).  A matched detection inherits the box's ignore
 * flag; an unmatched detection is ignored iff its own area lies outside the range.  IoU with a crowd box is intersection /
 * detection area; every IoU is fp32 in the operation order of ssdk_map_match and is computed once.  Matching does not depend on
 * maxDets: ssdk_cocoeval_accumulate applies it through `rank`.
 *
 *   keys  [B, D]     exactly as ssdk_apsweep_match writes them: (class << 32) | ~ordered(score), class = num_classes for a slot
 *                    that does not count (score <= conf_threshold or class outside [0, num_classes)).
 *   rank  [B, D]     how many counted detections of the same image and class precede the slot (0 for a slot that does not count):
 *                    pycocotools' dt[0:maxDet] per image and category is rank < maxDet.
 *   flags [B, D, A]  bit t = matched at iou_thresholds[t]; bit 16 + t = ignored at iou_thresholds[t]; 0 for a slot that does not
 *                    count.  Every slot is written.
 *   npig  [A, C]     non-ignored ground-truth boxes per area range and class, ACCUMULATED (zero it before an epoch). */
int ssdk_cocoeval_match(const float* scores, const float* boxes, const float* classes, int B, int D,
                        const float* targets, int G, const int* gt_crowd, const float* gt_area, const float* area_scale,
                        int num_classes, float conf_threshold, const float* iou_thresholds, int T,
                        const float* area_ranges, int A,
                        long long* keys, int* rank, int* flags, int* npig, void* stream);

/* Once per epoch: the records sorted by key (stable; flags [n, A] and rank [n] in that order), seg_offsets [C + 1] the start of
 * every class among them.  Grid (class, threshold, area range x maxDets), one wave each, fp64.
 *   max_dets  HOST pointer: M <= 4 values >= 1, ascending.  A record counts at max_dets[m] iff rank < max_dets[m] and it is not
 *             ignored at (a, t); ignored records are neither true nor false positives.
 *   ap     [A, M, T, C]  101-point interpolation as ssdk_apsweep_average_precision (SSDK_AP_RULE_COCO) over the records that
 *                        count: precision tp / (tp + fp) exactly (pycocotools adds numpy.spacing(1) to the denominator: a relative
 *                        difference of at most 3e-16).
 *   recall [A, M, T, C]  tp / npig after the last record that counts; 0 if none counts.
 * Both are NaN where npig[a, c] == 0. */
int ssdk_cocoeval_accumulate(const int* flags_sorted, const int* rank_sorted, const long long* seg_offsets, const int* npig,
                             int num_classes, int T, int A, const int* max_dets, int M,
                             double* ap, double* recall, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SSDK_COCOEVAL_H_ */
