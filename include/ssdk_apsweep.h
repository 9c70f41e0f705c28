/*
 * ssdk_apsweep.h -- C-ABI of the average-precision sweep over several IoU thresholds (csrc/ssdk_apsweep.hip), part of
 * libssdk.so: the bookkeeping behind AP@[.50:.95] of an eval epoch.
 *
 * A header of its own next to ssdk.h, like ssdk_cat.h and ssdk_convt.h: the entry points of ssdk.h are a closed list under
 * SSDK_VERSION 245, and this addition changes neither.  Conventions (pointers, streams, return values, ssdk_last_error) are those
 * of ssdk.h.
 *
 * Both entry points share the argument contract of ssdk_map_match / ssdk_map_average_precision (ssdk.h), of which they are the
 * many-threshold form: fp32 detections as the decoder returns them (scores [B, D], boxes [B, D, 4] ltrb, classes [B, D]), targets
 * [B, G, 5] = ltrb + label with label < 0 as padding, D <= 2048, G <= SSDK_MAX_GT, IoU in fp32 in the operation order of
 * ssdk_map_match (the two share one device function).  Each call is ONE launch: no allocation, no workspace, no synchronisation,
 * hipGraph-capturable.  The only atomics are integer ones (LDS minima, the ground-truth counts), so the results do not depend on
 * scheduling and are bit-reproducible.  Every argument error is SSDK_E_BADARG with a message, before any device call.
 */
#ifndef SSDK_APSWEEP_H_
#define SSDK_APSWEEP_H_

#include "ssdk.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the most IoU thresholds one launch takes: a true-positive mask has one bit per threshold */
#define SSDK_APSWEEP_MAX_T 16

/* How a detection becomes a true positive.
 *   SSDK_AP_RULE_REFERENCE  the rule of the reference's MeanAveragePrecision (ssdk_map_match) at every threshold: a detection with
 *                           score > conf_threshold looks only at the same-class ground-truth box of highest IoU (first maximum;
 *                           this does not depend on the threshold).  At threshold t it is a true positive iff that IoU >= t and no
 *                           detection of lower index reaches t on the same box.  max_dets is ignored.  With T = 1 the keys, flags
 *                           and counts are the bits ssdk_map_match writes.
 *   SSDK_AP_RULE_COCO       the greedy rule of pycocotools' evaluateImg for one area range without ignore regions (crowd boxes,
 *                           area ranges, maxDets per category and recall: ssdk_cocoeval.h).
 *                           The caller passes each image's detections in descending score order.  Only the first max_dets valid
 *                           detections of an image (score > conf_threshold, 0 <= class < num_classes) count; the others get the
 *                           sentinel key like padding.  Per class and threshold independently the class's detections are walked in
 *                           order: a detection takes, among the same-class boxes not yet taken at this threshold, the one of
 *                           highest IoU >= t -- among equal IoUs the box of HIGHEST index, which is what the `<` in pycocotools'
 *                           loop amounts to -- and is a true positive; the box is then taken.  Otherwise it is a false positive. */
enum { SSDK_AP_RULE_REFERENCE = 0, SSDK_AP_RULE_COCO = 1 };

/* One launch per batch, one workgroup per image.
 *   iou_thresholds  HOST pointer: T values, strictly ascending, in (0, 1]; copied into the kernel arguments.
 *   keys [B, D]     exactly as ssdk_map_match writes them: (class << 32) | ~ordered(score), class = num_classes for a slot that
 *                   does not count, so that it sorts behind every class.
 *   tp_mask [B, D]  bit t set = true positive at iou_thresholds[t]; every slot is written.
 *   npos [C]        ground-truth boxes per class, ACCUMULATED (zero it before an epoch), exactly as ssdk_map_match. */
int ssdk_apsweep_match(const float* scores, const float* boxes, const float* classes, int B, int D,
                       const float* targets, int G, int num_classes, float conf_threshold,
                       const float* iou_thresholds, int T, int rule, int max_dets,
                       long long* keys, int* tp_mask, int* npos, void* stream);

/* Once per epoch: the records sorted by key (stable), seg_offsets [C + 1] the start of every class among them.  Grid (class,
 * threshold), one wave each, fp64; precision at rank n is tp / n exactly.
 *   ap [T * C]  ap[t * num_classes + c]; NaN where npos[c] == 0, 0 for a class with ground truth and no detections.
 *   SSDK_AP_RULE_REFERENCE  the VOC area of ssdk_map_average_precision (one shared body; with T = 1 the same bits).
 *   SSDK_AP_RULE_COCO       101-point interpolation: ap = mean_k q_k, q_k = the right-to-left running maximum of the precision at
 *                           the first rank whose recall tp / npos is >= r_k, or 0 if there is none; r_k = k * 0.01 in fp64 with
 *                           r_100 = 1.0, the values numpy.linspace(0.0, 1.0, 101) holds.  pycocotools divides by
 *                           tp + fp + numpy.spacing(1) where this divides by tp + fp: a relative difference of at most 3e-16. */
int ssdk_apsweep_average_precision(const int* tp_mask_sorted, const long long* seg_offsets, const int* npos,
                                   int num_classes, int T, int rule, double* ap, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SSDK_APSWEEP_H_ */
