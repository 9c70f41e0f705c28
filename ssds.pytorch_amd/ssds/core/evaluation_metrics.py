"""VOC-style mean average precision of an eval epoch on the HIP device -- the reference's ``MeanAveragePrecision``
(``ssds/core/evaluation_metrics.py:5-142``, driven by ``pipeline_anchor_basic.py:161-182``) with the same
constructor, ``__call__(detections, targets)`` and ``get_results()`` contract.

The reference loops over images x classes in Python and appends to per-class lists; here a batch is ONE launch
(``ssdk_map_match``) that appends a (sort key, true-positive flag) record per detection slot, and ``get_results`` is
one radix sort of the epoch's records plus one launch (``ssdk_map_average_precision``).  Nothing returns to the host
before ``get_results``.  Tie contract: among same-class boxes of equal IoU the first wins (``argmax`` on CPU);
detections of equal score keep their arrival order (the reference's ``np.argsort(...)[::-1]`` leaves it undefined).
The numpy-2 breakage of the reference (``np.float`` / ``np.NAN``, :90, :126) does not apply.

``AveragePrecisionSweep`` is the same bookkeeping over several IoU thresholds at once (``ssdk_apsweep_match`` /
``ssdk_apsweep_average_precision``, include/ssdk_apsweep.h): the number quoted for COCO-shaped data, AP averaged over IoU
0.50 ... 0.95, under pycocotools' greedy rule -- or the reference's rule at every threshold.  ``CocoSummary`` is the full
twelve-number table of pycocotools for boxes (``ssdk_cocoeval_match`` / ``ssdk_cocoeval_accumulate``, include/ssdk_cocoeval.h):
area ranges, crowd regions, maxDets per image and category, recall.  All classes ``merge()`` their records over the ranks of a
process group at the end of an epoch (``merge_records``)."""
from collections import OrderedDict
import ctypes

import numpy as np
import torch
import torch.distributed as dist

from ssds import _native as N

COCO_IOUS = np.linspace(0.5, 0.95, 10).astype(np.float32)  # 0.50 : 0.05 : 0.95 as the fp32 values the kernel compares with
COCO_AREAS = np.array([[0, 1e10], [0, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e10]], np.float32)  # all, small, medium, large
COCO_MAX_DETS = (1, 10, 100)


def merge_records(keys, tp, npos, group=None, width=1, num_classes=None):
    """The records of every rank of ``group``, on every rank: ``keys`` [n] int64 and ``tp`` [n] (flags or masks) of this rank are
    padded to the longest rank's length with sentinel records (key class = num_classes = ``npos.numel()``, flag 0: they sort
    behind every class, like the padded slots of a batch), all-gathered and concatenated in rank order; ``npos`` [C] is
    sum-reduced.  -> (keys, tp, npos) on the device of ``keys``, identical on all ranks.  The collectives run on the tensors'
    device where the backend can (RCCL), else staged through the host (gloo).  Run it once, at the end of an epoch: it
    synchronises.  ``width`` > 1: ``tp`` is [n, width] (several words per record); ``num_classes``: the sentinel class where it is
    not ``npos.numel()`` (counts of another shape than [C]).

    The result equals a one-process evaluation of the same images whenever no two detections of a class have equal scores:
    records of equal key keep their arrival order under the stable sort, and that order becomes rank-major here."""
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
        return keys, tp, npos
    world, dev = dist.get_world_size(group), keys.device
    on_device = keys.is_cuda and dist.get_backend(group) == "nccl"
    if not on_device:
        keys, tp, npos = keys.cpu(), tp.cpu(), npos.cpu()
    keys, tp, npos = keys.contiguous().view(-1), tp.contiguous().view(-1), npos.clone()
    if width > 1:
        tp = tp.view(-1, width)
    n = torch.tensor([keys.numel()], dtype=torch.int64, device=keys.device)
    counts = [torch.zeros_like(n) for _ in range(world)]
    dist.all_gather(counts, n, group=group)
    longest = max(int(c) for c in counts)
    sentinel = (int(npos.numel() if num_classes is None else num_classes) << 32) | 0xFFFFFFFF
    pk = torch.full((longest,), sentinel, dtype=torch.int64, device=keys.device)
    pt = torch.zeros((longest,) + tuple(tp.shape[1:]), dtype=tp.dtype, device=keys.device)
    pk[:keys.numel()] = keys
    pt[:tp.shape[0]] = tp
    all_k = [torch.empty_like(pk) for _ in range(world)]
    all_t = [torch.empty_like(pt) for _ in range(world)]
    dist.all_gather(all_k, pk, group=group)
    dist.all_gather(all_t, pt, group=group)
    dist.all_reduce(npos, op=dist.ReduceOp.SUM, group=group)
    return torch.cat(all_k).to(dev), torch.cat(all_t).to(dev), npos.to(dev)


def _merge_into(metric, tp_dtype, group, width=1, counts_shape=None):
    """``merge()`` of the metric classes: this rank's records replaced by those of all ranks.  A rank that saw no batch joins
    the collectives with no records.  ``width`` words per record; ``counts_shape``: that of the counts where it is not [C]."""
    if metric._npos is None:
        dev = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
        metric._npos = torch.zeros(counts_shape or metric.num_classes, device=dev, dtype=torch.int32)
    dev = metric._npos.device
    keys = torch.cat(metric._keys) if metric._keys else torch.empty(0, dtype=torch.int64, device=dev)
    tp = torch.cat(metric._tp) if metric._tp else torch.empty((0,) if width == 1 else (0, width), dtype=tp_dtype, device=dev)
    keys, tp, metric._npos = merge_records(keys, tp, metric._npos, group, width, metric.num_classes)
    metric._keys, metric._tp = [keys], [tp]


def _sort_records(keys, tp, num_classes):
    """One stable radix sort of an epoch's records -> (sorted keys, tp in that order, the start of every class [C + 1])."""
    skeys, order = torch.sort(keys, stable=True)  # rocPRIM radix sort
    bounds = torch.arange(num_classes + 1, device=keys.device, dtype=torch.int64) << 32
    return skeys, tp[order].contiguous(), torch.searchsorted(skeys, bounds).contiguous()


class MeanAveragePrecision(object):
    def __init__(self, num_classes, conf_threshold, iou_threshold):
        self.num_classes = int(num_classes)
        self.conf_threshold = float(conf_threshold)
        self.iou_threshold = float(iou_threshold)
        self._keys, self._tp = [], []
        self._npos = None

    def __call__(self, detections, targets):
        """detections = (scores [B,D], boxes [B,D,4] ltrb, classes [B,D]) as returned by ``Decoder``; targets
        [B,G,5] = ltrb + label (-1 padding).  Appends this batch's records; no host synchronisation."""
        scores, boxes, classes = detections
        N.require_device(scores, "MeanAveragePrecision")
        dev = scores.device
        scores, boxes, classes = (x.contiguous().float() for x in (scores, boxes, classes))
        t = targets.to(dev).contiguous().float()
        B, D = int(scores.shape[0]), int(scores.shape[1])
        G = int(t.shape[1])
        if self._npos is None:
            self._npos = torch.zeros(self.num_classes, device=dev, dtype=torch.int32)
        keys = torch.empty((B, D), device=dev, dtype=torch.int64)
        tp = torch.empty((B, D), device=dev, dtype=torch.uint8)
        with torch.cuda.device(dev):
            rc = N.lib.ssdk_map_match(scores.data_ptr(), boxes.data_ptr(), classes.data_ptr(), B, D, t.data_ptr(), G,
                                      self.num_classes, self.conf_threshold, self.iou_threshold, keys.data_ptr(),
                                      tp.data_ptr(), self._npos.data_ptr(), N.stream_ptr(dev))
        N.check(rc, "map_match")
        self._keys.append(keys.view(-1))
        self._tp.append(tp.view(-1))

    def _sorted(self):
        keys, tp = torch.cat(self._keys), torch.cat(self._tp)
        skeys, order = torch.sort(keys, stable=True)  # rocPRIM radix sort
        bounds = torch.arange(self.num_classes + 1, device=keys.device, dtype=torch.int64) << 32
        seg = torch.searchsorted(skeys, bounds).contiguous()
        return skeys, tp[order].contiguous(), seg

    def get_results(self):
        """(mAP, (precision, recall, ap)) like the reference: ap[c] is NaN for a class without ground truth, mAP
        the mean over the others; precision / recall are per-class numpy arrays for PR curves."""
        C = self.num_classes
        if self._npos is None:
            return float("nan"), ([[0], [0]] * C, [[0], [1]] * C, [float("nan")] * C)
        dev = self._npos.device
        skeys, tp, seg = self._sorted()
        ap = torch.empty(C, device=dev, dtype=torch.float64)
        with torch.cuda.device(dev):
            rc = N.lib.ssdk_map_average_precision(tp.data_ptr(), seg.data_ptr(), self._npos.data_ptr(), C,
                                                  ap.data_ptr(), N.stream_ptr(dev))
        N.check(rc, "map_average_precision")
        mAP = float(torch.nanmean(ap)) if bool((self._npos > 0).any()) else float("nan")
        ap_h, npos_h, seg_h, tp_h = ap.cpu().numpy(), self._npos.cpu().numpy(), seg.cpu().numpy(), tp.cpu().numpy()
        recall, precision = [], []
        for c in range(C):  # PR-curve arrays for the caller's plots (evaluation_metrics.py:124-140)
            if npos_h[c] == 0:
                recall += [[0], [1]]
                precision += [[0], [0]]
                continue
            cum = np.cumsum(tp_h[seg_h[c]:seg_h[c + 1]].astype(np.int64))
            recall.append(cum.astype(float) / float(npos_h[c]))
            precision.append(cum.astype(float) / np.arange(1, len(cum) + 1, dtype=float))
        return mAP, (precision, recall, ap_h.tolist())

    def merge(self, group=None):
        """End of an epoch under data parallelism: afterwards every rank holds the records of all ranks (``merge_records``;
        equal to a one-process evaluation whenever no two detections of a class have equal scores)."""
        _merge_into(self, torch.uint8, group)

    def records(self):
        """Per class, in arrival order: (scores, detect_ismatched) and the ground-truth counts -- the reference's
        ``self.score`` / ``self.detect_ismatched`` / ``self.npos`` (:10-13), for tests."""
        keys, tp = torch.cat(self._keys).cpu().numpy(), torch.cat(self._tp).cpu().numpy().astype(bool)
        cls = (keys >> 32).astype(np.int64)
        u = (~keys & 0xFFFFFFFF).astype(np.uint32)
        bits = np.where(u & 0x80000000, u & 0x7FFFFFFF, ~u).astype(np.uint32)
        score = bits.view(np.float32)
        return ([score[cls == c] for c in range(self.num_classes)], [tp[cls == c] for c in range(self.num_classes)],
                self._npos.cpu().numpy())


class AveragePrecisionSweep(object):
    """Average precision at every threshold of ``iou_thresholds`` (strictly ascending, in (0, 1], at most ``N.APSWEEP_MAX_T``)
    from ONE launch per batch and one sort + one launch per epoch.  ``rule``: "coco" -- pycocotools' greedy matching (per class
    and threshold a detection takes the free box of highest IoU >= t; only the first ``max_dets`` detections of an image by
    score count) and 101-point interpolation (crowd regions, area ranges and recall: ``CocoSummary``); "reference" -- the rule and the
    VOC area of ``MeanAveragePrecision`` at every threshold (``max_dets`` is ignored).  Same ``__call__`` contract as
    ``MeanAveragePrecision``; nothing returns to the host before ``get_results``."""

    def __init__(self, num_classes, conf_threshold, iou_thresholds=COCO_IOUS, rule="coco", max_dets=100):
        if rule not in N.AP_RULE:
            raise ValueError("AveragePrecisionSweep: rule {!r} (one of {})".format(rule, sorted(N.AP_RULE)))
        self.num_classes = int(num_classes)
        self.conf_threshold = float(conf_threshold)
        self.iou_thresholds = np.asarray(iou_thresholds, dtype=np.float32).reshape(-1)
        self.rule, self.max_dets = rule, int(max_dets)
        self._thr = (ctypes.c_float * max(len(self.iou_thresholds), 1))(*[float(v) for v in self.iou_thresholds])
        self._keys, self._tp = [], []
        self._npos = None

    def __call__(self, detections, targets):
        """detections = (scores [B,D], boxes [B,D,4] ltrb, classes [B,D]) as returned by ``Decoder``; targets [B,G,5] = ltrb +
        label (-1 padding).  Appends this batch's records; no host synchronisation.  Under the COCO rule every image's
        detections are put into descending score order first (stable: a ``Decoder`` output stays as it is)."""
        scores, boxes, classes = detections
        N.require_device(scores, "AveragePrecisionSweep")
        dev = scores.device
        scores, boxes, classes = (x.contiguous().float() for x in (scores, boxes, classes))
        if self.rule == "coco":
            scores, order = torch.sort(scores, dim=1, descending=True, stable=True)
            classes = torch.gather(classes, 1, order)
            boxes = torch.gather(boxes, 1, order.unsqueeze(-1).expand(-1, -1, 4)).contiguous()
        t = targets.to(dev).contiguous().float()
        B, D = int(scores.shape[0]), int(scores.shape[1])
        if t.shape[1] == 0:  # a batch without any box: one padding row, so that the pointer is one
            t = t.new_full((B, 1, 5), -1.0)
        G = int(t.shape[1])
        if self._npos is None:
            self._npos = torch.zeros(self.num_classes, device=dev, dtype=torch.int32)
        keys = torch.empty((B, D), device=dev, dtype=torch.int64)
        tp = torch.empty((B, D), device=dev, dtype=torch.int32)
        with torch.cuda.device(dev):
            rc = N.lib.ssdk_apsweep_match(scores.data_ptr(), boxes.data_ptr(), classes.data_ptr(), B, D, t.data_ptr(), G,
                                          self.num_classes, self.conf_threshold, self._thr, len(self.iou_thresholds),
                                          N.AP_RULE[self.rule], self.max_dets, keys.data_ptr(), tp.data_ptr(),
                                          self._npos.data_ptr(), N.stream_ptr(dev))
        N.check(rc, "apsweep_match")
        self._keys.append(keys.view(-1))
        self._tp.append(tp.view(-1))

    def merge(self, group=None):
        """End of an epoch under data parallelism: afterwards every rank holds the records of all ranks (``merge_records``;
        equal to a one-process evaluation whenever no two detections of a class have equal scores)."""
        _merge_into(self, torch.int32, group)

    def average_precision(self):
        """ap [T, C] fp64 on the device (NaN: a class without ground truth): one sort and one launch."""
        dev = self._npos.device
        _, tp, seg = _sort_records(torch.cat(self._keys), torch.cat(self._tp), self.num_classes)
        T, C = len(self.iou_thresholds), self.num_classes
        ap = torch.empty((T, C), device=dev, dtype=torch.float64)
        with torch.cuda.device(dev):
            rc = N.lib.ssdk_apsweep_average_precision(tp.data_ptr(), seg.data_ptr(), self._npos.data_ptr(), C, T,
                                                      N.AP_RULE[self.rule], ap.data_ptr(), N.stream_ptr(dev))
        N.check(rc, "apsweep_average_precision")
        return ap

    def get_results(self):
        """(mAP, detail): mAP = the mean of the non-NaN entries of ap[T, C] (AP@[.50:.95] with the default thresholds);
        detail = {"iou_thresholds" [T], "ap" numpy [T, C] (NaN: a class without ground truth), "mAP_per_iou" [T]}."""
        T, C = len(self.iou_thresholds), self.num_classes
        if self._npos is None or not self._keys:
            ap = np.full((T, C), np.nan)
        else:
            ap = self.average_precision().cpu().numpy()
        have = ~np.isnan(ap)
        per_iou = np.array([ap[t][have[t]].mean() if have[t].any() else np.nan for t in range(T)])
        mAP = float(ap[have].mean()) if have.any() else float("nan")
        return mAP, {"iou_thresholds": self.iou_thresholds.copy(), "ap": ap, "mAP_per_iou": per_iou}

    def records(self):
        """(key class [n] with num_classes where a slot does not count, scores [n], masks [n], npos [C]) in arrival order, as
        numpy -- for tests."""
        keys = torch.cat(self._keys).cpu().numpy()
        u = (~keys & 0xFFFFFFFF).astype(np.uint32)
        bits = np.where(u & 0x80000000, u & 0x7FFFFFFF, ~u).astype(np.uint32)
        return (keys >> 32).astype(np.int64), bits.view(np.float32), torch.cat(self._tp).cpu().numpy(), self._npos.cpu().numpy()


class CocoSummary(object):
    """The twelve numbers pycocotools prints for boxes -- AP, AP50, AP75, APs, APm, APl, AR1, AR10, AR100, ARs, ARm, ARl -- from ONE
    launch per batch (``ssdk_cocoeval_match``) and one sort + one launch per epoch (``ssdk_cocoeval_accumulate``).  The rule is
    pycocotools' ``evaluateImg`` / ``accumulate``: per (image, category, area range, threshold) greedy matching in score order with
    ignored boxes (crowd, or an area outside the range) behind the others, a crowd box taken any number of times, IoU against a
    crowd box = intersection / detection area; maxDets per image AND category; 101-point interpolation.  Deviations: IoU in fp32,
    no ``np.spacing(1)`` in the precision denominator, and the box area where no ``area`` is supplied.  Segmentation and
    keypoints are not evaluated.  Same life cycle as ``AveragePrecisionSweep``; nothing returns to the host before
    ``get_results``."""

    takes_extras = True  # eval_anchor_based_epoch: crowd, area and area_scale of a batch are passed as keywords

    def __init__(self, num_classes, conf_threshold, iou_thresholds=COCO_IOUS, area_ranges=COCO_AREAS, max_dets=COCO_MAX_DETS):
        self.num_classes = int(num_classes)
        self.conf_threshold = float(conf_threshold)
        self.iou_thresholds = np.asarray(iou_thresholds, dtype=np.float32).reshape(-1)
        self.area_ranges = np.asarray(area_ranges, dtype=np.float32).reshape(-1, 2)
        self.max_dets = tuple(int(m) for m in max_dets)
        self._thr = (ctypes.c_float * max(len(self.iou_thresholds), 1))(*[float(v) for v in self.iou_thresholds])
        self._rng = (ctypes.c_float * max(self.area_ranges.size, 2))(*[float(v) for v in self.area_ranges.reshape(-1)])
        self._md = (ctypes.c_int * max(len(self.max_dets), 1))(*self.max_dets)
        self._keys, self._tp = [], []  # a record: its key and [rank, flags of every area range] as int32
        self._npos = None              # [A, C] non-ignored boxes

    def __call__(self, detections, targets, crowd=None, area=None, area_scale=None):
        """detections = (scores [B,D], boxes [B,D,4] ltrb, classes [B,D]) as returned by ``Decoder``; targets [B,G,5] = ltrb +
        label (-1 padding); crowd [B,G] (non-zero = crowd region), area [B,G] (source pixels) and area_scale [B] (source pixels
        per network pixel) are optional.  Every image's detections are put into descending score order first (stable).  Appends
        this batch's records; no host synchronisation."""
        scores, boxes, classes = detections
        N.require_device(scores, "CocoSummary")
        dev = scores.device
        scores, boxes, classes = (x.contiguous().float() for x in (scores, boxes, classes))
        scores, order = torch.sort(scores, dim=1, descending=True, stable=True)
        classes = torch.gather(classes, 1, order)
        boxes = torch.gather(boxes, 1, order.unsqueeze(-1).expand(-1, -1, 4)).contiguous()
        t = targets.to(dev).contiguous().float()
        B, D = int(scores.shape[0]), int(scores.shape[1])
        if t.shape[1] == 0:  # a batch without any box: one padding row, so that the pointer is one
            t, crowd, area = t.new_full((B, 1, 5), -1.0), None, None
        G, A = int(t.shape[1]), len(self.area_ranges)
        crowd = None if crowd is None else crowd.to(dev).to(torch.int32).contiguous()
        area = None if area is None else area.to(dev).float().contiguous()
        area_scale = None if area_scale is None else area_scale.to(dev).float().contiguous()
        for name, x, shape in (("crowd", crowd, (B, G)), ("area", area, (B, G)), ("area_scale", area_scale, (B,))):
            if x is not None and tuple(x.shape) != shape:
                raise ValueError("CocoSummary: {} has shape {}, expected {}".format(name, tuple(x.shape), shape))
        if self._npos is None:
            self._npos = torch.zeros((A, self.num_classes), device=dev, dtype=torch.int32)
        keys = torch.empty((B, D), device=dev, dtype=torch.int64)
        rec = torch.empty((1 + A, B, D), device=dev, dtype=torch.int32)  # the launch writes rank [B, D] and flags [B, D, A]
        rank, flags = rec[0], rec[1:].view(B, D, A)
        with torch.cuda.device(dev):
            rc = N.lib.ssdk_cocoeval_match(scores.data_ptr(), boxes.data_ptr(), classes.data_ptr(), B, D, t.data_ptr(), G,
                                           None if crowd is None else crowd.data_ptr(), None if area is None else area.data_ptr(),
                                           None if area_scale is None else area_scale.data_ptr(), self.num_classes,
                                           self.conf_threshold, self._thr, len(self.iou_thresholds), self._rng, A,
                                           keys.data_ptr(), rank.data_ptr(), flags.data_ptr(), self._npos.data_ptr(),
                                           N.stream_ptr(dev))
        N.check(rc, "cocoeval_match")
        self._keys.append(keys.view(-1))
        self._tp.append(torch.cat([rank.reshape(-1, 1), flags.reshape(-1, A)], dim=1))

    def merge(self, group=None):
        """End of an epoch under data parallelism: afterwards every rank holds the records of all ranks (``merge_records``;
        equal to a one-process evaluation whenever no two detections of a class have equal scores)."""
        A = len(self.area_ranges)
        _merge_into(self, torch.int32, group, 1 + A, (A, self.num_classes))

    def accumulate(self):
        """(ap, recall), each [A, M, T, C] fp64 on the device (NaN: no non-ignored box of the class in the range): one sort and
        one launch."""
        dev = self._npos.device
        A, M, T, C = len(self.area_ranges), len(self.max_dets), len(self.iou_thresholds), self.num_classes
        keys, rec = torch.cat(self._keys), torch.cat(self._tp)
        skeys, order = torch.sort(keys, stable=True)  # rocPRIM radix sort
        bounds = torch.arange(C + 1, device=dev, dtype=torch.int64) << 32
        seg = torch.searchsorted(skeys, bounds).contiguous()
        rec = rec[order]
        rank, flags = rec[:, 0].contiguous(), rec[:, 1:].contiguous()
        out = torch.empty((2, A, M, T, C), device=dev, dtype=torch.float64)
        with torch.cuda.device(dev):
            rc = N.lib.ssdk_cocoeval_accumulate(flags.data_ptr(), rank.data_ptr(), seg.data_ptr(), self._npos.data_ptr(), C, T, A,
                                                self._md, M, out[0].data_ptr(), out[1].data_ptr(), N.stream_ptr(dev))
        N.check(rc, "cocoeval_accumulate")
        return out[0], out[1]

    @staticmethod
    def _mean(x):
        x = np.asarray(x, np.float64)
        x = x[~np.isnan(x)]
        return float(x.mean()) if x.size else float("nan")

    def get_results(self):
        """(AP, detail): detail = {"summary": the twelve numbers in pycocotools' order, each the mean over the non-NaN entries of
        the slice ``summarize`` takes, "ap" and "recall": numpy [A, M, T, C], "iou_thresholds", "area_ranges", "max_dets"}.  The
        summary reads area range 0 as "all" and 1 .. 3 as small / medium / large, the LAST maxDets for AP and ARs / ARm / ARl, and
        maxDets 0 .. 2 for AR1 / AR10 / AR100 (the defaults are COCO's); a number whose slice does not exist is NaN."""
        A, M, T, C = len(self.area_ranges), len(self.max_dets), len(self.iou_thresholds), self.num_classes
        if self._npos is None or not self._keys:
            ap, recall = np.full((A, M, T, C), np.nan), np.full((A, M, T, C), np.nan)
        else:
            ap, recall = (x.cpu().numpy() for x in self.accumulate())
        thr = self.iou_thresholds
        last = M - 1
        s = OrderedDict()
        s["AP"] = self._mean(ap[0, last])
        s["AP50"] = self._mean(ap[0, last][thr == np.float32(0.5)])
        s["AP75"] = self._mean(ap[0, last][thr == np.float32(0.75)])
        for name, a in (("APs", 1), ("APm", 2), ("APl", 3)):
            s[name] = self._mean(ap[a, last]) if a < A else float("nan")
        for m, name in enumerate(("AR1", "AR10", "AR100")):
            s[name] = self._mean(recall[0, m]) if m < M else float("nan")
        for name, a in (("ARs", 1), ("ARm", 2), ("ARl", 3)):
            s[name] = self._mean(recall[a, last]) if a < A else float("nan")
        return s["AP"], {"summary": s, "ap": ap, "recall": recall, "iou_thresholds": thr.copy(),
                         "area_ranges": self.area_ranges.copy(), "max_dets": self.max_dets}

    def records(self):
        """(key class [n], scores [n], rank [n], flags [n, A], npig [A, C]) in arrival order, as numpy -- for tests."""
        keys = torch.cat(self._keys).cpu().numpy()
        rec = torch.cat(self._tp).cpu().numpy()
        u = (~keys & 0xFFFFFFFF).astype(np.uint32)
        bits = np.where(u & 0x80000000, u & 0x7FFFFFFF, ~u).astype(np.uint32)
        return (keys >> 32).astype(np.int64), bits.view(np.float32), rec[:, 0], rec[:, 1:], self._npos.cpu().numpy()
