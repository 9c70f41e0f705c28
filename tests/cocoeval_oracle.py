"""CPU oracle of the COCO detection summary (include/ssdk_cocoeval.h, ssds.core.evaluation_metrics.CocoSummary).

TEST INFRASTRUCTURE ONLY.  A numpy restatement of pycocotools' ``COCOeval`` for boxes, written like pycocotools and unlike the
kernel: ``evaluate_img`` per (image, category, area range) with the boxes argsorted ignore-last by mergesort and the ``for d`` /
``for g`` loops with their ``continue`` / ``break``; ``accumulate`` over the per-image results cut to ``dt[0:maxDet]`` with
``tps = dtm & ~dtIg``, cumulative sums and ``searchsorted``; ``summarize`` with the twelve slices.  IoU is fp32 in the reference's
operation order (``oracle.map_oracle.matrix_iou``), against a crowd box intersection / detection area; thresholds and areas are
compared in fp32; precision and recall in fp64 with pycocotools' ``np.spacing(1)`` in the precision denominator.

``COUNTERS`` of an ``evaluate`` call say how often each branch of the rule fired, so that a test can tell whether its inputs
reach them.  The seeded generator redraws a detection until no IoU lies within the margin of a threshold, no area lies within a
relative 1e-4 of 32^2 or 96^2 and every detection area is > 0, and draws the scores from a permutation; ``conditions`` checks all
four on what the generator returned."""
from collections import OrderedDict

import numpy as np

from oracle.map_oracle import matrix_iou

F32 = np.float32
COCO_IOUS = np.linspace(0.5, 0.95, 10).astype(F32)
SWEEP16 = np.linspace(0.2, 0.95, 16).astype(F32)
COCO_AREAS = np.array([[0, 1e10], [0, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e10]], F32)  # all, small, medium, large
COCO_MAX_DETS = (1, 10, 100)
ALL_AREAS = COCO_AREAS[:1]
BRANCHES = ("crowd_retake", "break", "ignored_absorption", "unmatched_out_of_range")


def crowd_iou(a, b):
    """intersection / area of a, the intersection as ``matrix_iou`` computes it."""
    a, b = a.astype(F32), b.astype(F32)
    lt = np.maximum(a[:, None, :2], b[None, :, :2])
    rb = np.minimum(a[:, None, 2:], b[None, :, 2:])
    area_i = (np.prod(rb - lt, axis=2, dtype=F32) * (lt < rb).all(axis=2)).astype(F32)
    area_a = np.prod(a[:, 2:] - a[:, :2], axis=1, dtype=F32)
    with np.errstate(invalid="ignore", divide="ignore"):
        return area_i / area_a[:, None]


def box_area(b, scale):
    """(r - l) * (b - t) * scale in fp32, in that order."""
    b = np.asarray(b, F32)
    return ((b[..., 2] - b[..., 0]) * (b[..., 3] - b[..., 1]) * F32(scale)).astype(F32)


def ious_of(dt_boxes, gt_boxes, iscrowd):
    """[len(dt), len(gt)] fp32: IoU, or intersection / detection area against a crowd box (maskUtils.iou with iscrowd)."""
    iou = matrix_iou(dt_boxes, gt_boxes)
    if len(gt_boxes) and np.any(iscrowd):
        iou = np.where(np.asarray(iscrowd, bool)[None, :], crowd_iou(dt_boxes, gt_boxes), iou).astype(F32)
    return iou


def evaluate_img(dt_boxes, dt_area, gt_boxes, gt_area, gt_crowd, a_rng, thresholds, counters):
    """pycocotools ``evaluateImg`` for one (image, category, area range): detections in descending score order.
    -> (dtm [T, D] bool, dtIg [T, D] bool, gtIg [G] bool in the ORIGINAL box order)."""
    T, D, G = len(thresholds), len(dt_boxes), len(gt_boxes)
    ignore = np.array([bool(gt_crowd[g]) or gt_area[g] < a_rng[0] or gt_area[g] > a_rng[1] for g in range(G)], bool)
    gtind = np.argsort(ignore.astype(np.int64), kind="mergesort")  # non-ignored first, stable
    gtIg = ignore[gtind]
    iscrowd = np.asarray(gt_crowd, bool)[gtind] if G else np.zeros(0, bool)
    ious = ious_of(dt_boxes, gt_boxes, gt_crowd)[:, gtind] if G and D else np.zeros((D, G), F32)
    gtm = np.zeros((T, G), np.int64)
    dtm = np.zeros((T, D), np.int64)
    dtIg = np.zeros((T, D), bool)
    if G and D:
        for tind, t in enumerate(thresholds):
            for dind in range(D):
                iou = F32(t)
                m = -1
                for gind in range(G):
                    # if this gt already matched, and not a crowd, continue
                    if gtm[tind, gind] > 0 and not iscrowd[gind]:
                        continue
                    # if dt matched to reg gt, and on ignore gt, stop
                    if m > -1 and not gtIg[m] and gtIg[gind]:
                        counters["break"] += 1
                        break
                    # continue to next gt unless better match made
                    if ious[dind, gind] < iou:
                        continue
                    # if match successful and best so far, store appropriately
                    iou = ious[dind, gind]
                    m = gind
                if m == -1:
                    continue
                if iscrowd[m] and gtm[tind, m] > 0:
                    counters["crowd_retake"] += 1
                if gtIg[m] and not iscrowd[m]:
                    counters["ignored_absorption"] += 1
                dtIg[tind, dind] = gtIg[m]
                dtm[tind, dind] = gtind[m] + 1
                gtm[tind, m] = dind + 1
    # set unmatched detections outside of area range to ignore
    a = np.array([ar < a_rng[0] or ar > a_rng[1] for ar in dt_area], bool).reshape(1, D)
    unmatched_out = np.logical_and(dtm == 0, np.repeat(a, T, 0))
    counters["unmatched_out_of_range"] += int(unmatched_out.sum())
    dtIg = np.logical_or(dtIg, unmatched_out)
    return dtm > 0, dtIg, ignore


def new_counters():
    return OrderedDict((k, 0) for k in BRANCHES)


def evaluate(detections, targets, num_classes, conf_threshold, thresholds, area_ranges=COCO_AREAS, crowd=None, area=None,
             area_scale=None, counters=None):
    """One batch -> (cls [B, D] with num_classes where a slot does not count, rank [B, D], flags [B, D, A] int32 (bit t matched,
    bit 16 + t ignored), npig [A, C]).  Every image's detections are in descending score order."""
    scores, boxes, classes = (np.asarray(x, F32) for x in detections)
    targets = np.asarray(targets, F32)
    thr, rng = np.asarray(thresholds, F32), np.asarray(area_ranges, F32).reshape(-1, 2)
    counters = new_counters() if counters is None else counters
    B, D = scores.shape
    G, C, A, T = targets.shape[1], num_classes, len(rng), len(thr)
    cls = np.full((B, D), C, np.int64)
    rank = np.zeros((B, D), np.int32)
    flags = np.zeros((B, D, A), np.int64)
    npig = np.zeros((A, C), np.int64)
    for b in range(B):
        scale = F32(1.0) if area_scale is None else F32(area_scale[b])
        s, bx, cl, tg = scores[b], boxes[b], classes[b], targets[b]
        valid = (s > F32(conf_threshold)) & (cl >= 0) & (cl < C)
        cls[b, valid] = cl[valid].astype(np.int64)
        g_crowd = np.zeros(G, bool) if crowd is None else np.asarray(crowd[b]) != 0
        g_area = box_area(tg[:, :4], scale) if area is None else np.asarray(area[b], F32)
        d_area = box_area(bx, scale)
        cats = sorted(set(float(v) for v in tg[:, 4] if 0 <= v < C) | set(float(v) for v in cl[valid]))
        for c in cats:
            rows = np.nonzero(tg[:, 4] == F32(c))[0]
            dets = np.nonzero(valid & (cl == F32(c)))[0]  # dt sorted by score: the image's order
            rank[b, dets] = np.arange(len(dets))
            for a in range(A):
                dtm, dtIg, gtIg = evaluate_img(bx[dets], d_area[dets], tg[rows, :4], g_area[rows], g_crowd[rows], rng[a], thr, counters)
                npig[a, int(c)] += int(np.count_nonzero(~gtIg))
                for t in range(T):
                    flags[b, dets, a] |= (dtm[t].astype(np.int64) << t) | (dtIg[t].astype(np.int64) << (16 + t))
    return cls, rank, flags.astype(np.uint32).view(np.int32).reshape(B, D, A), npig


def accumulate(cls, scores, rank, flags, npig, num_classes, T, max_dets=COCO_MAX_DETS):
    """pycocotools ``accumulate`` over the flattened records of an epoch in arrival order -> (ap [A, M, T, C], recall
    [A, M, T, C]); NaN where pycocotools leaves -1 (no non-ignored box of the category in the range)."""
    cls, scores, rank = np.asarray(cls).ravel(), np.asarray(scores, F32).ravel(), np.asarray(rank).ravel()
    A = npig.shape[0]
    flags = np.asarray(flags).reshape(-1, A).view(np.uint32).astype(np.int64)
    rec_thrs = np.linspace(0.0, 1.0, 101)
    ap = np.full((A, len(max_dets), T, num_classes), np.nan)
    recall = np.full((A, len(max_dets), T, num_classes), np.nan)
    for k in range(num_classes):
        for a in range(A):
            for m, max_det in enumerate(max_dets):
                if npig[a, k] == 0:
                    continue
                sel = np.nonzero((cls == k) & (rank < max_det))[0]  # e['dtScores'][0:maxDet] of every image, concatenated
                inds = np.argsort(-scores[sel].astype(np.float64), kind="mergesort")
                f = flags[sel][inds, a]
                for t in range(T):
                    dtm, dtIg = ((f >> t) & 1).astype(bool), ((f >> (16 + t)) & 1).astype(bool)
                    tps = np.logical_and(dtm, np.logical_not(dtIg))
                    fps = np.logical_and(np.logical_not(dtm), np.logical_not(dtIg))
                    tp = np.cumsum(tps).astype(np.float64)
                    fp = np.cumsum(fps).astype(np.float64)
                    nd = len(tp)
                    rc = tp / npig[a, k]
                    pr = tp / (fp + tp + np.spacing(1))
                    q = np.zeros(101)
                    recall[a, m, t, k] = rc[-1] if nd else 0
                    pr = pr.tolist()
                    for i in range(nd - 1, 0, -1):
                        if pr[i] > pr[i - 1]:
                            pr[i - 1] = pr[i]
                    where = np.searchsorted(rc, rec_thrs, side="left")
                    for ri, pi in enumerate(where):
                        if pi < nd:
                            q[ri] = pr[pi]
                    ap[a, m, t, k] = np.mean(q)
    return ap, recall


def _mean(x):
    x = np.asarray(x, np.float64)
    x = x[~np.isnan(x)]
    return float(x.mean()) if x.size else float("nan")


def summarize(ap, recall, thresholds):
    """The twelve numbers of pycocotools' ``summarize`` (boxes) from ap / recall [4, 3, T, C] over (all, small, medium, large) x
    maxDets (1, 10, 100): each the mean over the entries of its slice that are not NaN (-1 there)."""
    thr = np.asarray(thresholds, F32)
    t50, t75 = (np.nonzero(thr == F32(v))[0] for v in (0.5, 0.75))
    out = OrderedDict()
    out["AP"] = _mean(ap[0, 2])
    out["AP50"] = _mean(ap[0, 2][t50])
    out["AP75"] = _mean(ap[0, 2][t75])
    out["APs"], out["APm"], out["APl"] = (_mean(ap[a, 2]) for a in (1, 2, 3))
    out["AR1"], out["AR10"], out["AR100"] = (_mean(recall[0, m]) for m in (0, 1, 2))
    out["ARs"], out["ARm"], out["ARl"] = (_mean(recall[a, 2]) for a in (1, 2, 3))
    return out


class Summary(object):
    """The oracle with the interface of the device metric."""

    def __init__(self, num_classes, conf_threshold, thresholds=COCO_IOUS, area_ranges=COCO_AREAS, max_dets=COCO_MAX_DETS):
        self.C, self.conf, self.thr = num_classes, conf_threshold, np.asarray(thresholds, F32)
        self.rng, self.max_dets = np.asarray(area_ranges, F32).reshape(-1, 2), tuple(max_dets)
        self.cls, self.scores, self.rank, self.flags = [], [], [], []
        self.npig = np.zeros((len(self.rng), num_classes), np.int64)
        self.counters = new_counters()

    def __call__(self, detections, targets, crowd=None, area=None, area_scale=None):
        cls, rank, flags, npig = evaluate(detections, targets, self.C, self.conf, self.thr, self.rng, crowd, area, area_scale,
                                          self.counters)
        self.cls.append(cls.ravel())
        self.scores.append(np.asarray(detections[0], F32).ravel())
        self.rank.append(rank.ravel())
        self.flags.append(flags.reshape(-1, len(self.rng)))
        self.npig += npig
        return cls, rank, flags, npig

    def arrays(self):
        if not self.cls:
            shape = (len(self.rng), len(self.max_dets), len(self.thr), self.C)
            return np.full(shape, np.nan), np.full(shape, np.nan)
        return accumulate(np.concatenate(self.cls), np.concatenate(self.scores), np.concatenate(self.rank), np.concatenate(self.flags),
                          self.npig, self.C, len(self.thr), self.max_dets)

    def get_results(self):
        ap, recall = self.arrays()
        summary = summarize(ap, recall, self.thr)
        return summary["AP"], {"summary": summary, "ap": ap, "recall": recall}


# ---- the conditions under which flags are compared bit for bit ---------------------------------------------------------------
MARGIN = 1e-4
AREA_EDGES = (32.0 ** 2, 96.0 ** 2)
AREA_MARGIN = 1e-4  # relative


def iou_margin(cases, thresholds):
    """The smallest |IoU - t| over the (detection, same-class box) pairs of ``cases`` and all t, crowd boxes in their own form."""
    thr = np.asarray(thresholds, F32).astype(np.float64)
    best = np.inf
    for case in cases:
        (scores, boxes, classes), targets = case["detections"], case["targets"]
        for b in range(len(scores)):
            tg = targets[b]
            cr = np.zeros(len(tg), bool) if case["crowd"] is None else case["crowd"][b] != 0
            for c in set(float(v) for v in tg[:, 4] if v >= 0):
                rows, dets = tg[:, 4] == F32(c), classes[b] == F32(c)
                if not dets.any():
                    continue
                iou = ious_of(boxes[b][dets], tg[rows, :4], cr[rows]).astype(np.float64)
                iou = iou[~np.isnan(iou)]
                if iou.size:
                    best = min(best, float(np.min(np.abs(iou[:, None] - thr[None, :]))))
    return best


def _areas(case):
    out = []
    for b in range(len(case["targets"])):
        scale = 1.0 if case["area_scale"] is None else case["area_scale"][b]
        real = case["targets"][b][:, 4] >= 0
        g = box_area(case["targets"][b][:, :4], scale) if case["area"] is None else case["area"][b]
        out.append((box_area(case["detections"][1][b], scale)[case["detections"][0][b] > 0], np.asarray(g, F32)[real]))
    return out


def conditions(cases, thresholds):
    """{"iou_margin", "distinct_scores", "area_margin" (smallest relative distance of an area to 32^2 / 96^2), "min_det_area"}."""
    seen, distinct = set(), True
    rel, low = np.inf, np.inf
    for case in cases:
        scores, _, classes = case["detections"]
        for s, c in zip(scores.ravel(), classes.ravel()):
            if s > 0:
                distinct = distinct and (float(c), float(s)) not in seen
                seen.add((float(c), float(s)))
        for d, g in _areas(case):
            for v in (d, g):
                for e in AREA_EDGES:
                    if v.size:
                        rel = min(rel, float(np.min(np.abs(v.astype(np.float64) - e) / e)))
            if d.size:
                low = min(low, float(d.min()))
    return {"iou_margin": iou_margin(cases, thresholds), "distinct_scores": distinct, "area_margin": rel, "min_det_area": low}


# ---- seeded inputs ----------------------------------------------------------------------------------------------------------
def _area_ok(v, scale):
    a = float(v) * float(scale)
    return a > 0 and all(abs(a - e) / e >= 2 * AREA_MARGIN for e in AREA_EDGES)


def make_case(seed, B, D, G, C, thresholds, batches=1, crowd=0.2, with_area=False, area_scale=None, all_crowd_image=None,
              empty_image=None, no_gt_class=None, full=False, clustered=False):
    """[case] * batches, case = dict(detections, targets, crowd, area, area_scale): scores descending per image and zero padded,
    boxes ltrb with sides of 8 .. 260 (log-uniform: small, medium and large areas), targets [B, G, 5] with -1 rows as padding,
    ``crowd`` [B, G] int32 (share ``crowd`` of the boxes; None if 0), ``area`` [B, G] (0.5 .. 1 of the box area; None unless
    ``with_area``), ``area_scale`` [B] (None | a list that is cycled).  Detections: jittered copies of a box, small boxes inside a
    crowd box (several per crowd box: it is taken again), and random ones.  ``no_gt_class``: no box of that class, detections of
    it.  ``all_crowd_image`` / ``empty_image``: an image whose boxes are all crowd / that has none."""
    rs = np.random.RandomState(seed)
    thr = np.asarray(thresholds, F32).astype(np.float64)
    pool = rs.permutation(1 << 20)[: batches * B * D].astype(np.float64)
    all_scores = (0.05 + 0.9 * (pool + 1) / float((1 << 20) + 1)).astype(F32)
    assert len(np.unique(all_scores)) == len(all_scores)
    gt_classes = [c for c in range(C) if c != no_gt_class]
    out, k = [], 0
    for _ in range(batches):
        scores, boxes = np.zeros((B, D), F32), np.zeros((B, D, 4), F32)
        classes, targets = np.zeros((B, D), F32), np.full((B, G, 5), -1, F32)
        crowds, areas = np.zeros((B, G), np.int32), np.zeros((B, G), F32)
        scales = None if area_scale is None else np.array([area_scale[b % len(area_scale)] for b in range(B)], F32)
        for b in range(B):
            scale = 1.0 if scales is None else float(scales[b])
            span = 60 if clustered else 400
            g = 0 if b == empty_image else (G if (b == 0 or full) else rs.randint(0, G + 1))
            for j in range(g):
                while True:
                    w, h = np.exp(rs.uniform(np.log(8), np.log(260), 2))
                    x, y = rs.random_sample(2) * span
                    row = np.array([x, y, x + w, y + h, gt_classes[rs.randint(0, len(gt_classes))]], F32)
                    ar = F32(box_area(row[:4], 1.0) * F32(rs.uniform(0.5, 1.0))) if with_area else box_area(row[:4], 1.0)
                    if _area_ok(ar, 1.0 if with_area else scale):
                        break
                targets[b, j] = row
                areas[b, j] = ar
                crowds[b, j] = 1 if (b == all_crowd_image or rs.random_sample() < crowd) else 0
            n = D if (b == 0 or full) else rs.randint(max(D // 2, 1), D + 1)
            for i in range(n):
                while True:
                    u = rs.random_sample()
                    if g > 0 and u < 0.75:
                        j = rs.randint(0, g)
                        t = targets[b, j]
                        if crowds[b, j] and rs.random_sample() < 0.7:  # a box mostly inside the crowd region
                            wh = (t[2:4] - t[:2]) * (0.2 + 0.5 * rs.random_sample(2))
                            xy = t[:2] + (t[2:4] - t[:2] - wh) * rs.uniform(-0.1, 1.1, 2)
                            bx = np.concatenate([xy, xy + wh]).astype(F32)
                        else:
                            amp = 0.02 + 0.5 * rs.random_sample()
                            bx = t[:4] + ((rs.random_sample(4) - 0.5) * amp * np.tile(t[2:4] - t[:2], 2)).astype(F32)
                        cl = t[4] if rs.random_sample() < 0.9 else rs.randint(0, C)
                    else:
                        xy = rs.random_sample(2) * span
                        bx = np.concatenate([xy, xy + np.exp(rs.uniform(np.log(8), np.log(260), 2))]).astype(F32)
                        cl = rs.randint(0, C) if (no_gt_class is None or rs.random_sample() < 0.7) else no_gt_class
                    if not (bx[2] > bx[0] and bx[3] > bx[1]) or not _area_ok(box_area(bx, 1.0), scale):
                        continue
                    rows = targets[b, :, 4] == F32(cl)
                    if rows.any():
                        iou = ious_of(bx[None].astype(F32), targets[b][rows, :4], crowds[b][rows] != 0).astype(np.float64)
                        if np.min(np.abs(iou[0][:, None] - thr[None, :])) < 2 * MARGIN:
                            continue
                    break
                boxes[b, i], classes[b, i] = bx, cl
            scores[b, :n] = np.sort(all_scores[k:k + n])[::-1]
            k += D
        out.append(dict(detections=(scores, boxes, classes), targets=targets, crowd=crowds if crowd > 0 or all_crowd_image is not None else None,
                        area=areas if with_area else None, area_scale=scales))
    return out
