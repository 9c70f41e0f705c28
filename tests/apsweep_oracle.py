"""CPU oracle of the average-precision sweep (include/ssdk_apsweep.h, ssds.core.evaluation_metrics.AveragePrecisionSweep).

TEST INFRASTRUCTURE ONLY.  A numpy restatement of both matching rules and both AP forms: IoU in fp32 in the reference's operation
order (``oracle.map_oracle.matrix_iou``), thresholds compared in fp32, AP in fp64.

  rule "reference"  ``evaluation_metrics.py:48-56`` of the reference at every threshold: a detection above the score threshold
                    looks at the same-class box of highest IoU (first maximum) only; it is a true positive at t iff that IoU >= t
                    and no earlier detection reached t on the same box.  AP: the VOC area (``oracle.map_oracle``).
  rule "coco"       pycocotools ``evaluateImg`` without crowd and area ranges: only the first ``max_dets`` valid detections of an
                    image count; per class and threshold a detection takes the free box of highest IoU >= t, among equal IoUs the
                    one of HIGHEST index (the ``<`` in its loop).  AP: 101-point interpolation as in ``accumulate`` (without the
                    ``np.spacing(1)`` in the precision denominator).

Two CONDITION checkers say when the device may be compared bit for bit: ``iou_margin`` (no IoU closer than the margin to a
threshold, so a last-bit difference of an IoU could not flip a flag) and ``distinct_scores`` (ranking ties are outside the
contract).  The seeded generator redraws a detection until the first holds and draws its scores from a permutation, so both hold
by construction; the tests still assert them on what the generator returned."""
import numpy as np

from oracle.map_oracle import matrix_iou

F32 = np.float32
COCO_IOUS = np.linspace(0.5, 0.95, 10).astype(F32)
SWEEP16 = np.linspace(0.2, 0.95, 16).astype(F32)


def decode_keys(keys):
    """device keys [..] int64 -> (class (num_classes = does not count), score fp32)."""
    keys = np.asarray(keys).astype(np.int64)
    cls = (keys >> 32).astype(np.int64)
    u = (~keys & 0xFFFFFFFF).astype(np.uint32)
    bits = np.where(u & 0x80000000, u & 0x7FFFFFFF, ~u).astype(np.uint32)
    return cls, bits.view(F32)


def match(detections, targets, num_classes, conf_threshold, thresholds, rule, max_dets=100, assigned=None):
    """-> (cls [B, D] with num_classes where a slot does not count, mask [B, D] int32, npos [C]) of one batch.  ``assigned``: a dict
    that receives {(image, detection, threshold index): target row} of every true positive."""
    scores, boxes, classes = (np.asarray(x, F32) for x in detections)
    targets = np.asarray(targets, F32)
    thr = np.asarray(thresholds, F32)
    B, D = scores.shape
    C = num_classes
    cls = np.full((B, D), C, np.int64)
    mask = np.zeros((B, D), np.int32)
    npos = np.zeros(C, np.int64)
    for b in range(B):
        s, bx, cl, tg = scores[b], boxes[b], classes[b], targets[b]
        for lab in tg[:, 4]:
            if 0 <= lab < C:
                npos[int(lab)] += 1
        above = s > F32(conf_threshold)
        valid = above & (cl >= 0) & (cl < C)
        if rule == "reference":
            cls[b, valid] = cl[valid].astype(np.int64)
            first = {}
            for i in np.nonzero(above)[0]:
                rows = np.nonzero(tg[:, 4] == cl[i])[0]
                if not len(rows):
                    continue
                iou = matrix_iou(bx[i:i + 1], tg[rows, :4])[0]
                v = iou.copy()  # first maximum under `iou > best`: a NaN first IoU is never replaced, a later NaN never wins
                v[1:][np.isnan(v[1:])] = -np.inf
                j = 0 if np.isnan(v[0]) else int(np.argmax(v))
                for t in range(len(thr)):
                    if iou[j] >= thr[t] and (t, rows[j]) not in first:
                        first[(t, rows[j])] = i
                        mask[b, i] |= 1 << t
                        if assigned is not None:
                            assigned[(b, int(i), t)] = int(rows[j])
            continue
        kept = np.nonzero(valid)[0][:max_dets]
        cls[b, kept] = cl[kept].astype(np.int64)
        for c in sorted(set(float(v) for v in tg[:, 4] if 0 <= v < C)):
            rows = np.nonzero(tg[:, 4] == F32(c))[0]
            dets = [i for i in kept if cl[i] == F32(c)]
            if not dets:
                continue
            iou = matrix_iou(bx[dets], tg[rows, :4])
            for t in range(len(thr)):
                taken = np.zeros(len(rows), bool)
                for di, i in enumerate(dets):
                    best, m = thr[t], -1
                    for gi in range(len(rows)):
                        if taken[gi] or not (iou[di, gi] >= best):
                            continue
                        best, m = iou[di, gi], gi
                    if m >= 0:
                        taken[m] = True
                        mask[b, i] |= 1 << t
                        if assigned is not None:
                            assigned[(b, int(i), t)] = int(rows[m])
    return cls, mask, npos


def ap_voc(tpl, npos):
    """The VOC area of the reference (evaluation_metrics.py:104-112); tpl: 0/1 by rank."""
    if npos == 0:
        return np.nan
    tpl = np.asarray(tpl, np.int64)
    if not tpl.size:
        return 0.0
    tp = np.cumsum(tpl)
    rec = tp.astype(float) / float(npos)
    prec = tp.astype(float) / np.arange(1, len(tp) + 1, dtype=float)
    r = np.concatenate([[0], rec, [1]])
    p = np.concatenate([[0], prec, [0]])
    for i in range(len(p) - 2, -1, -1):
        p[i] = max(p[i], p[i + 1])
    idx = np.where(r[1:] != r[:-1])[0] + 1
    return float(np.sum((r[idx] - r[idx - 1]) * p[idx]))


def ap_coco(tpl, npos):
    """101-point interpolation (pycocotools ``accumulate``): q_k = the envelope of the precision at the first rank whose recall
    is >= linspace(0, 1, 101)[k], 0 if there is none; their mean."""
    if npos == 0:
        return np.nan
    tpl = np.asarray(tpl, np.int64)
    n = len(tpl)
    if n == 0:
        return 0.0
    tp = np.cumsum(tpl)
    rc = tp.astype(np.float64) / float(npos)
    pr = tp.astype(np.float64) / np.arange(1, n + 1, dtype=np.float64)
    for i in range(n - 1, 0, -1):
        if pr[i] > pr[i - 1]:
            pr[i - 1] = pr[i]
    inds = np.searchsorted(rc, np.linspace(0.0, 1.0, 101), side="left")
    q = np.zeros(101)
    for k, pi in enumerate(inds):
        if pi < n:
            q[k] = pr[pi]
    return float(np.mean(q))


def ranked_flags(cls, scores, mask, num_classes, T):
    """Flattened records in arrival order -> flags[c][t] = 0/1 by rank (score descending, ties in arrival order)."""
    cls, scores, mask = np.asarray(cls).ravel(), np.asarray(scores, F32).ravel(), np.asarray(mask).ravel()
    out = []
    for c in range(num_classes):
        sel = np.nonzero(cls == c)[0]
        order = sel[np.argsort(-scores[sel].astype(np.float64), kind="stable")]
        out.append([(mask[order] >> t) & 1 for t in range(T)])
    return out


class Sweep(object):
    """The oracle with the interface of the device metric: ``__call__`` per batch, ``get_results() -> (mAP, ap [T, C])``."""

    def __init__(self, num_classes, conf_threshold, thresholds=COCO_IOUS, rule="coco", max_dets=100):
        self.C, self.conf, self.thr, self.rule, self.max_dets = num_classes, conf_threshold, np.asarray(thresholds, F32), rule, max_dets
        self.cls, self.scores, self.mask, self.npos = [], [], [], np.zeros(num_classes, np.int64)

    def __call__(self, detections, targets):
        cls, mask, npos = match(detections, targets, self.C, self.conf, self.thr, self.rule, self.max_dets)
        self.cls.append(cls.ravel())
        self.scores.append(np.asarray(detections[0], F32).ravel())
        self.mask.append(mask.ravel())
        self.npos += npos

    def get_results(self):
        T = len(self.thr)
        ap = np.full((T, self.C), np.nan)
        if self.cls:
            flags = ranked_flags(np.concatenate(self.cls), np.concatenate(self.scores), np.concatenate(self.mask), self.C, T)
            form = ap_voc if self.rule == "reference" else ap_coco
            for c in range(self.C):
                for t in range(T):
                    ap[t, c] = form(flags[c][t], int(self.npos[c]))
        return (float(np.nanmean(ap)) if not np.all(np.isnan(ap)) else float("nan")), ap


# ---- the conditions under which flags are compared bit for bit ---------------------------------------------------------------
def iou_margin(cases, thresholds):
    """The smallest |IoU - t| over the (detection, same-class box) pairs of ``cases`` = [(detections, targets)] and all t."""
    thr = np.asarray(thresholds, F32).astype(np.float64)
    best = np.inf
    for (scores, boxes, classes), targets in cases:
        for b in range(len(scores)):
            tg = targets[b]
            for c in set(float(v) for v in tg[:, 4] if v >= 0):
                rows, dets = tg[:, 4] == F32(c), classes[b] == F32(c)
                if not dets.any():
                    continue
                iou = matrix_iou(boxes[b][dets], tg[rows, :4]).astype(np.float64)
                iou = iou[~np.isnan(iou)]
                if iou.size:
                    best = min(best, float(np.min(np.abs(iou[:, None] - thr[None, :]))))
    return best


def distinct_scores(cases, conf_threshold=0.0):
    """No two detections of a class above the score threshold share a score, over all of ``cases``."""
    seen = {}
    for (scores, _, classes), _ in cases:
        for s, c in zip(np.asarray(scores).ravel(), np.asarray(classes).ravel()):
            if s > conf_threshold:
                if (float(c), float(s)) in seen:
                    return False
                seen[(float(c), float(s))] = True
    return True


# ---- seeded inputs ----------------------------------------------------------------------------------------------------------
MARGIN = 1e-4


def make_case(seed, B, D, G, C, thresholds, batches=1, clustered=False, empty_image=None, no_det_image=None, bad_class=0.0,
              full_gt=False):
    """[(detections, targets)] * batches in the shape of a Decoder output: scores descending per image and zero padded, boxes
    ltrb, classes; targets [B, G, 5] ltrb + label with -1 rows as padding.  Detections are jittered copies of the ground truth
    (jitter up to half a side, so the IoUs spread over 0.3 .. 1) plus random false positives; ``clustered`` puts the boxes of an
    image close together so that a detection overlaps several of them.  ``bad_class``: that share of the detections gets a class
    outside [0, C).  ``empty_image`` / ``no_det_image``: an image index without boxes / without detections.  A detection is
    redrawn until every IoU with a same-class box keeps 2 * MARGIN from every threshold."""
    rs = np.random.RandomState(seed)
    thr = np.asarray(thresholds, F32).astype(np.float64)
    pool = rs.permutation(1 << 20)[: batches * B * D].astype(np.float64)
    all_scores = (0.05 + 0.9 * (pool + 1) / float((1 << 20) + 1)).astype(F32)
    assert len(np.unique(all_scores)) == len(all_scores)
    out, k = [], 0
    for _ in range(batches):
        scores, boxes = np.zeros((B, D), F32), np.zeros((B, D, 4), F32)
        classes, targets = np.zeros((B, D), F32), np.full((B, G, 5), -1, F32)
        for b in range(B):
            g = 0 if b == empty_image else (G if (b == 0 or full_gt) else rs.randint(0, G + 1))
            for j in range(g):
                w, h = 30 + 120 * rs.random_sample(2)
                x, y = rs.random_sample(2) * (60 if clustered else 400)
                targets[b, j] = [x, y, x + w, y + h, rs.randint(0, C)]
            n = 0 if b == no_det_image else rs.randint(D // 2, D + 1)
            for i in range(n):
                while True:
                    if g > 0 and rs.random_sample() < 0.8:
                        t = targets[b, rs.randint(0, g)]
                        amp = 0.02 + 0.5 * rs.random_sample()
                        bx = t[:4] + ((rs.random_sample(4) - 0.5) * amp * np.tile(t[2:4] - t[:2], 2)).astype(F32)
                        cl = t[4] if rs.random_sample() < 0.9 else rs.randint(0, C)
                    else:
                        xy = rs.random_sample(2) * 400
                        bx = np.concatenate([xy, xy + 30 + 120 * rs.random_sample(2)]).astype(F32)
                        cl = rs.randint(0, C)
                    rows = targets[b, :, 4] == F32(cl)
                    if rows.any():
                        iou = matrix_iou(bx[None].astype(F32), targets[b][rows, :4]).astype(np.float64)
                        if np.min(np.abs(iou[0][:, None] - thr[None, :])) < 2 * MARGIN:
                            continue
                    break
                if rs.random_sample() < bad_class:
                    cl = C + rs.randint(0, 3) if rs.random_sample() < 0.5 else -1 - rs.randint(0, 2)
                boxes[b, i], classes[b, i] = bx, cl
            scores[b, :n] = np.sort(all_scores[k:k + n])[::-1]
            k += D
        out.append(((scores, boxes, classes), targets))
    return out


def hand_case():
    """One image, one class, boxes of height 10: GT A = [0,0,10,10], B = [4,0,14,10]; d1 = [1,0,11,10] (score 0.9: IoU 0.818
    with A, 0.538 with B), d2 = [1.5,0,11.5,10] (0.8: 0.739 with A, 0.600 with B); thresholds [0.5, 0.65, 0.8, 0.85].
    -> (detections, targets, thresholds, {rule: (masks, ap per threshold)})."""
    targets = np.array([[[0, 0, 10, 10, 0], [4, 0, 14, 10, 0]]], F32)
    det = (np.array([[0.9, 0.8]], F32), np.array([[[1, 0, 11, 10], [1.5, 0, 11.5, 10]]], F32), np.zeros((1, 2), F32))
    want = {"coco": ([0b0111, 0b0001], [1.0, 51.0 / 101.0, 51.0 / 101.0, 0.0]),
            "reference": ([0b0111, 0b0000], [0.5, 0.5, 0.5, 0.0])}
    return det, targets, np.array([0.5, 0.65, 0.8, 0.85], F32), want
