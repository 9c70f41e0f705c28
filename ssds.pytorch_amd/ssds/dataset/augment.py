"""Training input pipeline: the reference's DALI graph (``ssds/dataset/dali_dataiterator.py:72-103``) with the random
numbers drawn on the host and the pixels moved by ONE HIP pass (``ssdk_augment``, csrc/ssdk_augment.hip).

* ``sample_batch`` -- pure numpy, the only place random numbers are drawn: SSD random crop, colour twist folded into one
  3x4 matrix per image, horizontal flip, paste onto a canvas, resize.  Returns the kernel's descriptors and the target
  tensor of the loaders' contract (``dali_dataiterator.py:153-186``): ``[B, maxG, 5] = (x, y, w, h, label)`` in pixels of
  ``IMAGE_SIZE``, padding rows -1.
* ``PackedDetectionSource`` -- shards ``*.npz`` of packed uint8 HWC RGB images and their boxes (tools/pack_dataset.py).
* ``AugmentedLoader`` -- shards batches over ranks, stages each packed batch in pinned memory, uploads it and launches the
  kernel on a side stream one batch ahead; same iteration contract as ``SyntheticDetectionLoader``.

The semantics (and where they leave DALI on purpose) are in DESIGN.md "Data input"; tests/augment_oracle.py restates the
pixel path in fp64.  torch is imported only by the loader."""
import glob
import os

import numpy as np

# the numpy view of ssdk_augment_desc (include/ssdk.h); _native.AugmentDesc is the ctypes one, and both are compared with
# ssdk_augment_desc_bytes() before anything is launched
DESC_DTYPE = np.dtype([("src_offset", "<i8"), ("src_h", "<i4"), ("src_w", "<i4"), ("crop_x", "<i4"), ("crop_y", "<i4"),
                       ("crop_w", "<i4"), ("crop_h", "<i4"), ("canvas_w", "<i4"), ("canvas_h", "<i4"), ("paste_x", "<i4"),
                       ("paste_y", "<i4"), ("flip", "<i4"), ("color", "<f4", (12,)), ("fill", "<f4", (3,))], align=True)

CROP_THRESHOLDS = (0.0, 0.1, 0.3, 0.5, 0.7, 0.9)  # dali_dataiterator.py:31-38; option 0 is "no crop", option k is CROP_THRESHOLDS[k-1]
CROP_ROUNDS = 8  # options drawn per image before it is left uncropped (option -1)

# NTSC RGB -> YIQ; the way back is its fp64 inverse
RGB_TO_YIQ = np.array([[0.299, 0.587, 0.114], [0.596, -0.274, -0.322], [0.211, -0.523, 0.312]], np.float64)
YIQ_TO_RGB = np.linalg.inv(RGB_TO_YIQ)
IDENTITY_COLOR = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float32)


def vec3(v):
    """PREPROC.MEAN / STD: a scalar (the shipped configs: 0 and 255) or three per-channel values."""
    a = np.asarray(v, np.float64).reshape(-1)
    if a.size == 1:
        a = np.repeat(a, 3)
    if a.size != 3:
        raise ValueError("PREPROC.MEAN / STD must be a scalar or three values, got {!r}".format(v))
    return a


def color_matrix(hue_deg, sat, bri, con):
    """hue rotation (degrees) and saturation scaling of the chroma plane in YIQ, then ``bri * (128 + con * (v - 128))``:
    all affine, folded in fp64 into one 3x4 matrix applied to (r, g, b, 1).  Broadcasts over leading dimensions."""
    hue, sat, bri, con = (np.asarray(v, np.float64) for v in (hue_deg, sat, bri, con))
    shape = np.broadcast(hue, sat, bri, con).shape
    c, s = np.cos(np.deg2rad(hue)) * sat, np.sin(np.deg2rad(hue)) * sat
    twist = np.zeros(shape + (3, 3), np.float64)
    twist[..., 0, 0] = 1
    twist[..., 1, 1], twist[..., 1, 2] = c, -s
    twist[..., 2, 1], twist[..., 2, 2] = s, c
    hsv = YIQ_TO_RGB @ twist @ RGB_TO_YIQ
    m = np.empty(shape + (3, 4), np.float64)
    m[..., :3] = (bri * con)[..., None, None] * hsv
    m[..., 3] = (bri * 128.0 * (1.0 - con))[..., None]
    return m


def batch_rng(seed, rank, epoch, batch_index):
    """The generator of one batch: reproducible, and different on every rank, epoch and batch."""
    return np.random.default_rng([int(seed), int(rank), int(epoch), int(batch_index)])


def _pad_boxes(boxes, B):
    n = np.array([len(b) for b in boxes], np.int64)
    G = max(1, int(n.max()) if B else 1)
    out = np.zeros((B, G, 5), np.float64)
    for i, b in enumerate(boxes):
        if len(b):
            out[i, :len(b)] = np.asarray(b, np.float64).reshape(-1, 5)
    return out, np.arange(G)[None, :] < n[:, None]


def _sample_crops(rng, Wf, Hf, ltrb, valid, preproc):
    """SSD random crop for the whole batch at once: per round one option per image and CROP_ATTEMPTS rectangles, the
    first acceptable one wins.  -> integer rectangles (x, y, w, h) [B, 4], option [B], round [B]."""
    B = Wf.shape[0]
    A = int(preproc["CROP_ATTEMPTS"])
    s0, s1 = (float(v) for v in preproc["CROP_SCALE"])
    a0, a1 = (float(v) for v in preproc["CROP_ASPECT_RATIO"])
    thr = np.asarray(CROP_THRESHOLDS, np.float64)
    rect = np.stack([np.zeros(B), np.zeros(B), Wf, Hf], 1).astype(np.int64)
    option = np.full(B, -1, np.int64)
    rnd = np.full(B, CROP_ROUNDS, np.int64)
    todo = np.ones(B, bool)
    has_box = valid.any(1)
    for r in range(CROP_ROUNDS):
        opt_all = rng.integers(0, len(thr) + 1, size=B)
        u_all = rng.random((B, A, 4))  # drawn for every image, so the stream does not depend on how early others settled
        nocrop = todo & (opt_all == 0)
        option[nocrop], rnd[nocrop] = 0, r
        todo &= ~nocrop
        sel = np.nonzero(todo)[0]  # the images still looking for a crop: only they are evaluated
        if not len(sel):
            continue
        opt, u = opt_all[sel], u_all[sel]
        W_, H_ = Wf[sel, None], Hf[sel, None]
        bl, bt, br, bb = (ltrb[sel, None, :, k] for k in range(4))  # [S, 1, G]
        bcx, bcy, barea = (bl + br) * 0.5, (bt + bb) * 0.5, (br - bl) * (bb - bt)
        t = thr[opt - 1][:, None]
        rw, rh = s0 + (s1 - s0) * u[:, :, 0], s0 + (s1 - s0) * u[:, :, 1]
        aspect = (rw * W_) / (rh * H_)
        ok = (aspect >= a0) & (aspect <= a1)
        px, py = u[:, :, 2] * (1.0 - rw), u[:, :, 3] * (1.0 - rh)
        l = np.minimum(np.floor(px * W_), W_ - 1)
        tp = np.minimum(np.floor(py * H_), H_ - 1)
        cw = np.maximum(np.minimum(np.floor((px + rw) * W_), W_) - l, 1)
        ch = np.maximum(np.minimum(np.floor((py + rh) * H_), H_) - tp, 1)
        L, T, R, Bm = l[:, :, None], tp[:, :, None], (l + cw)[:, :, None], (tp + ch)[:, :, None]  # [S, A, 1]
        keep = valid[sel, None, :] & (bcx > L) & (bcx < R) & (bcy > T) & (bcy < Bm)
        iw = np.maximum(np.minimum(br, R) - np.maximum(bl, L), 0)
        ih = np.maximum(np.minimum(bb, Bm) - np.maximum(bt, T), 0)
        inter = iw * ih
        iou = inter / (barea + (cw * ch)[:, :, None] - inter + 1e-300)
        low = (keep & (iou < t[:, :, None])).any(2)
        ok &= ~has_box[sel, None] | (keep.any(2) & ~low)
        hit = np.nonzero(ok.any(1))[0]
        f = ok.argmax(1)[hit]
        idx = sel[hit]
        rect[idx] = np.stack([l[hit, f], tp[hit, f], cw[hit, f], ch[hit, f]], 1).astype(np.int64)
        option[idx], rnd[idx] = opt[hit], r
        todo[idx] = False
    return rect, option, rnd


def sample_batch(rng, shapes, boxes, preproc, image_size, training, max_gt=None):
    """Descriptors and targets of one batch.

    rng         numpy.random.Generator (``batch_rng``)
    shapes      [B, 2] (height, width) of the source images
    boxes       B arrays [n_i, 5] = (l, t, r, b, label) in source pixels
    preproc     cfg.DATASET.PREPROC (or a dict with its keys)
    image_size  (height, width) of the network input, as cfg.MODEL.IMAGE_SIZE
    max_gt      None: maxG = max(1, most boxes in the batch); an integer: exactly that many rows, an image with more boxes
                keeps its largest by area

    -> (descs [B] of DESC_DTYPE with src_offset 0, targets [B, maxG, 5] float32, info); info holds per image ``option``
    (0 no crop, k threshold CROP_THRESHOLDS[k-1], -1 left uncropped after CROP_ROUNDS rounds), ``round``, the kept boxes
    ``keep`` [B, G] (columns = the order of ``boxes[i]``), ``rows`` (per image: which of ``boxes[i]`` fill the rows of its targets),
    the colour parameters, and ``dropped`` (boxes cut by max_gt)."""
    shapes = np.asarray(shapes, np.int64).reshape(-1, 2)
    B = shapes.shape[0]
    if len(boxes) != B:
        raise ValueError("sample_batch: {} shapes but {} box arrays".format(B, len(boxes)))
    H, W = int(image_size[0]), int(image_size[1])
    Hs, Ws = shapes[:, 0], shapes[:, 1]
    padded, valid = _pad_boxes(boxes, B)
    ltrb, labels = padded[:, :, :4].copy(), padded[:, :, 4]
    fill = vec3(preproc["MEAN"])
    descs = np.zeros(B, DESC_DTYPE)
    descs["src_h"], descs["src_w"] = Hs, Ws
    descs["fill"] = fill.astype(np.float32)
    info = {}
    if training:
        rect, info["option"], info["round"] = _sample_crops(rng, Ws.astype(np.float64), Hs.astype(np.float64), ltrb, valid, preproc)
        cx, cy, cw, ch = (rect[:, k] for k in range(4))
        bcx, bcy = (ltrb[:, :, 0] + ltrb[:, :, 2]) * 0.5, (ltrb[:, :, 1] + ltrb[:, :, 3]) * 0.5
        cropped = (info["option"] > 0)[:, None]
        inside = (bcx > cx[:, None]) & (bcx < (cx + cw)[:, None]) & (bcy > cy[:, None]) & (bcy < (cy + ch)[:, None])
        keep = valid & (inside | ~cropped)
        # clip to the rectangle and shift
        ltrb[:, :, 0] = np.clip(ltrb[:, :, 0], cx[:, None], (cx + cw)[:, None]) - cx[:, None]
        ltrb[:, :, 2] = np.clip(ltrb[:, :, 2], cx[:, None], (cx + cw)[:, None]) - cx[:, None]
        ltrb[:, :, 1] = np.clip(ltrb[:, :, 1], cy[:, None], (cy + ch)[:, None]) - cy[:, None]
        ltrb[:, :, 3] = np.clip(ltrb[:, :, 3], cy[:, None], (cy + ch)[:, None]) - cy[:, None]
        # colour: hue, saturation, brightness, contrast -> one matrix
        hd, bd = float(preproc["HUE_DELTA"]), float(preproc["BRI_DELTA"]) / 256.0
        (c0, c1), (t0, t1) = preproc["CONTRAST_RANGE"], preproc["SATURATION_RANGE"]
        u = rng.random((B, 8))
        hue, sat = (2 * u[:, 0] - 1) * hd, t0 + (t1 - t0) * u[:, 1]
        bri, con = 1 + (2 * u[:, 2] - 1) * bd, c0 + (c1 - c0) * u[:, 3]
        info.update(hue=hue, sat=sat, bri=bri, con=con)
        descs["color"] = color_matrix(hue, sat, bri, con).reshape(B, 12).astype(np.float32)
        # flip
        flip = u[:, 4] < 0.5
        fl, fr = cw[:, None] - ltrb[:, :, 2], cw[:, None] - ltrb[:, :, 0]
        ltrb[:, :, 0] = np.where(flip[:, None], fl, ltrb[:, :, 0])
        ltrb[:, :, 2] = np.where(flip[:, None], fr, ltrb[:, :, 2])
        # paste
        ratio = 1 + (float(preproc["MAX_EXPAND_RATIO"]) - 1) * u[:, 5]
        canvas_w = np.maximum(np.floor(cw * ratio), cw).astype(np.int64)
        canvas_h = np.maximum(np.floor(ch * ratio), ch).astype(np.int64)
        paste_x = np.floor(u[:, 6] * (canvas_w - cw)).astype(np.int64)
        paste_y = np.floor(u[:, 7] * (canvas_h - ch)).astype(np.int64)
        ltrb[:, :, 0::2] += paste_x[:, None, None]
        ltrb[:, :, 1::2] += paste_y[:, None, None]
    else:
        cx, cy, cw, ch = np.zeros(B, np.int64), np.zeros(B, np.int64), Ws, Hs
        keep, flip = valid, np.zeros(B, bool)
        canvas_w, canvas_h, paste_x, paste_y = Ws, Hs, np.zeros(B, np.int64), np.zeros(B, np.int64)
        descs["color"] = IDENTITY_COLOR  # exactly: folding hue = 0 gives the identity only to rounding
        info["option"], info["round"] = np.zeros(B, np.int64), np.zeros(B, np.int64)
    for name, v in (("crop_x", cx), ("crop_y", cy), ("crop_w", cw), ("crop_h", ch), ("canvas_w", canvas_w),
                    ("canvas_h", canvas_h), ("paste_x", paste_x), ("paste_y", paste_y), ("flip", flip)):
        descs[name] = v
    # resize: canvas -> IMAGE_SIZE; (l, t, r, b) -> (x, y, w, h)
    sx, sy = (W / canvas_w.astype(np.float64))[:, None], (H / canvas_h.astype(np.float64))[:, None]
    xywh = np.stack([ltrb[:, :, 0] * sx, ltrb[:, :, 1] * sy, (ltrb[:, :, 2] - ltrb[:, :, 0]) * sx,
                     (ltrb[:, :, 3] - ltrb[:, :, 1]) * sy, labels], 2)
    count = keep.sum(1)
    dropped = 0
    if max_gt is None:
        G = max(1, int(count.max()) if B else 1)
    else:
        G = int(max_gt)
        if G < 1:
            raise ValueError("max_gt must be at least 1")
    targets = np.full((B, G, 5), -1.0, np.float32)
    which = []
    for i in range(B):
        rows, src = xywh[i, keep[i]], np.nonzero(keep[i])[0]
        if len(rows) > G:  # only with max_gt: keep the largest by area, in their original order
            dropped += len(rows) - G
            largest = np.sort(np.argsort(-(rows[:, 2] * rows[:, 3]), kind="stable")[:G])
            rows, src = rows[largest], src[largest]
        targets[i, :len(rows)] = rows
        which.append(src)
    info.update(keep=keep, dropped=dropped, rows=which)
    return descs, targets, info


class PackedDetectionSource(object):
    """Shards ``*.npz`` under ``path`` (tools/pack_dataset.py): ``pixels`` uint8 flat (HWC RGB images back to back),
    ``offsets`` [N] first byte of each image, ``shapes`` [N, 2] (height, width), ``boxes`` [M, 5] = (l, t, r, b, label >= 0)
    in source pixels, ``box_offsets`` [N + 1].  Optional: ``box_crowd`` [M] int32 (non-zero = crowd region) and ``box_area`` [M]
    float32 (source pixels), for the COCO summary of the eval phase.  Plain arrays: nothing is unpickled."""

    KEYS = ("pixels", "offsets", "shapes", "boxes", "box_offsets")
    OPTIONAL = ("box_crowd", "box_area")

    def __init__(self, path):
        files = sorted(glob.glob(os.path.join(path, "*.npz")))
        if not files:
            raise FileNotFoundError("PackedDetectionSource: no *.npz shard under {!r} (tools/pack_dataset.py writes them)".format(path))
        self.shards, starts = [], [0]
        for f in files:
            with np.load(f, allow_pickle=False) as z:
                missing = [k for k in self.KEYS if k not in z.files]
                if missing:
                    raise ValueError("{}: missing arrays {}".format(f, missing))
                s = {k: z[k] for k in self.KEYS}
                extra = {k: z[k] for k in self.OPTIONAL if k in z.files}
            check_shard(f, **s)
            for k, v in extra.items():
                if v.shape != (len(s["boxes"]),):
                    raise ValueError("{}: {} has shape {}, one value per box expected".format(f, k, v.shape))
            s.update(extra)
            self.shards.append(s)
            starts.append(starts[-1] + len(s["shapes"]))
        self.starts = np.asarray(starts, np.int64)

    def __len__(self):
        return int(self.starts[-1])

    def _locate(self, i):
        if not 0 <= i < len(self):
            raise IndexError(i)
        k = int(np.searchsorted(self.starts, i, side="right")) - 1
        return self.shards[k], i - int(self.starts[k])

    def shape(self, i):
        s, j = self._locate(i)
        return int(s["shapes"][j, 0]), int(s["shapes"][j, 1])

    def pixels(self, i):
        """flat uint8 view of image i (height * width * 3 bytes)"""
        s, j = self._locate(i)
        o = int(s["offsets"][j])
        return s["pixels"][o:o + int(s["shapes"][j, 0]) * int(s["shapes"][j, 1]) * 3]

    def image(self, i):
        h, w = self.shape(i)
        return self.pixels(i).reshape(h, w, 3)

    def boxes(self, i):
        s, j = self._locate(i)
        return s["boxes"][int(s["box_offsets"][j]):int(s["box_offsets"][j + 1])]

    def _per_box(self, key, i):
        s, j = self._locate(i)
        return s[key][int(s["box_offsets"][j]):int(s["box_offsets"][j + 1])] if key in s else None

    def crowd(self, i):
        """[n_i] int32 crowd flags of image i's boxes, or None if its shard holds no ``box_crowd``."""
        return self._per_box("box_crowd", i)

    def area(self, i):
        """[n_i] float32 annotation areas of image i's boxes (source pixels), or None if its shard holds no ``box_area``."""
        return self._per_box("box_area", i)


def check_shard(name, pixels, offsets, shapes, boxes, box_offsets):
    """The invariants of one shard (writer and reader): the kernel's own descriptor check relies on none of them."""
    n = len(shapes)
    ok = (pixels.dtype == np.uint8 and pixels.ndim == 1 and np.asarray(shapes).shape == (n, 2) and len(offsets) == n
          and len(box_offsets) == n + 1 and np.asarray(boxes).ndim == 2 and np.asarray(boxes).shape[1] == 5)
    if ok and n:
        size = np.asarray(shapes, np.int64).prod(1) * 3
        off, bo = np.asarray(offsets, np.int64), np.asarray(box_offsets, np.int64)
        ok = bool((size > 0).all() and (off >= 0).all() and (off + size <= pixels.size).all() and bo[0] == 0
                  and bo[-1] == len(boxes) and (np.diff(bo) >= 0).all())
        if ok and len(boxes):
            b = np.asarray(boxes, np.float64)
            ok = bool((b[:, 2] > b[:, 0]).all() and (b[:, 3] > b[:, 1]).all() and (b[:, 4] >= 0).all())
    if not ok:
        raise ValueError("{}: not a packed detection shard (see PackedDetectionSource)".format(name))


def epoch_batches(n, batch_size, rank, world_size, training, seed, epoch):
    """The index batches of one rank in one epoch.  Training: one permutation per (seed, epoch), the same on every rank,
    dealt out round-robin, every rank the same number of FULL batches (DDP needs equal step counts; at most
    world_size * batch_size - 1 images wait for the next permutation).  Eval: in order, every image exactly once, the last
    batch of a rank may be short."""
    order = np.random.default_rng([int(seed), int(epoch)]).permutation(n) if training else np.arange(n)
    if training:
        per_rank = (n // world_size) // batch_size * batch_size
        mine = order[rank::world_size][:per_rank]
    else:
        mine = order[rank::world_size]
    return [mine[i:i + batch_size] for i in range(0, len(mine), batch_size)]


class AugmentedLoader(object):
    """(images [B,3,H,W] ``dtype``, targets [B,maxG,5] float32) batches on ``device``, augmented by ``ssdk_augment``.

    Per batch: the host samples the descriptors (``sample_batch``, seeded by (seed, rank, epoch, batch index)), packs the
    batch's images into a pinned buffer, and on a side stream uploads it and launches the kernel -- one batch ahead of the
    consumer, which waits on an event.  Iterating starts the next epoch (``set_epoch`` chooses one).  ``max_gt``: None
    follows the reference's contract (maxG varies per batch); an integer pads every batch to that many rows
    (GraphedTrainStep's static tensors) and counts the boxes it had to drop in ``dropped``.  ``workers``: 1 stages in a worker
    thread, 0 in the consumer's thread (same batches: every batch has its own generator).  ``eval_extras`` (eval only): batches
    are (images, targets, extras) with extras = dict(crowd [B,maxG] int32, area [B,maxG] float32 in source pixels, area_scale [B]
    float32 = source pixels per network pixel) on ``device`` -- what ``CocoSummary`` takes next to the targets."""

    SLOTS = 3  # staging buffers: the batch whose kernel may still run, the one launched ahead, the one being packed

    def __init__(self, source, dataset_cfg, batch_size, device, dtype=None, training=True, seed=1234, rank=0, world_size=1,
                 max_gt=None, image_size=None, workers=1, eval_extras=False):
        self.source, self.cfg, self.batch_size, self.device = source, dataset_cfg, int(batch_size), device
        self.dtype, self.training, self.seed, self.rank, self.world_size = dtype, bool(training), int(seed), int(rank), int(world_size)
        self.max_gt, self.workers, self.eval_extras = max_gt, int(workers), bool(eval_extras)
        if self.eval_extras and self.training:
            raise ValueError("AugmentedLoader: eval_extras describes the un-augmented boxes of an eval batch (training=False)")
        self.image_size = tuple(int(v) for v in (image_size if image_size is not None else dataset_cfg["IMAGE_SIZE"]))
        self.preproc = dataset_cfg["PREPROC"]
        self.mean, self.std = vec3(self.preproc["MEAN"]), vec3(self.preproc["STD"])
        self.epoch, self.dropped = 0, 0
        self._slots = None
        if len(self.batches(0)) == 0:
            raise ValueError("AugmentedLoader: {} images give rank {} of {} no batch of {}".format(
                len(source), rank, world_size, batch_size))

    def batches(self, epoch):
        return epoch_batches(len(self.source), self.batch_size, self.rank, self.world_size, self.training, self.seed, epoch)

    def __len__(self):
        return len(self.batches(self.epoch))

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def describe(self, epoch, batch_index, indices):
        """Host half of one batch: (descs with src_offset filled in, targets, info, total bytes)."""
        shapes = np.array([self.source.shape(int(i)) for i in indices], np.int64)
        boxes = [self.source.boxes(int(i)) for i in indices]
        rng = batch_rng(self.seed, self.rank, epoch, batch_index)
        descs, targets, info = sample_batch(rng, shapes, boxes, self.preproc, self.image_size, self.training, self.max_gt)
        size = shapes.prod(1) * 3
        descs["src_offset"] = np.concatenate([[0], np.cumsum(size)[:-1]])
        return descs, targets, info, int(size.sum())

    def extras(self, indices, targets, info):
        """Host half of ``eval_extras``: numpy crowd / area [B, maxG] along the rows of ``targets`` (0 on padding rows; the source
        box area where the shard holds no ``box_area``, 0 where it holds no ``box_crowd``) and area_scale [B]."""
        B, G = targets.shape[0], targets.shape[1]
        crowd, area, scale = np.zeros((B, G), np.int32), np.zeros((B, G), np.float32), np.zeros(B, np.float32)
        has = lambda f: getattr(self.source, f, None) is not None  # noqa: E731
        for b, i in enumerate(indices):
            rows = info["rows"][b]
            h, w = self.source.shape(int(i))
            scale[b] = (w / float(self.image_size[1])) * (h / float(self.image_size[0]))
            c = self.source.crowd(int(i)) if has("crowd") else None
            a = self.source.area(int(i)) if has("area") else None
            if a is None:
                bx = np.asarray(self.source.boxes(int(i)), np.float32).reshape(-1, 5)
                a = (bx[:, 2] - bx[:, 0]) * (bx[:, 3] - bx[:, 1])
            area[b, :len(rows)] = np.asarray(a, np.float32)[rows]
            if c is not None:
                crowd[b, :len(rows)] = np.asarray(c, np.int32)[rows]
        return dict(crowd=crowd, area=area, area_scale=scale)

    # ---- staging (a worker thread) and launch (the consumer's thread) ------------------------------------------------
    def _prepare(self, k, epoch, batch_index, indices):
        """Worker thread: sample the descriptors and pack the batch's images into the slot's pinned buffers."""
        import torch

        descs, targets, info, nbytes = self.describe(epoch, batch_index, indices)
        B = len(indices)
        s = self._slots[k % self.SLOTS]
        if s["event"] is not None:
            s["event"].synchronize()  # the upload and the kernel that read these buffers last (SLOTS batches ago)
        if s["host"] is None or s["host"].numel() < nbytes:
            s["host"] = torch.empty(nbytes + nbytes // 4, dtype=torch.uint8, pin_memory=True)
        if s["descs"] is None:
            s["descs"] = torch.empty(self.batch_size * DESC_DTYPE.itemsize, dtype=torch.uint8, pin_memory=True)
            s["targets"] = {}
        host = s["host"].numpy()
        for d, i in zip(descs, indices):
            px = self.source.pixels(int(i))
            host[int(d["src_offset"]):int(d["src_offset"]) + px.size] = px
        # pinned: the library's async copy reads the descriptors after the call has returned
        s["descs"].numpy()[:B * DESC_DTYPE.itemsize] = descs.view(np.uint8).reshape(-1)
        t_host = s["targets"].get(targets.shape)
        if t_host is None:
            t_host = s["targets"][targets.shape] = torch.empty(targets.shape, dtype=torch.float32, pin_memory=True)
        t_host.numpy()[...] = targets
        extras = self.extras(indices, targets, info) if self.eval_extras else None
        return dict(slot=s, B=B, nbytes=nbytes, targets=t_host, dropped=info["dropped"], extras=extras)

    def _launch(self, prep):
        """Consumer's thread: upload and kernel on the side stream, an event behind them."""
        import torch

        from ssds import _native as N

        s, B, nbytes = prep["slot"], prep["B"], prep["nbytes"]
        self.dropped += prep["dropped"]
        ws_bytes = int(N.lib.ssdk_augment_workspace_bytes(self.batch_size))
        dtype = self.dtype if self.dtype is not None else torch.float32
        with torch.cuda.stream(self._stream):
            if s["dev"] is None or s["dev"].numel() < nbytes:
                s["dev"] = torch.empty(s["host"].numel(), dtype=torch.uint8, device=self.device)
            if s["ws"] is None:
                s["ws"] = torch.empty(ws_bytes, dtype=torch.uint8, device=self.device)
            s["dev"][:nbytes].copy_(s["host"][:nbytes], non_blocking=True)
            targets = prep["targets"].to(self.device, non_blocking=True)
            images = torch.empty((B, 3) + self.image_size, dtype=dtype, device=self.device)
            augment_into(images, s["dev"], nbytes, s["descs"].numpy(), B, self.mean, self.std, s["ws"])
            extras = None
            if prep["extras"] is not None:  # (a few hundred bytes: from pageable memory, the copy is done when .to returns)
                extras = {k: torch.from_numpy(v).to(self.device) for k, v in prep["extras"].items()}
            s["event"] = torch.cuda.Event()
            s["event"].record(self._stream)
        return images, targets, s["event"], extras

    def __iter__(self):
        import torch
        from concurrent.futures import ThreadPoolExecutor

        if self._slots is None:
            self._slots = [dict(host=None, dev=None, descs=None, ws=None, event=None, targets=None) for _ in range(self.SLOTS)]
            self._stream = torch.cuda.Stream(self.device)
            self._pool = ThreadPoolExecutor(max_workers=1) if self.workers else _Inline()
        epoch = self.epoch
        self.epoch += 1
        self.dropped = 0
        batches = self.batches(epoch)
        n = len(batches)
        # staged two batches ahead (host), launched one batch ahead (device)
        staged = {b: self._pool.submit(self._prepare, b, epoch, b, batches[b]) for b in range(min(2, n))}
        nxt = self._launch(staged.pop(0).result())
        for b in range(n):
            images, targets, event, extras = nxt
            if b + 1 < n:
                nxt = self._launch(staged.pop(b + 1).result())
            if b + 2 < n:
                staged[b + 2] = self._pool.submit(self._prepare, b + 2, epoch, b + 2, batches[b + 2])
            cur = torch.cuda.current_stream(self.device)
            cur.wait_event(event)
            images.record_stream(cur)  # allocated on the side stream, consumed on this one
            targets.record_stream(cur)
            if extras is not None:
                for v in extras.values():
                    v.record_stream(cur)
                yield images, targets, extras
                continue
            yield images, targets
        if self.rank == 0 and self.max_gt is not None:
            print("AugmentedLoader: epoch {}: {} boxes dropped by max_gt = {}".format(epoch, self.dropped, self.max_gt))


class _Inline(object):
    """``workers=0``: the staging runs in the consumer's thread, at the point where a worker would have been handed it."""

    class _Done(object):
        def __init__(self, value):
            self.value = value

        def result(self):
            return self.value

    def submit(self, fn, *args):
        return self._Done(fn(*args))


def augment_into(images, pixels_dev, pixels_bytes, descs_host_u8, B, mean, std, workspace):
    """``ssdk_augment`` on the current stream: ``images`` [B,3,H,W] (device) from the packed device buffer ``pixels_dev`` and
    the host descriptor bytes ``descs_host_u8`` (a uint8 numpy view of DESC_DTYPE records, pinned for an async caller)."""
    import ctypes

    from ssds import _native as N

    if DESC_DTYPE.itemsize != int(N.lib.ssdk_augment_desc_bytes()):
        raise N.SsdkError("augment: DESC_DTYPE has {} bytes, the library's ssdk_augment_desc {}".format(
            DESC_DTYPE.itemsize, int(N.lib.ssdk_augment_desc_bytes())))
    N.require_device(images, "augment")
    N.require_device(pixels_dev, "augment")
    if not images.is_contiguous() or images.dim() != 4 or images.shape[0] != B or images.shape[1] != 3:
        raise ValueError("augment: images must be a contiguous [B,3,H,W] tensor")
    if descs_host_u8.dtype != np.uint8 or descs_host_u8.size < B * DESC_DTYPE.itemsize or not descs_host_u8.flags["C_CONTIGUOUS"]:
        raise ValueError("augment: descriptors must be {} contiguous bytes".format(B * DESC_DTYPE.itemsize))
    if pixels_bytes > pixels_dev.numel():
        raise ValueError("augment: pixels_bytes {} exceeds the device buffer ({})".format(pixels_bytes, pixels_dev.numel()))
    vec = lambda v: (ctypes.c_float * 3)(*[float(x) for x in vec3(v)])  # noqa: E731
    import torch

    with torch.cuda.device(images.device):
        rc = N.lib.ssdk_augment(pixels_dev.data_ptr(), int(pixels_bytes),
                                ctypes.cast(descs_host_u8.ctypes.data, ctypes.POINTER(N.AugmentDesc)), int(B),
                                int(images.shape[2]), int(images.shape[3]), vec(mean), vec(std), images.data_ptr(),
                                N.dtype_code(images), workspace.data_ptr(), int(workspace.numel()), N.stream_ptr(images.device))
    N.check(rc, "augment")
    return images
