#!/usr/bin/env python
"""Write shards for ``ssds.dataset.augment.PackedDetectionSource``: ``*.npz`` holding ``pixels`` (uint8, flat: HWC RGB
images back to back), ``offsets`` [N], ``shapes`` [N, 2] (height, width), ``boxes`` [M, 5] = (l, t, r, b, label >= 0) in
source pixels and ``box_offsets`` [N + 1] -- the layout ``ssdk_augment`` takes, no pickled objects.  Optional, for the COCO
summary of the eval phase: ``box_crowd`` [M] int32 (non-zero = crowd region) and ``box_area`` [M] float32 (the annotation's area in
source pixels, e.g. of its mask), in the order of ``boxes``.

    from tools.pack_dataset import write_shards
    write_shards(out_dir, images, boxes, per_shard=256)        # images: HxWx3 uint8 arrays, boxes: [n_i, 5] arrays
    write_shards(out_dir, images, boxes, crowd=c, area=a)      # c, a: [n_i] arrays per image (either may be left out)

    python tools/pack_dataset.py --synthetic 256 --out DIR     # a seeded toy set: filled rectangles on a gradient,
                                                               # the rectangles being the boxes

Decoding JPEG or reading COCO json is not part of this project (it owns no decoder): decode with whatever you have and
hand the arrays to ``write_shards``."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ssds.pytorch_amd"))


def write_shards(out_dir, images, boxes, per_shard=256, prefix="shard", crowd=None, area=None):
    """-> the shard paths, in order.  ``crowd`` / ``area``: per image an array [n_i] in the order of its boxes, written as
    ``box_crowd`` / ``box_area``; None: the shard holds no such array."""
    from ssds.dataset.augment import check_shard

    if len(images) != len(boxes):
        raise ValueError("{} images but {} box arrays".format(len(images), len(boxes)))
    for name, extra in (("crowd", crowd), ("area", area)):
        if extra is not None and (len(extra) != len(boxes) or any(np.asarray(e).reshape(-1).shape[0] != np.asarray(b).reshape(-1, 5).shape[0]
                                                                   for e, b in zip(extra, boxes))):
            raise ValueError("{}: one value per box of every image".format(name))
    os.makedirs(out_dir, exist_ok=True)
    paths = []
    for k, lo in enumerate(range(0, len(images), per_shard)):
        imgs = [np.ascontiguousarray(im, np.uint8) for im in images[lo:lo + per_shard]]
        for im in imgs:
            if im.ndim != 3 or im.shape[2] != 3:
                raise ValueError("images must be HxWx3 uint8, got {}".format(im.shape))
        bxs = [np.asarray(b, np.float32).reshape(-1, 5) for b in boxes[lo:lo + per_shard]]
        size = np.array([im.size for im in imgs], np.int64)
        shard = dict(pixels=np.concatenate([im.reshape(-1) for im in imgs]),
                     offsets=np.concatenate([[0], np.cumsum(size)[:-1]]).astype(np.int64),
                     shapes=np.array([im.shape[:2] for im in imgs], np.int32),
                     boxes=np.concatenate(bxs) if bxs else np.zeros((0, 5), np.float32),
                     box_offsets=np.concatenate([[0], np.cumsum([len(b) for b in bxs])]).astype(np.int64))
        path = os.path.join(out_dir, "{}_{:05d}.npz".format(prefix, k))
        check_shard(path, **shard)
        for key, extra, dtype in (("box_crowd", crowd, np.int32), ("box_area", area, np.float32)):
            if extra is not None:
                shard[key] = np.concatenate([np.asarray(e, dtype).reshape(-1) for e in extra[lo:lo + per_shard]] + [np.zeros(0, dtype)])
        np.savez(path, **shard)
        paths.append(path)
    return paths


def synthetic_set(n, seed=0, height=(120, 200), width=(160, 260), max_boxes=6, num_classes=5):
    """A seeded toy set: every image is a two-axis colour gradient with 0..max_boxes filled rectangles, whose outlines are
    its boxes and whose colour encodes the label.  height / width: an int or an inclusive (low, high) range."""
    rng = np.random.default_rng([int(seed), 7])
    images, boxes = [], []
    rand = lambda v: int(v) if np.isscalar(v) else int(rng.integers(v[0], v[1] + 1))  # noqa: E731
    for _ in range(n):
        h, w = rand(height), rand(width)
        y, x = np.mgrid[0:h, 0:w]
        base = rng.integers(0, 96, 3)
        im = np.stack([base[0] + 128 * x // w, base[1] + 128 * y // h, base[2] + 64 * (x + y) // (w + h)], 2).astype(np.uint8)
        rows = []
        for _ in range(int(rng.integers(0, max_boxes + 1))):
            bw, bh = max(2, int(w * rng.uniform(0.15, 0.7))), max(2, int(h * rng.uniform(0.15, 0.7)))
            l, t = int(rng.integers(0, w - bw + 1)), int(rng.integers(0, h - bh + 1))
            label = int(rng.integers(0, num_classes))
            im[t:t + bh, l:l + bw] = ((255 - 40 * label) % 256, (60 + 35 * label) % 256, (200 - 30 * label) % 256)
            rows.append((l, t, l + bw, t + bh, label))
        images.append(im)
        boxes.append(np.array(rows, np.float32).reshape(-1, 5))
    return images, boxes


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", required=True, help="directory the shards are written to")
    ap.add_argument("--synthetic", type=int, required=True, metavar="N", help="write a seeded toy set of N images")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--height", type=int, nargs="+", default=[120, 200], help="one value, or low high (inclusive)")
    ap.add_argument("--width", type=int, nargs="+", default=[160, 260])
    ap.add_argument("--max-boxes", type=int, default=6)
    ap.add_argument("--classes", type=int, default=5)
    ap.add_argument("--per-shard", type=int, default=256)
    args = ap.parse_args(argv)
    rng_arg = lambda v: v[0] if len(v) == 1 else (v[0], v[1])  # noqa: E731
    images, boxes = synthetic_set(args.synthetic, args.seed, rng_arg(args.height), rng_arg(args.width), args.max_boxes, args.classes)
    paths = write_shards(args.out, images, boxes, args.per_shard)
    print("wrote {} images, {} boxes into {} shard(s) under {}".format(len(images), sum(len(b) for b in boxes), len(paths), args.out))


if __name__ == "__main__":
    main()
