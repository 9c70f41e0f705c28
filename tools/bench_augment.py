#!/usr/bin/env python
"""Measurements of the training input pipeline (ssds/dataset/augment.py, csrc/ssdk_augment.hip).  Nothing is gated on them.

    python tools/bench_augment.py --mode kernel   # ssdk_augment alone: batch 64 -> 512x512 bf16 from ~640x480 sources;
                                                  #   algorithmic bytes / event time.  For the kernel's own time run it under
                                                  #   `rocprofv3 --kernel-trace --stats -- python tools/bench_augment.py --mode kernel`
    python tools/bench_augment.py --mode loader   # AugmentedLoader batches per second, the consumer only waits
    python tools/bench_augment.py --mode step     # ms per training step (SSD-MobileNetV2@512, batch 64): the synthetic loader's
                                                  #   fixed batch and the packed loader's batches, alternating in one process

A seeded toy set (tools/pack_dataset.py) is written into a temporary directory; each mode prints one JSON line."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ssds.pytorch_amd"), os.path.join(ROOT, "tools")]


def toy_source(tmp, unique, repeat, seed=0):
    import pack_dataset
    from ssds.dataset.augment import PackedDetectionSource

    images, boxes = pack_dataset.synthetic_set(unique, seed=seed, height=(440, 520), width=(600, 680), max_boxes=8, num_classes=80)
    pack_dataset.write_shards(tmp, images * repeat, boxes * repeat, per_shard=64)
    return PackedDetectionSource(tmp)


def algorithmic_bytes(descs, H, W, itemsize):
    """every source byte of the crops once (a down-scaling factor above 2 skips rows and columns; not subtracted) + the output once"""
    src = int((descs["crop_w"].astype(np.int64) * descs["crop_h"] * 3).sum())
    return src, len(descs) * 3 * H * W * itemsize


def mode_kernel(args, src, cfg):
    import torch

    from ssds import _native as N
    from ssds.dataset import augment as A

    dev = torch.device("cuda")
    dtype = getattr(torch, args.dtype)
    H, W = cfg["IMAGE_SIZE"]
    loader = A.AugmentedLoader(src, cfg, args.batch, dev, dtype=dtype, training=True, seed=1)
    batches = []
    for b, idx in enumerate(loader.batches(0)[:4]):
        descs, _, _, nbytes = loader.describe(0, b, idx)
        pixels = torch.from_numpy(np.concatenate([src.pixels(int(i)) for i in idx])).to(dev)
        batches.append((descs, descs.view(np.uint8).reshape(-1), pixels, nbytes))
    out = torch.empty((args.batch, 3, H, W), dtype=dtype, device=dev)
    ws = torch.empty(int(N.lib.ssdk_augment_workspace_bytes(args.batch)), dtype=torch.uint8, device=dev)
    run = lambda k: A.augment_into(out, batches[k][2], batches[k][3], batches[k][1], args.batch, 0, 255, ws)  # noqa: E731
    for k in range(args.warmup):
        run(k % len(batches))
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)]
    for k, (a, b) in enumerate(ev):
        a.record()
        run(k % len(batches))
        b.record()
    torch.cuda.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in ev)
    byts = [algorithmic_bytes(d[0], H, W, out.element_size()) for d in batches]
    mean_bytes = float(np.mean([s + o for s, o in byts]))
    med = ms[len(ms) // 2]
    return {"mode": "kernel", "batch": args.batch, "size": [H, W], "dtype": args.dtype, "launches": args.steps,
            "event_ms_median": round(med, 4), "event_ms_min": round(ms[0], 4), "event_ms_max": round(ms[-1], 4),
            "note": "event time includes the descriptor copy and the launch gap; the kernel's own time: rocprofv3 --kernel-trace --stats",
            "algorithmic_MB_source": round(float(np.mean([s for s, _ in byts])) / 1e6, 2),
            "algorithmic_MB_output": round(float(np.mean([o for _, o in byts])) / 1e6, 2),
            "GB_per_s_at_event_median": round(mean_bytes / med / 1e6, 1)}


def mode_loader(args, src, cfg):
    import torch

    from ssds.dataset import augment as A

    dev = torch.device("cuda")
    loader = A.AugmentedLoader(src, cfg, args.batch, dev, dtype=getattr(torch, args.dtype), training=True, seed=1)
    n, t0 = 0, None
    while n < args.warmup + args.steps:
        for images, targets in loader:
            torch.cuda.current_stream().synchronize()
            n += 1
            if n == args.warmup:
                t0 = time.perf_counter()
            if n >= args.warmup + args.steps:
                break
    el = time.perf_counter() - t0
    t = time.perf_counter()
    for b, idx in enumerate(loader.batches(0)[:4]):
        loader.describe(0, b, idx)
    host = (time.perf_counter() - t) / min(4, len(loader))
    return {"mode": "loader", "batch": args.batch, "dtype": args.dtype, "batches": args.steps,
            "batches_per_s": round(args.steps / el, 1), "images_per_s": round(args.steps * args.batch / el, 1),
            "host_sampling_ms_per_batch": round(host * 1e3, 2)}


def mode_step(args, src, cfg_d):
    import torch

    from ssds.core import config
    from ssds.dataset import augment as A
    from ssds.dataset.synthetic import SyntheticDetectionLoader
    from ssds.modeling import model_builder
    from ssds.pipeline.pipeline_anchor_ddp import train_step
    from ssds.utils.train_ddp import Solver

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    cfg = config.cfg_from_file(os.path.join(ROOT, "experiments", "cfgs", "ssd_mobilenetv2_512.yml"))
    cfg.TRAIN.BATCH_SIZE = args.batch
    cfg.EXP_DIR = os.path.join(tempfile.gettempdir(), "ssdk_bench_augment")
    torch.manual_seed(1234)
    solver = Solver(cfg, 0, dev)
    mwl = solver.wrap()
    mwl.train()
    anchors = model_builder.create_anchors(cfg.MODEL, mwl.model, cfg.MODEL.IMAGE_SIZE)
    fixed = SyntheticDetectionLoader(args.batch, cfg.MODEL.IMAGE_SIZE, cfg.MODEL.NUM_CLASSES, 1, dev, seed=1234).batch()
    loader = A.AugmentedLoader(src, cfg.DATASET, args.batch, dev, dtype=getattr(torch, args.dtype), training=True, seed=1,
                               image_size=cfg.MODEL.IMAGE_SIZE, workers=args.workers)

    def packed_batches():
        while True:
            for batch in loader:
                yield batch

    it = packed_batches()

    host = {"synthetic": [], "packed": []}

    def run(kind, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            images, targets = fixed if kind == "synthetic" else next(it)
            train_step(mwl, images, targets, anchors, solver.optimizer)
        host[kind].append(round((time.perf_counter() - t0) / steps * 1e3, 3))  # the host's share: steps enqueued, not yet run
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps * 1e3

    for kind in ("synthetic", "packed"):
        run(kind, args.warmup)
    res = {"synthetic": [], "packed": []}
    for _ in range(args.repeats):
        for kind in ("synthetic", "packed"):
            res[kind].append(round(run(kind, args.steps), 3))
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    return {"mode": "step", "workers": args.workers, "host_enqueue_ms": {k: v[1:] for k, v in host.items()}, "batch": args.batch, "steps_per_repeat": args.steps, "images_dtype": args.dtype,
            "synthetic_ms": res["synthetic"], "packed_ms": res["packed"], "synthetic_ms_median": med(res["synthetic"]),
            "packed_ms_median": med(res["packed"]), "synthetic_spread_ms": round(max(res["synthetic"]) - min(res["synthetic"]), 3),
            "note": "synthetic = one fixed device batch reused every step (tools/bench_train.py); packed = a new augmented batch per step"}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--mode", required=True, choices=("kernel", "loader", "step"))
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--dtype", default=None, help="images dtype (kernel, loader: bfloat16; step: float32, what train_ddp feeds)")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5, help="step mode: alternations of synthetic / packed")
    ap.add_argument("--workers", type=int, default=1, help="step mode: AugmentedLoader(workers=...): 0 stages in the consumer's thread")
    ap.add_argument("--unique", type=int, default=64, help="distinct toy images")
    ap.add_argument("--repeat-set", type=int, default=6, help="times the distinct images are repeated in the set")
    args = ap.parse_args()
    if args.dtype is None:
        args.dtype = "float32" if args.mode == "step" else "bfloat16"
    preproc = {"MEAN": 0, "STD": 255, "CROP_SCALE": [0.3, 1.0], "CROP_ASPECT_RATIO": [0.5, 2.0], "CROP_ATTEMPTS": 50, "HUE_DELTA": 9,
               "BRI_DELTA": 16, "CONTRAST_RANGE": [0.75, 1.25], "SATURATION_RANGE": [0.75, 1.25], "MAX_EXPAND_RATIO": 2.0}
    cfg = {"IMAGE_SIZE": [args.size, args.size], "PREPROC": preproc}
    with tempfile.TemporaryDirectory() as tmp:
        src = toy_source(tmp, args.unique, args.repeat_set)
        out = {"kernel": mode_kernel, "loader": mode_loader, "step": mode_step}[args.mode](args, src, cfg)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
