"""The COCO summary (csrc/ssdk_cocoeval.hip) against the sweep it stands beside (csrc/ssdk_apsweep.hip, COCO rule) on the inputs
of tools/apsweep_probe.py: what the eight further numbers of the table cost.

  per batch   one ``ssdk_cocoeval_match`` (T = 10, the four COCO area ranges; once without and once with crowd flags on a tenth of
              the boxes and an ``area_scale``) against one ``ssdk_apsweep_match`` (T = 10, one range, no ignore regions): B = 64
              images, D = 100 detections, C = 80 classes, G = 8 and G = 64 boxes.  Per side a hipGraph of CALLS calls is captured and
              replayed REPS times between two device events, the sides alternating, ROUNDS rounds.
  per epoch   one stable sort of the epoch's records + one ``ssdk_cocoeval_accumulate`` (four ranges x maxDets 1 / 10 / 100 x ten
              thresholds) against one sort + one ``ssdk_apsweep_average_precision`` (the records of EPOCH_BATCHES batches), eagerly
              between two device events, alternating.

No ratio is expected in advance: the new launch matches under four area ranges where the sweep matches under one.  One JSON line
each: the median and the spread in us.

    python tools/cocoeval_probe.py [--out FILE.jsonl]
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "ssds.pytorch_amd"), os.path.join(ROOT, "tools")]

from apsweep_probe import B, C, CALLS, CONF, D, EPOCH_BATCHES, GTS, REPS, ROUNDS, batch, stats  # noqa: E402

A, MAX_DETS = 4, (1, 10, 100)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch

    assert torch.cuda.is_available(), "cocoeval_probe needs a HIP device"
    from ssds import _native as N
    from ssds.core.evaluation_metrics import COCO_AREAS, COCO_IOUS

    L, dev = N.lib, torch.device("cuda")
    thr = (ctypes.c_float * 10)(*[float(v) for v in COCO_IOUS])
    rng = (ctypes.c_float * (2 * A))(*[float(v) for v in COCO_AREAS.reshape(-1)])
    md = (ctypes.c_int * len(MAX_DETS))(*MAX_DETS)
    lines = []

    def emit(rec):
        lines.append(rec)
        print(json.dumps(rec), flush=True)

    def coco_match(scores, boxes, classes, tg, G, crowd, scale, keys, rank, flags, npig):
        N.check(L.ssdk_cocoeval_match(scores.data_ptr(), boxes.data_ptr(), classes.data_ptr(), B, D, tg.data_ptr(), G,
                                      None if crowd is None else crowd.data_ptr(), None, None if scale is None else scale.data_ptr(),
                                      C, CONF, thr, 10, rng, A, keys.data_ptr(), rank.data_ptr(), flags.data_ptr(), npig.data_ptr(),
                                      N.stream_ptr(dev)), "cocoeval_match")

    side = torch.cuda.Stream()
    for G in GTS:
        scores, boxes, classes, tg = batch(G, 7 + G, torch)
        g = torch.Generator(device="cuda").manual_seed(70 + G)
        crowd = (torch.rand(B, G, device=dev, generator=g) < 0.1).to(torch.int32)
        scale = 0.5 + 3.5 * torch.rand(B, device=dev, generator=g)
        keys = torch.empty((B, D), device=dev, dtype=torch.int64)
        mask = torch.empty((B, D), device=dev, dtype=torch.int32)
        rank = torch.empty((B, D), device=dev, dtype=torch.int32)
        flags = torch.empty((B, D, A), device=dev, dtype=torch.int32)
        npos = torch.zeros(C, device=dev, dtype=torch.int32)
        npig = torch.zeros((A, C), device=dev, dtype=torch.int32)

        def sweep():
            N.check(L.ssdk_apsweep_match(scores.data_ptr(), boxes.data_ptr(), classes.data_ptr(), B, D, tg.data_ptr(), G, C, CONF, thr,
                                         10, N.AP_RULE["coco"], 100, keys.data_ptr(), mask.data_ptr(), npos.data_ptr(),
                                         N.stream_ptr(dev)), "apsweep_match")

        fns = {"cocoeval_match": lambda: coco_match(scores, boxes, classes, tg, G, None, None, keys, rank, flags, npig),
               "cocoeval_match_crowd_scale": lambda: coco_match(scores, boxes, classes, tg, G, crowd, scale, keys, rank, flags, npig),
               "sweep_coco": sweep}
        graphs = {}
        for key, fn in fns.items():
            with torch.cuda.stream(side):
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                for _ in range(CALLS):
                    fn()
            graph.replay()
            torch.cuda.synchronize()
            graphs[key] = graph
        times = {key: [] for key in fns}
        for _ in range(ROUNDS):
            for key in fns:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(REPS):
                    graphs[key].replay()
                e1.record()
                torch.cuda.synchronize()
                times[key].append(e0.elapsed_time(e1) * 1e3 / (CALLS * REPS))
        for key in fns:
            emit(dict(what="per batch", side=key, B=B, D=D, C=C, G=G, T=10, A=A if key != "sweep_coco" else 1, **stats(times[key])))

    # ---- the end of an epoch
    G = 8
    all_keys, all_rec, all_mask = [], [], []
    npos = torch.zeros(C, device=dev, dtype=torch.int32)
    npig = torch.zeros((A, C), device=dev, dtype=torch.int32)
    for it in range(EPOCH_BATCHES):
        scores, boxes, classes, tg = batch(G, 1000 + it, torch)
        keys = torch.empty((B, D), device=dev, dtype=torch.int64)
        mask = torch.empty((B, D), device=dev, dtype=torch.int32)
        rank = torch.empty((B, D), device=dev, dtype=torch.int32)
        flags = torch.empty((B, D, A), device=dev, dtype=torch.int32)
        coco_match(scores, boxes, classes, tg, G, None, None, keys, rank, flags, npig)
        N.check(L.ssdk_apsweep_match(scores.data_ptr(), boxes.data_ptr(), classes.data_ptr(), B, D, tg.data_ptr(), G, C, CONF, thr, 10,
                                     N.AP_RULE["coco"], 100, keys.data_ptr(), mask.data_ptr(), npos.data_ptr(), N.stream_ptr(dev)),
                "apsweep_match")
        all_keys.append(keys.view(-1))
        all_rec.append(torch.cat([rank.view(-1, 1), flags.view(-1, A)], 1))
        all_mask.append(mask.view(-1))
    keys, rec, mask = torch.cat(all_keys), torch.cat(all_rec), torch.cat(all_mask)
    bounds = torch.arange(C + 1, device=dev, dtype=torch.int64) << 32
    out = torch.empty((2, A, len(MAX_DETS), 10, C), device=dev, dtype=torch.float64)
    ap_sweep = torch.empty((10, C), device=dev, dtype=torch.float64)

    def summary():
        skeys, order = torch.sort(keys, stable=True)
        seg = torch.searchsorted(skeys, bounds).contiguous()
        r = rec[order]
        rank_s, flags_s = r[:, 0].contiguous(), r[:, 1:].contiguous()
        N.check(L.ssdk_cocoeval_accumulate(flags_s.data_ptr(), rank_s.data_ptr(), seg.data_ptr(), npig.data_ptr(), C, 10, A, md,
                                           len(MAX_DETS), out[0].data_ptr(), out[1].data_ptr(), N.stream_ptr(dev)), "cocoeval_accumulate")

    def sweep_ap():
        skeys, order = torch.sort(keys, stable=True)
        seg = torch.searchsorted(skeys, bounds).contiguous()
        m = mask[order].contiguous()
        N.check(L.ssdk_apsweep_average_precision(m.data_ptr(), seg.data_ptr(), npos.data_ptr(), C, 10, N.AP_RULE["coco"],
                                                 ap_sweep.data_ptr(), N.stream_ptr(dev)), "apsweep_average_precision")

    fns = {"sort_and_cocoeval_accumulate": summary, "sort_and_apsweep_average_precision": sweep_ap}
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    # (the two APs need not agree on these inputs: the jitter turns some detections inside out, and a detection of negative area
    # lies outside [0, 1e10] -- ignored where unmatched under the summary's rule, a false positive under the sweep's; on boxes of
    # positive area the two agree to the bit, which tests/test_gpu_cocoeval.py asserts)
    times = {key: [] for key in fns}
    for _ in range(ROUNDS):
        for key, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(REPS):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[key].append(e0.elapsed_time(e1) * 1e3 / REPS)
    for key in fns:
        emit(dict(what="per epoch", side=key, records=int(keys.numel()), C=C, T=10, A=A, M=len(MAX_DETS),
                  AP_sweep=float(np.nanmean(ap_sweep.cpu().numpy())), AP=float(np.nanmean(out[0, 0, 2].cpu().numpy())),
                  AR100=float(np.nanmean(out[1, 0, 2].cpu().numpy())), **stats(times[key])))

    if args.out:
        with open(args.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
