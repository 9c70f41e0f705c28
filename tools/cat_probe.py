"""``ssdk_cat2`` / ``ssdk_spp`` (csrc/ssdk_cat.hip: the channel concatenation with an optional nearest x2 upsample, and the SPP block of
the YOLO necks) against the expressions they replace on PyTorch-ROCm, on the same channels_last tensors of the same dtype:

    torch.cat((a, F.interpolate(b, scale_factor=2)), 1)        torch.cat((a, b), 1)
    torch.cat([x] + [F.max_pool2d(x, k, stride=1, padding=k // 2) for k in (5, 9, 13)], 1)

Per shape a hipGraph of CALLS calls of each is captured after warm-up and replayed REPS times between two device events (a window
of CALLS x REPS launches: milliseconds, against a timer resolution of microseconds), ROUNDS rounds ALTERNATING kernel and
expression; one JSON line per (op, shape, dtype) with the median and the spread in us of both, whether the outputs are the same
bits, and the algorithmic bytes of the op (every source and the output once) with the bandwidth they amount to as a share of the
8 TB/s HBM peak (of which a float4 copy reaches 79 %).

    python tools/cat_probe.py [--dtype bf16] [--cases 0,1] [--out FILE.jsonl]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "ssds.pytorch_amd")]

PEAK_BYTES = 8.0e12  # HBM3E

# the ops of experiments/cfgs/yolov3_resnet18_320.yml (maps 40 / 20 / 10: two top-down concatenations) and of
# yolov4_resnet18_512.yml (maps 64 / 32 / 16: SPP on 16 x 16 x 256, two top-down and two bottom-up concatenations), at the configs'
# batch 32 and at batch 1
#        op     H   W   C1   C2   up2            op     H   W   C
_OPS = [("cat", 20, 20, 256, 128, True), ("cat", 40, 40, 128, 64, True),
        ("cat", 32, 32, 128, 128, True), ("cat", 64, 64, 64, 64, True), ("cat", 32, 32, 128, 128, False),
        ("cat", 16, 16, 256, 256, False), ("spp", 16, 16, 256)]
CASES = [(op[0], n) + op[1:] for n in (32, 1) for op in _OPS]
CALLS, REPS, ROUNDS = 10, 20, 5


def _timed_graphs(fns):
    import torch

    graphs = {}
    for key, fn in fns.items():
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(CALLS):
                fn()
        g.replay()
        torch.cuda.synchronize()
        graphs[key] = g
    times = {key: [] for key in fns}
    for _ in range(ROUNDS):
        for key in fns:  # kernel, expression, kernel, expression, ...
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(REPS):
                graphs[key].replay()
            e1.record()
            torch.cuda.synchronize()
            times[key].append(e0.elapsed_time(e1) * 1e3 / (CALLS * REPS))
    return {key: sorted(t) for key, t in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp16"])
    ap.add_argument("--cases", default=None, help="comma-separated indices into CASES (default: all)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import torch.nn.functional as F
    from ssds.modeling.layers import fused_conv as FC

    assert torch.cuda.is_available(), "cat_probe needs a HIP device"
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float16
    cl = lambda t: t.to(dtype).contiguous(memory_format=torch.channels_last)
    out = open(args.out, "w") if args.out else None
    for ci in (range(len(CASES)) if args.cases is None else [int(v) for v in args.cases.split(",")]):
        case = CASES[ci]
        torch.manual_seed(ci)
        with torch.no_grad():
            if case[0] == "cat":
                _, n, h, w, c1, c2, up2 = case
                a = cl(torch.randn(n, c1, h, w, device="cuda"))
                b = cl(torch.randn((n, c2, h // 2, w // 2) if up2 else (n, c2, h, w), device="cuda"))
                y = torch.empty((n, c1 + c2, h, w), device="cuda", dtype=dtype).contiguous(memory_format=torch.channels_last)
                kernel = lambda: FC.cat_native(a, b, up2=up2, y=y)
                if up2:
                    library = lambda: torch.cat((a, F.interpolate(b, scale_factor=2)), 1)
                else:
                    library = lambda: torch.cat((a, b), 1)
                byt = 2 * (a.numel() + b.numel() + y.numel())
                shape = {"op": "cat", "N": n, "H": h, "W": w, "C1": c1, "C2": c2, "mode": "up2" if up2 else "same"}
            else:
                _, n, h, w, c = case
                x = cl(torch.randn(n, c, h, w, device="cuda") - 3.0)
                y = torch.empty((n, 4 * c, h, w), device="cuda", dtype=dtype).contiguous(memory_format=torch.channels_last)
                kernel = lambda: FC.spp_native(x, y=y)
                library = lambda: torch.cat([x] + [F.max_pool2d(x, k, stride=1, padding=k // 2) for k in (5, 9, 13)], 1)
                byt = 2 * (x.numel() + y.numel())
                shape = {"op": "spp", "N": n, "H": h, "W": w, "C": c}
            same = bool(torch.equal(kernel(), library()))
            times = _timed_graphs({"kernel": kernel, "library": library})
        k, l = times["kernel"], times["library"]
        med, lmed = k[len(k) // 2], l[len(l) // 2]
        row = dict(shape, dtype=args.dtype, same_bits=same,
                   kernel_us_median=round(med, 2), kernel_us_min=round(k[0], 2), kernel_us_max=round(k[-1], 2),
                   library_us_median=round(lmed, 2), library_us_min=round(l[0], 2), library_us_max=round(l[-1], 2),
                   speedup=round(lmed / med, 2), algorithmic_bytes=byt, GBps=round(byt / med / 1e3, 1),
                   fraction_of_hbm_peak=round(byt / (med * 1e-6) / PEAK_BYTES, 4))
        line = json.dumps(row)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()
    if out:
        out.close()


if __name__ == "__main__":
    main()
