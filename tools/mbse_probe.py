"""The three stages of ``ssdk_mbse`` (csrc/ssdk_mbse.hip: depthwise k x k + SiLU + pool partials, squeeze-excite gate, gated
projection) on the block shapes of EfficientNet-B0 @512, stage by stage and chained.  Per (shape, stage) a hipGraph of CALLS
calls is captured and replayed REPS times between two device events, three rounds; one JSON line each with the median and the
spread in us, the algorithmic bytes of the stage with the bandwidth they amount to (as a fraction of the 8 TB/s HBM peak) and,
for the projection, the fraction of the 2.5 PFLOP/s matrix peak.

    python tools/mbse_probe.py [--dtype fp16] [--batch 32] [--cases 0,1] [--out FILE.jsonl]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "ssds.pytorch_amd")]

PEAK_FLOPS = 2.5e15  # MI355X dense bf16 / fp16 matrix peak
PEAK_BYTES = 8.0e12  # HBM3E

# the distinct (C, Cout, k, stride, H = W of the depthwise input, residual) of B0's sixteen blocks at a 512 x 512 image, and how
# many blocks have that shape
CASES = [(32, 16, 3, 1, 256, False, 1), (96, 24, 3, 2, 256, False, 1), (144, 24, 3, 1, 128, True, 1), (144, 40, 5, 2, 128, False, 1),
         (240, 40, 5, 1, 64, True, 1), (240, 80, 3, 2, 64, False, 1), (480, 80, 3, 1, 32, True, 2), (480, 112, 5, 1, 32, False, 1),
         (672, 112, 5, 1, 32, True, 2), (672, 192, 5, 2, 32, False, 1), (1152, 192, 5, 1, 16, True, 3), (1152, 320, 3, 1, 16, False, 1)]
CALLS, REPS, ROUNDS = 10, 5, 3


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
        for key in fns:
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
    ap.add_argument("--dtype", default="fp16", choices=["bf16", "fp16"])
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--cases", default=None, help="comma-separated indices into CASES (default: all)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from ssds import _native as N
    from ssds.modeling.layers import fused_conv as FC
    from ssds.modeling.nets.efficientnet import MBConvBlock

    assert torch.cuda.is_available(), "mbse_probe needs a HIP device"
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float16
    out = open(args.out, "w") if args.out else None
    n = args.batch
    total = {"dw": 0.0, "gate": 0.0, "proj": 0.0, "all": 0.0}
    for ci in (range(len(CASES)) if args.cases is None else [int(v) for v in args.cases.split(",")]):
        c, cout, k, stride, h, residual, count = CASES[ci]
        cin = cout if residual else (c // 6 if c != 32 else 32)
        torch.manual_seed(ci)
        blk = MBConvBlock(cin, cout, c // cin, k, stride).eval().cuda()
        pk = FC.MbSePack(blk, dtype)
        assert (pk.cin, pk.cout, pk.residual) == (c, cout, residual), (pk.cin, pk.cout, pk.residual)
        ho = (h - 1) // stride + 1
        x = torch.randn(n, c, h, h, device="cuda").to(dtype).contiguous(memory_format=torch.channels_last)
        res = torch.randn(n, cout, ho, ho, device="cuda").to(dtype).contiguous(memory_format=torch.channels_last) if residual else None
        b = FC.mbse_native(x, pk, residual=res)
        kw = dict(t=b["t"], pool_partial=b["pool_partial"], gate=b["gate"], y=b["y"])
        fns = {"dw": lambda: FC.mbse_native(x, pk, stages=N.MBSE_DW, **kw),
               "gate": lambda: FC.mbse_native(x, pk, stages=N.MBSE_GATE, **kw),
               "proj": lambda: FC.mbse_native(x, pk, residual=res, stages=N.MBSE_PROJ, **kw),
               "all": lambda: FC.mbse_native(x, pk, residual=res, **kw)}
        times = _timed_graphs(fns)
        tiles = FC.mbse_pool_tiles(h, h, k, stride)
        byt = {"dw": 2 * n * c * (h * h + ho * ho) + 4 * n * tiles * c + 2 * k * k * c,
               "gate": 4 * (n * tiles * c + n * c + 2 * c * pk.r),
               "proj": 2 * n * ho * ho * (c + cout * (2 if residual else 1)) + 4 * n * c + 2 * c * cout}
        byt["all"] = 2 * n * (c * h * h + 2 * c * ho * ho + cout * ho * ho * (2 if residual else 1)) + 2 * c * (k * k + cout)
        macs = {"dw": n * ho * ho * k * k * c, "gate": 2 * n * c * pk.r, "proj": n * ho * ho * c * cout}
        macs["all"] = sum(macs.values())
        for what, t in times.items():
            med = t[len(t) // 2]
            total[what] += med * count
            row = {"C": c, "Cout": cout, "k": k, "stride": stride, "H": h, "N": n, "residual": residual, "blocks": count,
                   "dtype": args.dtype, "stage": what, "us_median": round(med, 2), "us_min": round(t[0], 2), "us_max": round(t[-1], 2),
                   "algorithmic_bytes": byt[what], "GBps": round(byt[what] / med / 1e3, 1),
                   "fraction_of_hbm_peak": round(byt[what] / (med * 1e-6) / PEAK_BYTES, 4),
                   "fraction_of_matrix_peak": round(2 * macs[what] / (med * 1e-6) / PEAK_FLOPS, 4)}
            line = json.dumps(row)
            print(line, flush=True)
            if out:
                out.write(line + "\n")
    line = json.dumps({"total_us_over_the_16_blocks": {k: round(v, 1) for k, v in total.items()}, "N": n, "dtype": args.dtype})
    print(line, flush=True)
    if out:
        out.write(line + "\n")
        out.close()


if __name__ == "__main__":
    main()
