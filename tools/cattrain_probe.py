"""The YOLO-only operations of the training step: the kernels of csrc/ssdk_cattrain.hip against the eager torch expression in the same
dtype, per (operation, shape, pass): the concatenations of yolov3_resnet18_320 and yolov4_resnet18_512 (``cat`` + ``interpolate``) and
the SPP block (3 x ``max_pool2d`` + ``cat``), forward and backward, at the configs' own shapes and batch 32.  Per (case, pass, side) a
hipGraph of CALLS calls is captured and replayed REPS times between two device events, the sides of a pass alternating, three rounds;
one JSON line each with the median and the spread in us, the algorithmic bytes and the fraction of the 8 TB/s HBM peak.

The eager backward is ``torch.autograd.grad`` through the graph of the eager expression; the native backward is one
``ssdk_cat_train_bwd`` / ``ssdk_spp_train_bwd`` call.

    python tools/cattrain_probe.py [--dtype bf16] [--cases 0,1] [--batch N] [--out FILE.jsonl]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "ssds.pytorch_amd")]

PEAK_HBM = 8.0e12  # MI355X HBM3E peak, bytes / s

# name, kind ("up2" | "same" | "spp"), C1 (spp: C), C2, H (= W) of the output
CASES = [
    ("yolov3 top-down 40^2", "up2", 128, 64, 40),
    ("yolov3 top-down 20^2", "up2", 256, 128, 20),
    ("yolov4 pan top-down 64^2", "up2", 64, 64, 64),
    ("yolov4 pan top-down 32^2", "up2", 128, 128, 32),
    ("yolov4 pan bottom-up 32^2", "same", 128, 128, 32),
    ("yolov4 pan bottom-up 16^2", "same", 256, 256, 16),
    ("yolov4 spp 16^2", "spp", 256, 0, 16),
]
BATCH = 32
CALLS, REPS, ROUNDS = 10, 5, 3


def _timed_graphs(fns, stream):
    """fns: {key: callable}.  Each callable captured CALLS times into a graph on ``stream`` (the stream the forward passes whose
    autograd graphs the backward callables walk were recorded on), the graphs replayed alternating, ROUNDS rounds of REPS replays
    between two device events -> {key: sorted us per call}."""
    import torch

    graphs = {}
    for key, fn in fns.items():
        with torch.cuda.stream(stream):
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=stream):
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
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp16"])
    ap.add_argument("--out", default=None)
    ap.add_argument("--cases", default=None, help="comma-separated indices into CASES (default: all)")
    ap.add_argument("--batch", type=int, default=BATCH)
    args = ap.parse_args()
    import torch
    import torch.nn.functional as F
    from ssds.modeling.layers import cattrain as CT

    assert torch.cuda.is_available(), "cattrain_probe needs a HIP device"
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float16
    out = open(args.out, "w") if args.out else None
    picked = range(len(CASES)) if args.cases is None else [int(v) for v in args.cases.split(",")]
    stream = torch.cuda.Stream()
    n = args.batch
    for ci in picked:
        name, kind, c1, c2, h = CASES[ci]
        torch.cuda.synchronize()

        def act(*shape):
            return torch.relu(torch.randn(*shape, device="cuda")).to(dtype).requires_grad_(True)

        if kind == "spp":
            x = act(n, c1, h, h)
            leaves = [x]
            gy = torch.randn(n, 4 * c1, h, h, device="cuda").to(dtype)
            eager = lambda: torch.cat([x] + [F.max_pool2d(x, kernel_size=k, stride=1, padding=k // 2) for k in (5, 9, 13)], dim=1)  # noqa: E731
            native = lambda: CT.spp(x)  # noqa: E731
            e_in, e_out = x.numel(), 4 * x.numel()
            byt = {"forward": 2 * (e_in + e_out), "backward": 2 * (e_in + e_out + e_in)}
        else:
            up = kind == "up2"
            a = act(n, c1, h, h)
            b = act(n, c2, h // 2, h // 2) if up else act(n, c2, h, h)
            leaves = [a, b]
            gy = torch.randn(n, c1 + c2, h, h, device="cuda").to(dtype)
            eager = lambda: torch.cat((a, F.interpolate(b, scale_factor=2, mode="nearest") if up else b), dim=1)  # noqa: E731
            native = lambda: CT.cat2(a, b, CT.UP2 if up else CT.SAME)  # noqa: E731
            e_src, e_out = a.numel() + b.numel(), gy.numel()
            byt = {"forward": 2 * (e_src + e_out), "backward": 2 * (e_out + e_src)}
        with torch.cuda.stream(stream):
            y_e, y_n = eager(), native()

        def no_grad(fn):
            def run():
                with torch.no_grad():
                    return fn()
            return run

        fns = {
            ("forward", "ssdk"): no_grad(native),
            ("forward", "eager"): no_grad(eager),
            ("backward", "ssdk"): lambda: torch.autograd.grad(y_n, leaves, gy, retain_graph=True),
            ("backward", "eager"): lambda: torch.autograd.grad(y_e, leaves, gy, retain_graph=True),
        }
        torch.cuda.synchronize()
        times = _timed_graphs(fns, stream)
        for (what, side), t in times.items():
            med = t[len(t) // 2]
            row = {"case": name, "kind": kind, "C1": c1, "C2": c2, "H": h, "W": h, "N": n, "dtype": args.dtype, "pass": what, "side": side,
                   "us_median": round(med, 2), "us_min": round(t[0], 2), "us_max": round(t[-1], 2), "algorithmic_bytes": byt[what],
                   "GBps": round(byt[what] / med / 1e3, 1), "fraction_of_hbm_peak": round(byt[what] / (med * 1e-6) / PEAK_HBM, 4)}
            line = json.dumps(row)
            print(line, flush=True)
            if out:
                out.write(line + "\n")
                out.flush()
        del fns, times, y_e, y_n
        torch.cuda.empty_cache()
    if out:
        out.close()


if __name__ == "__main__":
    main()
