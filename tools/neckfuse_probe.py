"""The neck operations of the training step: the kernels of csrc/ssdk_necktrain.hip against the eager torch expression in the same
dtype, per (operation, shape, pass): the FPN top-down upsample-add, the BiFPN top-down and bottom-up weighted fusions and the ResNet
stem's max-pool, forward and backward, at the configs' own shapes and per-GPU batch.  Per (case, pass, side) a hipGraph of CALLS calls
is captured and replayed REPS times between two device events, the sides of a pass alternating, three rounds; one JSON line each with
the median and the spread in us, the algorithmic bytes and the fraction of the 8 TB/s HBM peak.

The eager backward is ``torch.autograd.grad`` through the graph of the eager expression (all tensor gradients and the gradient of the
[K, L] weight parameter); the native backward is one ``ssdk_neck_fuse_bwd`` call (+ its weight-gradient launch).

    python tools/neckfuse_probe.py [--dtype bf16] [--cases 0,1] [--batch N] [--out FILE.jsonl]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "ssds.pytorch_amd")]

PEAK_HBM = 8.0e12  # MI355X HBM3E peak, bytes / s

# name, kind, C, H (= W) of the output, N (the config's batch per GPU).  kinds: "fpn_up" lateral + up(x); "bifpn_up" w0 a + w1 up(b);
# "bifpn_pool_skip" w0 a + w1 pool(b) + w2 skip; "bifpn_pool" w0 a + w1 pool(b); "pool" max_pool2d(3, 2, 1) of an H x H input
CASES = [
    ("fpn top-down 80^2", "fpn_up", 256, 80, 32),
    ("fpn top-down 40^2", "fpn_up", 256, 40, 32),
    ("bifpn top-down 112^2", "bifpn_up", 256, 112, 16),
    ("bifpn top-down 56^2", "bifpn_up", 256, 56, 16),
    ("bifpn top-down 28^2", "bifpn_up", 256, 28, 16),
    ("bifpn top-down 14^2", "bifpn_up", 256, 14, 16),
    ("bifpn bottom-up 56^2", "bifpn_pool_skip", 256, 56, 16),
    ("bifpn bottom-up 28^2", "bifpn_pool_skip", 256, 28, 16),
    ("bifpn bottom-up 14^2", "bifpn_pool_skip", 256, 14, 16),
    ("bifpn bottom-up 7^2", "bifpn_pool", 256, 7, 16),
    ("resnet stem pool 320^2", "pool", 64, 320, 32),
]
CALLS, REPS, ROUNDS = 10, 5, 3


def _timed_graphs(fns, stream):
    """fns: {key: callable}.  Each callable captured CALLS times into a graph on ``stream`` -- the stream the forward passes whose
    autograd graphs the backward callables walk were recorded on: the autograd engine runs a backward node on its forward's stream,
    which has to be the capturing one; the graphs replayed alternating, ROUNDS rounds of REPS replays between two device events
    -> {key: sorted us per call}."""
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
    ap.add_argument("--batch", type=int, default=0, help="a batch size instead of the configs'")
    args = ap.parse_args()
    import torch
    import torch.nn.functional as F
    from ssds.modeling.layers import neckfuse as NF

    assert torch.cuda.is_available(), "neckfuse_probe needs a HIP device"
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float16
    out = open(args.out, "w") if args.out else None
    picked = range(len(CASES)) if args.cases is None else [int(v) for v in args.cases.split(",")]
    stream = torch.cuda.Stream()
    for ci in picked:
        name, kind, c, h, n = CASES[ci]
        n = args.batch or n
        torch.cuda.synchronize()

        def act(*shape):
            return torch.relu(torch.randn(*shape, device="cuda")).to(dtype).requires_grad_(True)

        if kind == "pool":
            x = act(n, c, h, h)
            gy = torch.randn(n, c, h // 2, h // 2, device="cuda").to(dtype)
            with torch.cuda.stream(stream):
                y_e, y_n = F.max_pool2d(x, 3, 2, 1), NF.maxpool3x3s2(x)
            fns = {
                ("forward", "ssdk"): lambda: NF.maxpool3x3s2(x.detach()),
                ("forward", "eager"): lambda: F.max_pool2d(x.detach(), 3, 2, 1),
                ("backward", "ssdk"): lambda: torch.autograd.grad(y_n, (x,), gy, retain_graph=True),
                ("backward", "eager"): lambda: torch.autograd.grad(y_e, (x,), gy, retain_graph=True),
            }
            e_in, e_out = n * c * h * h, n * c * (h // 2) ** 2
            byt = {"forward": 2 * (e_in + e_out), "backward": 2 * (e_in + e_out + e_in)}
        else:
            a = act(n, c, h, h)
            gy = torch.randn(n, c, h, h, device="cuda").to(dtype)
            up = kind.endswith("_up")
            b = act(n, c, h // 2, h // 2) if up else act(n, c, 2 * h, 2 * h)
            skip = act(n, c, h, h) if kind == "bifpn_pool_skip" else None
            mode_b = NF.UP2 if up else NF.POOL2
            srcs = [a, b] + ([] if skip is None else [skip])
            if kind == "fpn_up":
                wp = wn = None
                eager = lambda: F.interpolate(b, scale_factor=2, mode="nearest") + a  # noqa: E731
                native = lambda: NF.neck_fuse(a, b, mode_b=NF.UP2)  # noqa: E731
                leaves = srcs
            else:
                wp = torch.full((len(srcs), 5), 0.5, device="cuda", requires_grad=True)  # the module's parameter

                def weights():
                    w = F.relu(wp)
                    return w / (torch.sum(w, dim=0) + 1e-6)

                def eager():
                    w = weights().to(dtype)
                    rb = F.interpolate(b, scale_factor=2, mode="nearest") if up else F.max_pool2d(b, kernel_size=2)
                    y = w[0, 2] * a + w[1, 2] * rb
                    return y if skip is None else y + w[2, 2] * skip

                def native():
                    return NF.neck_fuse(a, b, skip, weights(), 2, mode_b, NF.SAME)

                leaves = srcs + [wp]
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
            e_src = sum(t.numel() for t in srcs)
            e_out = a.numel()
            # backward: gy + every source (weight gradient, arg-max) read, every source's gradient written; without weights the
            # sources are not read and ga is gy itself
            byt = {"forward": 2 * (e_src + e_out), "backward": 2 * (e_out + 2 * e_src) if wp is not None else 2 * (e_out + b.numel())}
        torch.cuda.synchronize()
        times = _timed_graphs(fns, stream)
        for (what, side), t in times.items():
            med = t[len(t) // 2]
            row = {"case": name, "kind": kind, "C": c, "H": h, "W": h, "N": n, "dtype": args.dtype, "pass": what, "side": side,
                   "us_median": round(med, 2), "us_min": round(t[0], 2), "us_max": round(t[-1], 2), "algorithmic_bytes": byt[what],
                   "GBps": round(byt[what] / med / 1e3, 1), "fraction_of_hbm_peak": round(byt[what] / (med * 1e-6) / PEAK_HBM, 4)}
            line = json.dumps(row)
            print(line, flush=True)
            if out:
                out.write(line + "\n")
                out.flush()
        del fns, times
        torch.cuda.empty_cache()
    if out:
        out.close()


if __name__ == "__main__":
    main()
