"""Transposed 3x3 / stride 2 convolution of the Shelf training step: the kernels of csrc/ssdk_convttrain.hip against PyTorch-ROCm in
the same dtype, call by call -- prepare (against autocast's weight cast), forward + bias + skip (against aten.convolution, transposed,
followed by the add), input gradient, weight + bias gradient (aten.convolution_backward with those outputs asked for; and the weight
gradient alone, which prices the bias sum that rides on the pass) -- and the whole layer under autograd, forward + backward, on both
sides (``convttrain.convt3x3s2`` against ``F.conv_transpose2d(...) + skip``).
Per (shape, pass, side) a hipGraph of CALLS calls is captured and replayed REPS times between two device events, the sides of a pass
alternating, three rounds; one JSON line each with the median and the spread in us, the fraction of the 2.5 PFLOP/s matrix peak and
the algorithmic bytes.

Every (shape, dtype) runs in a child process of its own under a time limit; the first child that fails ends the run.

    python tools/convt_train_probe.py [--dtype bf16,fp16] [--cases 0,1] [--batch N] [--out FILE.jsonl] [--limit SECONDS]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "ssds.pytorch_amd")]

PEAK_FLOPS = 2.5e15  # MI355X dense bf16 / fp16 matrix peak

# name, Cin, Cout, H, W, N: the two decoder steps of shelf_resnet18_513.yml (each runs twice per forward) at the config's batch per GPU
CASES = [
    ("shelf decoder 17^2 -> 33^2", 512, 256, 17, 17, 32),
    ("shelf decoder 33^2 -> 65^2", 256, 128, 33, 33, 32),
]
CALLS, REPS, ROUNDS = 10, 5, 3


def _timed_graphs(fns):
    """fns: {key: callable}.  Each callable captured CALLS times into a graph; the graphs replayed alternating, ROUNDS rounds of
    REPS replays between two device events -> {key: sorted us per call}."""
    import torch

    graphs = {}
    side = torch.cuda.Stream()
    for key, fn in fns.items():
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):  # warm-up on a side stream, as torch.cuda.graph asks of autograd calls
            for _ in range(3):
                fn()
        torch.cuda.current_stream().wait_stream(side)
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


def run_case(ci, dtype_name, batch):
    """One (shape, dtype) on the current HIP device -> the JSON rows."""
    import torch
    import torch.nn.functional as F
    from ssds import _native as N
    from ssds.modeling.layers import convttrain as CT

    assert torch.cuda.is_available(), "convt_train_probe needs a HIP device"
    dtype = torch.bfloat16 if dtype_name == "bf16" else torch.float16
    code = N.BF16 if dtype_name == "bf16" else N.F16
    sp = N.stream_ptr
    name, cin, cout, h, w, n = CASES[ci]
    n = batch or n
    ho, wo = 2 * h - 1, 2 * w - 1
    x = torch.randn(n, cin, h, w, device="cuda").to(dtype)
    gy = torch.randn(n, cout, ho, wo, device="cuda").to(dtype)
    sk = torch.randn(n, cout, ho, wo, device="cuda").to(dtype)
    w32 = torch.randn(cin, cout, 3, 3, device="cuda") * (2.0 / (9 * cin)) ** 0.5
    w16 = w32.to(dtype)
    b32 = torch.randn(cout, device="cuda")
    b16 = b32.to(dtype)
    fwd, dg = CT.prepare_images(w32, dtype)
    y, gx, gw, gb = torch.empty_like(gy), torch.empty_like(x), torch.empty_like(w32), torch.empty_like(b32)
    need = int(N.lib.ssdk_convt_train_wgrad_workspace_bytes(n, cin, cout, h, w))
    ws = torch.empty(need + 16, dtype=torch.uint8, device="cuda")
    wsp = (ws.data_ptr() + 15) & ~15
    dev = x.device
    conv_args = ([2, 2], [1, 1], [1, 1], True, [0, 0], 1)
    xg, skg = x.clone().requires_grad_(True), sk.clone().requires_grad_(True)
    wg, bg = w32.clone().requires_grad_(True), b32.clone().requires_grad_(True)

    def layer_ssdk():
        yy = CT.convt3x3s2(xg, wg, bg, skg)
        torch.autograd.grad(yy, (xg, wg, bg, skg), gy)

    def layer_torch():  # what the module path runs under autocast: the weight cast, the library's three passes, the add
        with torch.autocast("cuda", dtype=dtype):
            yy = F.conv_transpose2d(xg, wg, bg, 2, 1) + skg
        torch.autograd.grad(yy, (xg, wg, bg, skg), gy)

    fns = {
        ("prepare", "ssdk"): lambda: N.check(N.lib.ssdk_convt_train_prepare(
            w32.data_ptr(), fwd.data_ptr(), dg.data_ptr(), cin, cout, code, sp(dev)), "prepare"),
        ("prepare", "torch"): lambda: w32.to(dtype),  # autocast's cast of the parameter
        ("forward", "ssdk"): lambda: N.check(N.lib.ssdk_convt_train_forward(
            x.data_ptr(), fwd.data_ptr(), b32.data_ptr(), sk.data_ptr(), y.data_ptr(), n, cin, cout, h, w, code, sp(dev)), "forward"),
        ("forward", "torch"): lambda: torch.ops.aten.convolution(x, w16, b16, *conv_args) + sk,
        ("dgrad", "ssdk"): lambda: N.check(N.lib.ssdk_convt_train_dgrad(
            gy.data_ptr(), dg.data_ptr(), gx.data_ptr(), n, cin, cout, h, w, code, sp(dev)), "dgrad"),
        ("dgrad", "torch"): lambda: torch.ops.aten.convolution_backward(gy, x, w16, None, *conv_args, [True, False, False]),
        ("wgrad", "ssdk"): lambda: N.check(N.lib.ssdk_convt_train_wgrad(
            x.data_ptr(), gy.data_ptr(), gw.data_ptr(), gb.data_ptr(), wsp, need, n, cin, cout, h, w, code, sp(dev)), "wgrad"),
        ("wgrad without gb", "ssdk"): lambda: N.check(N.lib.ssdk_convt_train_wgrad(
            x.data_ptr(), gy.data_ptr(), gw.data_ptr(), None, wsp, need, n, cin, cout, h, w, code, sp(dev)), "wgrad"),
        ("wgrad without gb", "torch"): lambda: torch.ops.aten.convolution_backward(gy, x, w16, None, *conv_args, [False, True, False]),
        ("wgrad", "torch"): lambda: torch.ops.aten.convolution_backward(gy, x, w16, [cout], *conv_args, [False, True, True]),
        ("forward+backward", "ssdk"): layer_ssdk,
        ("forward+backward", "torch"): layer_torch,
    }
    times = _timed_graphs(fns)
    macs = n * h * w * cin * cout * 9  # the taps that exist at the borders are a few less
    act = 2 * n * (cin * h * w + cout * ho * wo)
    skip_bytes = 2 * n * cout * ho * wo
    byt = {"prepare": cin * cout * 9 * (4 + 2 * 2), "forward": act + skip_bytes + 2 * cin * cout * 9, "dgrad": act + 2 * cin * cout * 9,
           "wgrad": act + 4 * cin * cout * 9, "wgrad without gb": act + 4 * cin * cout * 9, "forward+backward": 3 * act + skip_bytes + 8 * cin * cout * 9}
    nmac = {"prepare": 0, "forward": 1, "dgrad": 1, "wgrad": 1, "wgrad without gb": 1, "forward+backward": 3}
    rows = []
    for (what, side), t in times.items():
        med = t[len(t) // 2]
        rows.append({"case": name, "Cin": cin, "Cout": cout, "H": h, "W": w, "N": n, "dtype": dtype_name, "pass": what, "side": side,
                     "us_median": round(med, 2), "us_min": round(t[0], 2), "us_max": round(t[-1], 2), "algorithmic_bytes": byt[what],
                     "GBps": round(byt[what] / med / 1e3, 1), "fraction_of_peak": round(2 * macs * nmac[what] / (med * 1e-6) / PEAK_FLOPS, 4)})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="bf16,fp16", help="comma-separated: bf16, fp16")
    ap.add_argument("--out", default=None)
    ap.add_argument("--cases", default=None, help="comma-separated indices into CASES (default: all)")
    ap.add_argument("--batch", type=int, default=0, help="a batch size instead of the config's")
    ap.add_argument("--limit", type=int, default=240, help="seconds a (shape, dtype) child may take")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)  # CASE,DTYPE: run it in this process, print its rows
    args = ap.parse_args()
    if args.child:
        ci, dtype_name = args.child.split(",")
        for row in run_case(int(ci), dtype_name, args.batch):
            print("ROW " + json.dumps(row), flush=True)
        return 0
    out = open(args.out, "w") if args.out else None
    picked = range(len(CASES)) if args.cases is None else [int(v) for v in args.cases.split(",")]
    for ci in picked:
        for dtype_name in args.dtype.split(","):
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "%d,%s" % (ci, dtype_name), "--batch", str(args.batch)]
            try:
                res = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
            except subprocess.TimeoutExpired:
                print("case %d %s: no result within %d s -- stopping" % (ci, dtype_name, args.limit), file=sys.stderr)
                return 124
            if res.returncode != 0:
                print("case %d %s: exit status %d -- stopping\n%s" % (ci, dtype_name, res.returncode, res.stderr[-3000:]), file=sys.stderr)
                return res.returncode if res.returncode > 0 else 1
            for line in res.stdout.splitlines():
                if line.startswith("ROW "):
                    print(line[4:], flush=True)
                    if out:
                        out.write(line[4:] + "\n")
                        out.flush()
    if out:
        out.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
