"""Dense 3x3 convolution of the training step: the kernels of csrc/ssdk_conv3train.hip against PyTorch-ROCm's convolution (MIOpen)
in the same dtype, channels-first, pass by pass (prepare, forward, input gradient, weight gradient:
aten.convolution / aten.convolution_backward with one output asked for), and for the shapes under ``extras`` also against the
im2col path (pointwise.NativeConv3x3: forward, and backward as a whole).  Per (shape, pass, side) a hipGraph of CALLS calls is
captured and replayed REPS times between two device events, the sides of a pass alternating, three rounds; one JSON line each
with the median and the spread in us, the fraction of the 2.5 PFLOP/s bf16 peak and the algorithmic bytes.

    python tools/conv3_probe.py [--dtype bf16] [--cases 0,1] [--batch N] [--out FILE.jsonl]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "ssds.pytorch_amd")]

PEAK_FLOPS = 2.5e15  # MI355X dense bf16 / fp16 matrix peak

# name, Cin, Cout, stride, H, W, N (the config's batch per GPU), bias, under extras
CASES = [
    ("fpn tower 80^2", 256, 256, 1, 80, 80, 32, False, False),
    ("bifpn tower 112^2", 256, 256, 1, 112, 112, 16, False, False),
    ("fpn tower 40^2", 256, 256, 1, 40, 40, 32, False, False),
    ("fpn tower 20^2", 256, 256, 1, 20, 20, 32, False, False),
    ("fpn tower 10^2", 256, 256, 1, 10, 10, 32, False, False),
    ("fpn tower 5^2", 256, 256, 1, 5, 5, 32, False, False),
    ("bifpn tower 56^2", 256, 256, 1, 56, 56, 16, False, False),
    ("bifpn tower 28^2", 256, 256, 1, 28, 28, 16, False, False),
    ("bifpn tower 14^2", 256, 256, 1, 14, 14, 16, False, False),
    ("bifpn tower 7^2", 256, 256, 1, 7, 7, 16, False, False),
    ("head loc 80^2", 256, 36, 1, 80, 80, 32, True, False),
    ("head conf 80^2", 256, 720, 1, 80, 80, 32, True, False),
    ("resnet layer1", 64, 64, 1, 160, 160, 32, False, False),
    ("resnet layer2", 128, 128, 1, 80, 80, 32, False, False),
    ("resnet layer2 s2", 128, 128, 2, 160, 160, 32, False, False),
    ("resnet layer4", 512, 512, 1, 20, 20, 32, False, False),
    ("resnet layer4 s2", 512, 512, 2, 40, 40, 32, False, False),
    ("fpn extra 2048->256 s2", 2048, 256, 2, 20, 20, 32, False, True),
    ("fpn extra 256->256 s2", 256, 256, 2, 10, 10, 32, False, True),
    ("bifpn extra 912->256 s2", 912, 256, 2, 28, 28, 16, False, True),
    ("bifpn extra 256->256 s2", 256, 256, 2, 14, 14, 16, False, True),
]
CALLS, REPS, ROUNDS = 10, 5, 3


def _timed_graphs(fns):
    """fns: {key: callable}.  Each callable captured CALLS times into a graph; the graphs replayed alternating, ROUNDS rounds of
    REPS replays between two device events -> {key: sorted us per call}."""
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
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp16"])
    ap.add_argument("--out", default=None)
    ap.add_argument("--cases", default=None, help="comma-separated indices into CASES (default: all)")
    ap.add_argument("--batch", type=int, default=0, help="a batch size instead of the configs'")
    args = ap.parse_args()
    import torch
    import torch.nn as nn
    from ssds import _native as N
    from ssds.modeling.layers import denseconv as D
    from ssds.modeling.layers import pointwise as P

    assert torch.cuda.is_available(), "conv3_probe needs a HIP device"
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float16
    code = N.BF16 if args.dtype == "bf16" else N.F16
    sp = N.stream_ptr
    out = open(args.out, "w") if args.out else None
    picked = range(len(CASES)) if args.cases is None else [int(v) for v in args.cases.split(",")]
    for ci in picked:
        name, cin, cout, stride, h, w, n, bias, extras = CASES[ci]
        n = args.batch or n
        ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
        x = torch.randn(n, cin, h, w, device="cuda").to(dtype)
        dy = torch.randn(n, cout, ho, wo, device="cuda").to(dtype)
        w32 = torch.randn(cout, cin, 3, 3, device="cuda") * (2.0 / (9 * cin)) ** 0.5
        w16 = w32.to(dtype)
        b32 = torch.randn(cout, device="cuda") if bias else None
        b16 = None if b32 is None else b32.to(dtype)
        fwd, dg = D.prepare_images(w32, dtype)
        y, dx, dw = torch.empty_like(dy), torch.empty_like(x), torch.empty_like(w32)
        need = int(N.lib.ssdk_conv3x3_train_wgrad_workspace_bytes(n, cin, cout, h, w, stride))
        ws = torch.empty(need + 16, dtype=torch.uint8, device="cuda")
        wsp = (ws.data_ptr() + 15) & ~15
        dev = x.device
        conv_args = ([stride, stride], [1, 1], [1, 1], False, [0, 0], 1)
        bp = None if b32 is None else b32.data_ptr()
        fns = {
            ("forward", "ssdk"): lambda: N.check(N.lib.ssdk_conv3x3_train_forward(
                x.data_ptr(), fwd.data_ptr(), bp, y.data_ptr(), n, cin, cout, h, w, stride, code, sp(dev)), "forward"),
            ("forward", "miopen"): lambda: torch.ops.aten.convolution(x, w16, b16, *conv_args),
            ("dgrad", "ssdk"): lambda: N.check(N.lib.ssdk_conv3x3_train_dgrad(
                dy.data_ptr(), dg.data_ptr(), dx.data_ptr(), n, cin, cout, h, w, stride, code, sp(dev)), "dgrad"),
            ("dgrad", "miopen"): lambda: torch.ops.aten.convolution_backward(dy, x, w16, None, *conv_args, [True, False, False]),
            ("wgrad", "ssdk"): lambda: N.check(N.lib.ssdk_conv3x3_train_wgrad(
                x.data_ptr(), dy.data_ptr(), dw.data_ptr(), wsp, need, n, cin, cout, h, w, stride, code, sp(dev)), "wgrad"),
            ("wgrad", "miopen"): lambda: torch.ops.aten.convolution_backward(dy, x, w16, None, *conv_args, [False, True, False]),
            ("prepare", "ssdk"): lambda: N.check(N.lib.ssdk_conv3x3_train_prepare(
                w32.data_ptr(), fwd.data_ptr(), dg.data_ptr(), cin, cout, code, sp(dev)), "prepare"),
            ("prepare", "miopen"): lambda: w32.to(dtype),  # autocast's cast of the parameter
        }
        if extras:
            m = P.use_native_conv3x3(nn.Sequential(nn.Conv2d(cin, cout, 3, stride, 1, bias=bias)))[0].cuda()
            xg = x.clone().requires_grad_(True)

            def im2col_fwd():
                with torch.autocast("cuda", dtype=dtype):
                    return m(x)

            def im2col_step():  # forward + both gradients: the path has no separate passes
                with torch.autocast("cuda", dtype=dtype):
                    yy = m(xg)
                torch.autograd.grad(yy, (xg, m.weight), dy)

            fns[("forward", "im2col")] = im2col_fwd
            fns[("forward+dgrad+wgrad", "im2col")] = im2col_step
        times = _timed_graphs(fns)
        macs = n * ho * wo * cin * cout * 9
        act = 2 * n * (cin * h * w + cout * ho * wo)
        byt = {"forward": act + 2 * cin * cout * 9, "dgrad": act + 2 * cin * cout * 9, "wgrad": act + 4 * cin * cout * 9,
               "prepare": cin * cout * 9 * (4 + 2 * 2), "forward+dgrad+wgrad": 3 * act + 8 * cin * cout * 9}
        nmac = {"forward": 1, "dgrad": 1, "wgrad": 1, "prepare": 0, "forward+dgrad+wgrad": 3}
        for (what, side), t in times.items():
            med = t[len(t) // 2]
            row = {"case": name, "Cin": cin, "Cout": cout, "H": h, "W": w, "stride": stride, "N": n, "dtype": args.dtype, "pass": what,
                   "side": side, "us_median": round(med, 2), "us_min": round(t[0], 2), "us_max": round(t[-1], 2),
                   "algorithmic_bytes": byt[what], "GBps": round(byt[what] / med / 1e3, 1),
                   "fraction_of_peak": round(2 * macs * nmac[what] / (med * 1e-6) / PEAK_FLOPS, 4)}
            line = json.dumps(row)
            print(line, flush=True)
            if out:
                out.write(line + "\n")
                out.flush()
    if out:
        out.close()


if __name__ == "__main__":
    main()
