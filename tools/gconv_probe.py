"""Grouped 3x3 convolution: gconv3x3_any_kernel against its 16-wide sibling (gconv3x3_g16_tile_kernel) on tensors of the
same N, C, H, W and stride -- both move the same algorithmic bytes (input once + output once + weights), so the figure is
bytes / kernel time.  Per case a hipGraph of CALLS launches is captured and replayed REPS times between two device events,
the widths of a case alternating, three rounds; prints one JSON line per (case, width) with the median and the spread.

    python tools/gconv_probe.py [--batch 16] [--dtype bf16] [--out FILE]

--train: the TRAINING kernels (csrc/ssdk_gconvtrain.hip) instead -- forward, input gradient and weight gradient of every
(case, width) on NCHW tensors against PyTorch-ROCm's grouped convolution (MIOpen) in the same dtype, channels-first, pass by
pass (aten.convolution / aten.convolution_backward with one output asked for), the two sides alternating, three rounds; one JSON
line per (case, width, pass, side).  --out then writes JSON lines.

    python tools/gconv_probe.py --train [--batch 16] [--dtype bf16] [--out FILE.jsonl]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "ssds.pytorch_amd")]

# C, H, W, stride, widths (16 first: the yardstick)
CASES = [
    (128, 56, 56, 1, (16, 4, 8, 32, 64)),     # ResNeXt50 layer1 shape at 224 px
    (192, 56, 56, 1, (16, 24, 48)),           # 12 x 16 | 8 x 24 | 4 x 48
    (192, 112, 112, 2, (16, 24, 48)),
    (672, 28, 28, 1, (16, 24, 56, 112, 168)),  # 42 x 16 | 28 x 24 | 12 x 56 | 6 x 112 | 4 x 168
    (672, 56, 56, 2, (16, 24, 56, 112, 168)),
    (1920, 14, 14, 1, (16, 40, 120, 128)),    # RegNetX080 stage 4 width
    (408, 56, 56, 1, (24,)),                  # RegNetX016 stage 3 at 896 px (17 groups: a partial run)
    (912, 28, 28, 1, (24,)),                  # ... stage 4
]
CALLS, REPS, ROUNDS = 20, 10, 3


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


def train(args):
    import torch
    from ssds import _native as N
    from ssds.modeling.layers import groupedconv as G

    assert torch.cuda.is_available(), "gconv_probe needs a HIP device"
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float16
    code = N.BF16 if args.dtype == "bf16" else N.F16
    sp = N.stream_ptr
    out = open(args.out, "w") if args.out else None
    picked = range(len(CASES)) if args.cases is None else [int(v) for v in args.cases.split(",")]
    for ci in picked:
        c, h, w, stride, widths = CASES[ci]
        n = args.batch
        ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
        x = torch.randn(n, c, h, w, device="cuda").to(dtype)
        dy = torch.randn(n, c, ho, wo, device="cuda").to(dtype)
        for gw in widths:
            groups = c // gw
            w32 = torch.randn(c, gw, 3, 3, device="cuda") * (2.0 / (9 * gw)) ** 0.5
            w16 = w32.to(dtype)
            fwd, dg = G.prepare_images(w32, groups, dtype)
            y, dx = torch.empty_like(dy), torch.empty_like(x)
            dw = torch.empty_like(w32)
            need = int(N.lib.ssdk_gconv3x3_train_wgrad_workspace_bytes(n, c, h, w, groups, stride))
            ws = torch.empty(need + 16, dtype=torch.uint8, device="cuda")
            wsp = (ws.data_ptr() + 15) & ~15
            dev = x.device
            conv_args = ([stride, stride], [1, 1], [1, 1], False, [0, 0], groups)
            fns = {
                ("forward", "ssdk"): lambda: N.check(N.lib.ssdk_gconv3x3_train_forward(
                    x.data_ptr(), fwd.data_ptr(), y.data_ptr(), n, c, h, w, groups, stride, code, sp(dev)), "forward"),
                ("forward", "miopen"): lambda: torch.ops.aten.convolution(x, w16, None, *conv_args),
                ("dgrad", "ssdk"): lambda: N.check(N.lib.ssdk_gconv3x3_train_dgrad(
                    dy.data_ptr(), dg.data_ptr(), dx.data_ptr(), n, c, h, w, groups, stride, code, sp(dev)), "dgrad"),
                ("dgrad", "miopen"): lambda: torch.ops.aten.convolution_backward(dy, x, w16, None, *conv_args, [True, False, False]),
                ("wgrad", "ssdk"): lambda: N.check(N.lib.ssdk_gconv3x3_train_wgrad(
                    x.data_ptr(), dy.data_ptr(), dw.data_ptr(), wsp, need, n, c, h, w, groups, stride, code, sp(dev)), "wgrad"),
                ("wgrad", "miopen"): lambda: torch.ops.aten.convolution_backward(dy, x, w16, None, *conv_args, [False, True, False]),
                ("prepare", "ssdk"): lambda: N.check(N.lib.ssdk_gconv3x3_train_prepare(
                    w32.data_ptr(), fwd.data_ptr(), dg.data_ptr(), c, groups, code, sp(dev)), "prepare"),
                ("prepare", "miopen"): lambda: w32.to(dtype),  # autocast's cast of the parameter
            }
            times = _timed_graphs(fns)
            # the bytes each pass must move (16-bit tensors once each + weights / the fp32 gradient) and its multiply-adds
            macs = n * ho * wo * c * gw * 9
            byt = {"forward": 2 * n * c * (h * w + ho * wo) + 2 * c * gw * 9, "dgrad": 2 * n * c * (h * w + ho * wo) + 2 * c * gw * 9,
                   "wgrad": 2 * n * c * (h * w + ho * wo) + 4 * c * gw * 9, "prepare": c * gw * 9 * (4 + 2 * 2)}
            for (what, side), t in times.items():
                med = t[len(t) // 2]
                row = {"C": c, "H": h, "W": w, "stride": stride, "N": n, "gw": gw, "dtype": args.dtype, "pass": what, "side": side,
                       "us_median": round(med, 2), "us_min": round(t[0], 2), "us_max": round(t[-1], 2),
                       "GBps": round(byt[what] / med / 1e3, 1),
                       "TFLOPs": 0.0 if what == "prepare" else round(2 * macs / med / 1e6, 2)}
                line = json.dumps(row)
                print(line, flush=True)
                if out:
                    out.write(line + "\n")
                    out.flush()
    if out:
        out.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp16"])
    ap.add_argument("--out", default=None)
    ap.add_argument("--train", action="store_true", help="time the training kernels against MIOpen, pass by pass")
    ap.add_argument("--cases", default=None, help="--train: comma-separated indices into CASES (default: all)")
    args = ap.parse_args()
    if args.train:
        return train(args)
    import torch
    import torch.nn as nn
    from ssds import _native as N
    from ssds.modeling.layers import fused_conv as FC

    assert torch.cuda.is_available(), "gconv_probe needs a HIP device"
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float16
    rows = []
    for c, h, w, stride, widths in CASES:
        x = torch.randn(args.batch, c, h, w, device="cuda").to(dtype).contiguous(memory_format=torch.channels_last)
        graphs, kernels = {}, {}
        for gw in widths:
            conv = nn.Conv2d(c, c, 3, stride, 1, groups=c // gw, bias=False).cuda()
            pack = FC.ConvPack(conv, nn.BatchNorm2d(c).cuda(), "relu", dtype)
            for _ in range(3):
                y = FC.conv_native(x, pack)
            kernels[gw] = N.last_kernel()
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                for _ in range(CALLS):
                    y = FC.conv_native(x, pack)
            g.replay()
            torch.cuda.synchronize()
            graphs[gw] = (g, pack, y)
        times = {gw: [] for gw in widths}
        for _ in range(ROUNDS):
            for gw in widths:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(REPS):
                    graphs[gw][0].replay()
                e1.record()
                torch.cuda.synchronize()
                times[gw].append(e0.elapsed_time(e1) * 1e3 / (CALLS * REPS))  # us per launch
        ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
        for gw in widths:
            t = sorted(times[gw])
            byt = 2 * (args.batch * c * (h * w + ho * wo) + c * gw * 9)
            macs = args.batch * ho * wo * c * gw * 9
            rows.append({"C": c, "H": h, "W": w, "stride": stride, "N": args.batch, "gw": gw, "dtype": args.dtype,
                         "kernel": kernels[gw], "us_median": round(t[len(t) // 2], 2), "us_min": round(t[0], 2),
                         "us_max": round(t[-1], 2), "GBps": round(byt / t[len(t) // 2] / 1e3, 1),
                         "TFLOPs": round(2 * macs / t[len(t) // 2] / 1e6, 2)})
            print(json.dumps(rows[-1]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"tool": "tools/gconv_probe.py", "calls_per_graph": CALLS, "replays": REPS, "rounds": ROUNDS,
                       "device": torch.cuda.get_device_name(0), "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
