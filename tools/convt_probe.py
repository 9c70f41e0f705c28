"""``ssdk_convt3x3s2`` (csrc/ssdk_convt.hip: transposed 3x3 / stride 2 / pad 1 convolution + bias + skip, the decoder step of the
Shelf neck) against the expression it replaces, ``F.conv_transpose2d(x, w, b, stride=2, padding=1) + skip`` on channels_last
tensors of the same dtype on PyTorch-ROCm.  Per shape a hipGraph of CALLS calls of each is captured and replayed REPS times
between two device events, three rounds; one JSON line per shape with the median and the spread in us of both, the
algorithmic bytes of the step (x, skip, y and the weights once) with the bandwidth they amount to as a fraction of the 8 TB/s
HBM peak, and the fraction of the 2.5 PFLOP/s matrix peak.

    python tools/convt_probe.py [--dtype bf16] [--cases 0,1] [--out FILE.jsonl]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "ssds.pytorch_amd")]

PEAK_FLOPS = 2.5e15  # MI355X dense bf16 / fp16 matrix peak
PEAK_BYTES = 8.0e12  # HBM3E

# N, Cin, Cout, H, W: the two decoder steps of experiments/cfgs/shelf_resnet18_513.yml (17 -> 33 and 33 -> 65) at batch 32 and at
# batch 1, a wider / larger map, and the steps of the golden ResNet18 case (tests/golden/cases_shelf.py)
CASES = [(32, 512, 256, 17, 17), (32, 256, 128, 33, 33), (1, 512, 256, 17, 17), (1, 256, 128, 33, 33), (8, 128, 64, 65, 65),
         (2, 512, 256, 5, 4), (2, 256, 128, 9, 7)]
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
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp16"])
    ap.add_argument("--cases", default=None, help="comma-separated indices into CASES (default: all)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import torch.nn.functional as F
    from ssds.modeling.layers import fused_conv as FC

    assert torch.cuda.is_available(), "convt_probe needs a HIP device"
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float16
    out = open(args.out, "w") if args.out else None
    for ci in (range(len(CASES)) if args.cases is None else [int(v) for v in args.cases.split(",")]):
        n, cin, cout, h, w = CASES[ci]
        ho, wo = 2 * h - 1, 2 * w - 1
        torch.manual_seed(ci)
        m = torch.nn.ConvTranspose2d(cin, cout, 3, stride=2, padding=1).cuda()
        pk = FC.ConvTPack(m, dtype)
        wt = m.weight.detach().to(dtype).contiguous(memory_format=torch.channels_last)
        b = m.bias.detach().to(dtype)
        x = torch.randn(n, cin, h, w, device="cuda").to(dtype).contiguous(memory_format=torch.channels_last)
        skip = torch.randn(n, cout, ho, wo, device="cuda").to(dtype).contiguous(memory_format=torch.channels_last)
        y = torch.empty_like(skip)
        with torch.no_grad():
            got = FC.convt_native(x, pk, skip, y=y).float()
            lib = (F.conv_transpose2d(x, wt, b, stride=2, padding=1) + skip).float()
            err = float((got - lib).abs().max()) / max(float(lib.abs().max()), 1e-6)
            fns = {"kernel": lambda: FC.convt_native(x, pk, skip, y=y),
                   "library": lambda: F.conv_transpose2d(x, wt, b, stride=2, padding=1) + skip}
            times = _timed_graphs(fns)
        macs = n * cin * cout * (h * w + 2 * h * (w - 1) + 2 * (h - 1) * w + 4 * (h - 1) * (w - 1))
        byt = 2 * (n * (h * w * cin + 2 * ho * wo * cout) + 9 * cin * cout) + 4 * cout
        k, l = times["kernel"], times["library"]
        med = k[len(k) // 2]
        row = {"N": n, "Cin": cin, "Cout": cout, "H": h, "W": w, "dtype": args.dtype,
               "kernel_us_median": round(med, 2), "kernel_us_min": round(k[0], 2), "kernel_us_max": round(k[-1], 2),
               "library_us_median": round(l[len(l) // 2], 2), "library_us_min": round(l[0], 2), "library_us_max": round(l[-1], 2),
               "speedup": round(l[len(l) // 2] / med, 2), "max_abs_diff_over_max": round(err, 5),
               "algorithmic_bytes": byt, "GBps": round(byt / med / 1e3, 1),
               "fraction_of_hbm_peak": round(byt / (med * 1e-6) / PEAK_BYTES, 4),
               "fraction_of_matrix_peak": round(2 * macs / (med * 1e-6) / PEAK_FLOPS, 4)}
        line = json.dumps(row)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
    if out:
        out.close()


if __name__ == "__main__":
    main()
