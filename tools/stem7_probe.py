"""The 7x7 / stride-2 stem convolution of the training step: the kernels of csrc/ssdk_stem7train.hip against the parent routing --
``nn.Conv2d(3, 64, 7, 2, 3, bias=False)`` with its fp32 master weight under 16-bit autocast, i.e. the library convolution with the
cast of the parameter and the layout transposes it brings -- per (shape, dtype, pass): forward and weight gradient at 640 x 640,
batch 32 (fpn_resnet50_640 / fpn_resnext50_640) and 512 x 512, batch 64 (SSD on a ResNet).  After a warm-up the two sides of a pass
alternate, ROUNDS rounds of REPS calls between two device events; one JSON line each with the median and the spread in us, the
algorithmic bytes and the share of the HBM floor at the 8 TB/s peak.

    python tools/stem7_probe.py [--dtypes bf16,fp16] [--cases 0,1] [--batch N] [--out FILE.jsonl]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "ssds.pytorch_amd")]

PEAK_HBM = 8.0e12  # MI355X HBM3E peak, bytes / s

# name, N, Cin, H, W, Cout
CASES = [
    ("fpn_resnet50 640^2 batch 32", 32, 3, 640, 640, 64),
    ("ssd resnet 512^2 batch 64", 64, 3, 512, 512, 64),
]
WARMUP, REPS, ROUNDS = 5, 20, 3


def _timed(fns):
    """fns: {key: callable} -> {key: sorted us per call}; the callables alternate inside every round."""
    import torch

    for fn in fns.values():
        for _ in range(WARMUP):
            fn()
    torch.cuda.synchronize()
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
    return {key: sorted(t) for key, t in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtypes", default="bf16,fp16")
    ap.add_argument("--out", default=None)
    ap.add_argument("--cases", default=None, help="comma-separated indices into CASES (default: all)")
    ap.add_argument("--batch", type=int, default=0, help="a batch size instead of the cases'")
    args = ap.parse_args()
    import torch
    import torch.nn as nn
    from ssds.modeling.layers import stemconv as S

    assert torch.cuda.is_available(), "stem7_probe needs a HIP device"
    out = open(args.out, "w") if args.out else None
    picked = range(len(CASES)) if args.cases is None else [int(v) for v in args.cases.split(",")]
    for ci in picked:
        name, n, cin, h, w, cout = CASES[ci]
        n = args.batch or n
        for dname in args.dtypes.split(","):
            dtype = torch.bfloat16 if dname == "bf16" else torch.float16
            torch.manual_seed(0)
            conv = nn.Conv2d(cin, cout, 7, 2, 3, bias=False).cuda()
            wt = conv.weight
            x = torch.randn(n, cin, h, w, device="cuda").to(dtype)
            ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
            gy = torch.randn(n, cout, ho, wo, device="cuda").to(dtype)

            def lib_forward():
                with torch.autocast("cuda", dtype=dtype):
                    return conv(x)

            y_lib, y_ssdk = lib_forward(), S.stem_conv7x7s2(x, wt)
            torch.cuda.synchronize()
            diff = float((y_lib.float() - y_ssdk.float()).abs().max()) / max(float(y_lib.float().abs().max()), 1e-12)

            def no_grad(fn):
                def run():
                    with torch.no_grad():
                        return fn()
                return run

            fns = {
                ("forward", "ssdk"): no_grad(lambda: S.stem_conv7x7s2(x, wt)),
                ("forward", "library"): no_grad(lib_forward),
                ("wgrad", "ssdk"): lambda: torch.autograd.grad(y_ssdk, (wt,), gy, retain_graph=True),
                ("wgrad", "library"): lambda: torch.autograd.grad(y_lib, (wt,), gy, retain_graph=True),
            }
            e_in, e_out = x.numel(), gy.numel()
            byt = 2 * (e_in + e_out)  # either pass streams the image and the 64-channel map once
            times = _timed(fns)
            for (what, side), t in times.items():
                med = t[len(t) // 2]
                other = times[(what, "library" if side == "ssdk" else "ssdk")]
                row = {"case": name, "N": n, "Cin": cin, "H": h, "W": w, "Cout": cout, "dtype": dname, "pass": what, "side": side,
                       "us_median": round(med, 2), "us_min": round(t[0], 2), "us_max": round(t[-1], 2),
                       "ratio_to_other_side": round(med / other[len(other) // 2], 3), "algorithmic_bytes": byt,
                       "hbm_floor_us": round(byt / PEAK_HBM * 1e6, 2), "share_of_hbm_floor": round(byt / (med * 1e-6) / PEAK_HBM, 4),
                       "forward_max_abs_diff_over_max": round(diff, 6)}
                line = json.dumps(row)
                print(line, flush=True)
                if out:
                    out.write(line + "\n")
                    out.flush()
            del fns, times, y_lib, y_ssdk, x, gy
            torch.cuda.empty_cache()
    if out:
        out.close()


if __name__ == "__main__":
    main()
