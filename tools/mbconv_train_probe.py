"""The EfficientNet layers of the training step on csrc/ssdk_mbconvtrain.hip against the eager expressions they replace, per shape
of ``bifpn_efficientnetb0_512`` at batch 32: the nine 5x5 depthwise convolutions (forward, input gradient, weight gradient; against
``F.conv2d`` under autograd in the same dtype) and the sixteen squeeze-excite sites (forward and backward of
``silu_squeeze_excite``; against ``nn.SiLU`` followed by ``x * se(x)`` of nets/efficientnet.py under 16-bit autocast).  After a
warm-up the two sides of a row alternate, ROUNDS rounds of REPS calls between two device events; one JSON line each with the median
in us, the algorithmic bytes (computed here from the shapes) and their share of the 8 TB/s HBM peak.

    python tools/mbconv_train_probe.py [--dtypes bf16,fp16] [--batch 32] [--size 512] [--out FILE.jsonl]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "ssds.pytorch_amd")]

PEAK_HBM = 8.0e12  # MI355X HBM3E peak, bytes / s
WARMUP, REPS, ROUNDS = 3, 10, 3


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


def sites(size):
    """[(block name, hidden width C, Cr, k, stride, input H = W of the depthwise convolution)] of EfficientNet-B0 at size x size"""
    from ssds.modeling import nets

    net = nets.EfficientNetB0(outputs=[7])
    hw = (size - 1) // 2 + 1
    rows = []
    for j in range(7):
        for i, blk in enumerate(getattr(net, "stage%d" % (j + 1))):
            _, dw, se, _, _ = blk.parts()
            conv = dw[0]
            rows.append(("stage%d.%d" % (j + 1, i), conv.in_channels, se.se[1].out_channels, conv.kernel_size[0], conv.stride[0], hw))
            hw = (hw - 1) // conv.stride[0] + 1
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtypes", default="bf16,fp16")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--out", default=None, help="a file name; '{dtype}' in it is replaced per dtype")
    args = ap.parse_args()
    import torch
    import torch.nn as nn
    import torch.nn.functional as F
    from ssds.modeling.layers import mbconvtrain as M
    from ssds.modeling.nets.efficientnet import SqueezeExcitation

    assert torch.cuda.is_available(), "mbconv_train_probe needs a HIP device"
    n = args.batch
    for dname in args.dtypes.split(","):
        dtype = torch.bfloat16 if dname == "bf16" else torch.float16
        out = open(args.out.replace("{dtype}", dname), "w") if args.out else None

        def emit(row):
            line = json.dumps(row)
            print(line, flush=True)
            if out:
                out.write(line + "\n")
                out.flush()

        def rows_of(times, base, bytes_of):
            for (what, side), t in times.items():
                med = t[len(t) // 2]
                other = times[(what, "eager" if side == "ssdk" else "ssdk")]
                byt = bytes_of[what]
                emit(dict(base, **{"pass": what, "side": side, "us_median": round(med, 2), "us_min": round(t[0], 2),
                                   "us_max": round(t[-1], 2), "ratio_to_other_side": round(med / other[len(other) // 2], 3),
                                   "algorithmic_bytes": byt, "share_of_hbm_peak": round(byt / (med * 1e-6) / PEAK_HBM, 4)}))

        for name, c, cr, k, stride, hw in sites(args.size):
            torch.manual_seed(0)
            ho = (hw - 1) // stride + 1
            if k == 5:
                # one graph per gradient: an autograd.Function computes every gradient its inputs asked for at forward time, so the
                # input-gradient row differentiates a forward whose weight was detached, and the other way round
                x = torch.randn(n, c, hw, hw, device="cuda").to(dtype)
                w32 = torch.randn(c, 1, 5, 5, device="cuda") / 5
                w16 = w32.to(dtype)
                xg, w32g, w16g = x.clone().requires_grad_(True), w32.clone().requires_grad_(True), w16.clone().requires_grad_(True)
                gy = torch.randn(n, c, ho, ho, device="cuda").to(dtype)
                ys_x, ys_w = M.dwconv5x5(xg, w32, stride), M.dwconv5x5(x, w32g, stride)
                ye_x, ye_w = F.conv2d(xg, w16, None, stride, 2, 1, c), F.conv2d(x, w16g, None, stride, 2, 1, c)
                fns = {
                    ("forward", "ssdk"): lambda: M.dwconv5x5(x, w32, stride),
                    ("forward", "eager"): lambda: F.conv2d(x, w16, None, stride, 2, 1, c),
                    ("dgrad", "ssdk"): lambda: torch.autograd.grad(ys_x, (xg,), gy, retain_graph=True),
                    ("dgrad", "eager"): lambda: torch.autograd.grad(ye_x, (xg,), gy, retain_graph=True),
                    ("wgrad", "ssdk"): lambda: torch.autograd.grad(ys_w, (w32g,), gy, retain_graph=True),
                    ("wgrad", "eager"): lambda: torch.autograd.grad(ye_w, (w16g,), gy, retain_graph=True),
                }
                byt = 2 * (x.numel() + gy.numel())  # every pass streams the input-sized and the output-sized tensor once
                rows_of(_timed(fns), {"layer": name + " dw5x5", "N": n, "C": c, "H": hw, "W": hw, "stride": stride, "dtype": dname},
                        {"forward": byt, "dgrad": byt, "wgrad": byt})
                del fns, ys_x, ys_w, ye_x, ye_w, x, xg, gy
            # the squeeze-excite site behind the depthwise BatchNorm
            u = torch.randn(n, c, ho, ho, device="cuda").to(dtype).requires_grad_(True)
            gz = torch.randn(n, c, ho, ho, device="cuda").to(dtype)
            se = SqueezeExcitation(c, cr).cuda()
            act = nn.SiLU()
            params = [se.se[1].weight, se.se[1].bias, se.se[3].weight, se.se[3].bias]

            def eager_forward():
                with torch.autocast("cuda", dtype=dtype):
                    return se(act(u))

            def ssdk_forward():
                return M.silu_squeeze_excite(u, *params)

            z_s, z_e = ssdk_forward(), eager_forward()

            def no_grad(fn):
                def run():
                    with torch.no_grad():
                        return fn()
                return run

            fns = {
                ("forward", "ssdk"): no_grad(ssdk_forward),
                ("forward", "eager"): no_grad(eager_forward),
                ("backward", "ssdk"): lambda: torch.autograd.grad(z_s, [u] + params, gz, retain_graph=True),
                ("backward", "eager"): lambda: torch.autograd.grad(z_e, [u] + params, gz, retain_graph=True),
            }
            e = u.numel()
            # forward: u read by the pool and by the scale, z written; backward: u and dz read by the reduction and by the apply, du written
            rows_of(_timed(fns), {"layer": name + " silu+se", "N": n, "C": c, "Cr": cr, "H": ho, "W": ho, "dtype": dname},
                    {"forward": 2 * 3 * e, "backward": 2 * 5 * e})
            del fns, z_s, z_e, u, gz
            torch.cuda.empty_cache()
        if out:
            out.close()


if __name__ == "__main__":
    main()
