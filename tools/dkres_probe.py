"""``ssdk_dkres`` (csrc/ssdk_dkres.hip: a DarkNet residual block as one launch, the intermediate map in LDS) against the two
``ssdk_conv`` launches it replaces (1x1, then 3x3 with the block input added behind the activation) and against the torch expression
-- the ``Residual`` module in eval mode on channels_last tensors of the same dtype on PyTorch-ROCm.  The shapes are the five block
shapes of experiments/cfgs/yolov3_darknet53_416.yml and yolov4_darknet53_512.yml at batch 32.  Per shape every contender runs WARMUP
times, then REPS times between two device events, ROUNDS rounds; one JSON line per shape with the median and the spread in us of
each, the algorithmic FLOPs and bytes of the block (x in, y out, the weights once) and the FLOP/s and bytes/s the fused launch and
the two launches achieve.  A width ``ssdk_dkres_supported`` does not take has no fused column (``"fused_us_median": null``).

    python tools/dkres_probe.py [--dtype bf16] [--batch 32] [--cases 0,1] [--out FILE.jsonl]

``--e2e CFG`` instead times the whole detector of a config by device events: the recorded plan under SSDK_DKRES=1 and =0 and the
module path on PyTorch-ROCm (SSDK_FUSED_CONV=0), which bench.py refuses to time for the YOLO heads.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "ssds.pytorch_amd")]

PEAK_FLOPS = 2.5e15  # MI355X dense bf16 / fp16 matrix peak
PEAK_BYTES = 8.0e12  # HBM3E

# C, H = W: block1 .. block5 at 416 x 416 and at 512 x 512
CASES = [(64, 208), (128, 104), (256, 52), (512, 26), (1024, 13), (64, 256), (128, 128), (256, 64), (512, 32), (1024, 16)]
WARMUP, REPS, ROUNDS = 3, 10, 3


def _timed(fns):
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


def _spread(row, key, t):
    row[key + "_us_median"], row[key + "_us_min"], row[key + "_us_max"] = round(t[len(t) // 2], 2), round(t[0], 2), round(t[-1], 2)


def probe_blocks(args, dtype, out):
    import torch
    from ssds import _native as N
    from ssds.modeling.layers import fused_conv as FC
    from ssds.modeling.nets.darknet import Residual

    for ci in (range(len(CASES)) if args.cases is None else [int(v) for v in args.cases.split(",")]):
        c, h = CASES[ci]
        w, n = h, args.batch
        torch.manual_seed(ci)
        blk = Residual(c).cuda().eval()
        with torch.no_grad():
            for m in blk.modules():
                if isinstance(m, torch.nn.BatchNorm2d):
                    m.running_var.uniform_(0.5, 1.0)
                    m.weight.uniform_(0.5, 1.5)
        p1 = FC.ConvPack(blk.conv1x1[0], blk.conv1x1[1], "relu6", dtype)
        p2 = FC.ConvPack(blk.conv3x3[0], blk.conv3x3[1], "relu6", dtype)
        blk = blk.to(dtype).to(memory_format=torch.channels_last)
        x = (torch.randn(n, c, h, w, device="cuda") * 0.7).to(dtype).contiguous(memory_format=torch.channels_last)
        mid = torch.empty((n, c // 2, h, w), device="cuda", dtype=dtype).contiguous(memory_format=torch.channels_last)
        y = torch.empty_like(x)
        y2 = torch.empty_like(x)
        fused_ok = bool(N.lib.ssdk_dkres_supported(c, h, w, N.dtype_code(x)))

        def two():
            FC.conv_native(x, p1, y=mid)
            return FC.conv_native(mid, p2, residual=x, res_mode=0, y=y2)

        with torch.no_grad():
            fns = {"two": two, "torch": lambda: blk(x)}
            if fused_ok:
                fns["fused"] = lambda: FC.dkres_native(x, p1, p2, y=y)
            ref = two().float()
            scale = max(float(ref.abs().max()), 1e-6)
            err_t = float((blk(x).float() - ref).abs().max()) / scale
            err_f = float((FC.dkres_native(x, p1, p2, y=y).float() - ref).abs().max()) / scale if fused_ok else None
            times = _timed(fns)
        flops = 2.0 * n * h * w * (c * c // 2 + 9 * c * c // 2)
        byt = 2 * (2 * n * h * w * c + c * c // 2 + 9 * c * c // 2) + 4 * 3 * c
        row = {"C": c, "H": h, "W": w, "N": n, "dtype": args.dtype, "flops": flops, "algorithmic_bytes": byt}
        for key in ("fused", "two", "torch"):
            if key in times:
                _spread(row, key, times[key])
            else:
                row[key + "_us_median"] = None
        t2 = row["two_us_median"]
        for key in ("fused", "two"):
            med = row[key + "_us_median"]
            if med is not None:
                row[key + "_TFLOPs"] = round(flops / med / 1e6, 1)
                row[key + "_GBps"] = round(byt / med / 1e3, 1)
                row[key + "_fraction_of_matrix_peak"] = round(flops / (med * 1e-6) / PEAK_FLOPS, 4)
                row[key + "_fraction_of_hbm_peak"] = round(byt / (med * 1e-6) / PEAK_BYTES, 4)
        row["fused_over_two"] = round(row["fused_us_median"] / t2, 3) if fused_ok else None
        row["torch_over_two"] = round(row["torch_us_median"] / t2, 3)
        row["fused_max_abs_diff_over_max"] = None if err_f is None else round(err_f, 5)
        row["torch_max_abs_diff_over_max"] = round(err_t, 5)
        line = json.dumps(row)
        print(line, flush=True)
        if out:
            out.write(line + "\n")


def probe_e2e(args, dtype, out):
    import torch
    from ssds.core import config
    from ssds.modeling import model_builder
    from ssds.modeling.layers import fused_conv as FC

    cfg = config.cfg_from_file(args.e2e)
    torch.manual_seed(0)
    model = model_builder.create_model(cfg.MODEL).eval().cuda().to(dtype)
    hh, ww = cfg.MODEL.IMAGE_SIZE
    x = torch.rand(args.batch, 3, hh, ww, device="cuda").to(dtype)
    row = {"cfg": os.path.basename(args.e2e), "N": args.batch, "dtype": args.dtype}
    keep = {k: os.environ.get(k) for k in ("SSDK_DKRES", "SSDK_FUSED_CONV")}
    try:
        for key, env in (("plan_dkres1", {"SSDK_DKRES": "1"}), ("plan_dkres0", {"SSDK_DKRES": "0"}),
                         ("module_path", {"SSDK_FUSED_CONV": "0"})):
            os.environ.update(env)
            model.invalidate_plans()  # (the plan is recorded under the switch's value)
            runs = FC.STATS["plan_runs"]
            with torch.no_grad():
                t = _timed({key: lambda: model(x)})[key]
            assert (FC.STATS["plan_runs"] > runs) == key.startswith("plan"), key
            if key.startswith("plan"):
                (plan,) = [p for p in model.__dict__["_neck_plans"].values() if isinstance(p, FC.ConvPlan)]
                row[key + "_dkres_ops"] = sum(r["name"].startswith("dkres ") for r in plan.layer_table())
            _spread(row, key, t)
            row[key + "_img_per_s"] = round(args.batch / (t[len(t) // 2] * 1e-6), 1)
            for k in env:
                os.environ.pop(k)
    finally:
        for k, v in keep.items():
            if v is not None:
                os.environ[k] = v
    line = json.dumps(row)
    print(line, flush=True)
    if out:
        out.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp16"])
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--cases", default=None, help="comma-separated indices into CASES (default: all)")
    ap.add_argument("--e2e", default=None, metavar="CFG", help="time the whole detector of this config instead of the blocks")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    assert torch.cuda.is_available(), "dkres_probe needs a HIP device"
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float16
    out = open(args.out, "a") if args.out else None
    (probe_e2e if args.e2e else probe_blocks)(args, dtype, out)
    if out:
        out.close()


if __name__ == "__main__":
    main()
