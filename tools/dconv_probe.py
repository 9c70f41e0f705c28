"""The dilated 3x3 convolution of the RFB extras (csrc/ssdk_dconv.hip behind a 'dilated' ConvPack) against the torch expression --
``F.conv2d(x, w, padding=d, dilation=d)`` on channels_last tensors of the same dtype on PyTorch-ROCm (the convolution alone: the folded
BatchNorm the kernel also applies is not charged to torch).  The shapes are the dilated layers of experiments/cfgs/
ssd_resnet18_rfb_512.yml (128 -> 128 at 8 x 8 and 4 x 4, dilations 3 and 5) and shelf_resnet18_rfb_513.yml (128 -> 128 at 9 x 9,
64 -> 64 at 5 x 5) at batch 32, plus two larger maps (32 -> 32 at 64 x 64, 64 -> 64 at 32 x 32).  Per shape both contenders run WARMUP
times, then REPS times between two device events, ROUNDS rounds; one JSON line per shape with the median and the spread in us of
each, the layer's FLOPs (all nine taps, whether inside the map or not) and algorithmic bytes.

    python tools/dconv_probe.py [--dtype bf16] [--batch 32] [--cases 0,1] [--repeat K] [--out FILE.jsonl]

``--repeat K`` only labels the lines (field ``repeat``) of the K-th run of the identical command.

``--e2e CFG`` instead times the whole detector of a config by device events: the recorded plan (SSDK_DCONV=1) and the module path on
PyTorch-ROCm (SSDK_FUSED_CONV=0), forward alone; with SSDK_DCONV=0 the detector has no plan and runs its module path with fused heads.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "ssds.pytorch_amd")]

PEAK_FLOPS = 2.5e15  # MI355X dense bf16 / fp16 matrix peak
PEAK_BYTES = 8.0e12  # HBM3E

# Cin, Cout, H, W, dilation
CASES = [(128, 128, 8, 8, 3), (128, 128, 8, 8, 5), (128, 128, 4, 4, 3), (128, 128, 4, 4, 5),
         (128, 128, 9, 9, 3), (128, 128, 9, 9, 5), (64, 64, 5, 5, 3), (64, 64, 5, 5, 5),
         (32, 32, 64, 64, 3), (32, 32, 64, 64, 5), (64, 64, 32, 32, 3), (64, 64, 32, 32, 5)]
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


def _taps_inside(h, w, d):
    """mean number of the nine taps that fall inside an h x w map"""
    rows = sum(1 + (y - d >= 0) + (y + d < h) for y in range(h))
    cols = sum(1 + (x - d >= 0) + (x + d < w) for x in range(w))
    return rows * cols / float(h * w)


def probe_layers(args, dtype, out):
    import torch
    import torch.nn.functional as F
    from ssds import _native as N
    from ssds.modeling.layers import fused_conv as FC

    for ci in (range(len(CASES)) if args.cases is None else [int(v) for v in args.cases.split(",")]):
        cin, cout, h, w, d = CASES[ci]
        n = args.batch
        torch.manual_seed(ci)
        conv = torch.nn.Conv2d(cin, cout, 3, 1, d, dilation=d, bias=False).cuda()
        bn = torch.nn.BatchNorm2d(cout).cuda().eval()
        with torch.no_grad():
            bn.running_var.uniform_(0.5, 1.0)
            bn.weight.uniform_(0.5, 1.5)
        pk = FC.ConvPack(conv, bn, "none", dtype)
        assert pk.kind == "dilated" and N.lib.ssdk_dconv3x3_supported(cin, cout, h, w, d, N._DTYPES[dtype])
        wt = conv.weight.detach().to(dtype).contiguous(memory_format=torch.channels_last)
        x = (torch.randn(n, cin, h, w, device="cuda") * 0.7).to(dtype).contiguous(memory_format=torch.channels_last)
        y = torch.empty((n, cout, h, w), device="cuda", dtype=dtype).contiguous(memory_format=torch.channels_last)
        with torch.no_grad():
            fns = {"kernel": lambda: FC.conv_native(x, pk, y=y), "torch": lambda: F.conv2d(x, wt, None, 1, d, d)}
            ref = F.conv2d(x.float(), conv.weight.detach().to(dtype).float(), None, 1, d, d)
            ref = ref * pk.scale.view(1, -1, 1, 1) + pk.bias.view(1, -1, 1, 1)
            err = float((FC.conv_native(x, pk, y=y).float() - ref).abs().max()) / max(float(ref.abs().max()), 1e-6)
            assert N.last_kernel() == "dconv3x3_kernel"
            times = _timed(fns)
        flops = 2.0 * n * h * w * cout * 9 * cin
        byt = 2 * (n * h * w * (cin + cout) + 9 * cin * cout) + 4 * 2 * cout
        row = {"Cin": cin, "Cout": cout, "H": h, "W": w, "dilation": d, "N": n, "dtype": args.dtype, "repeat": args.repeat, "flops": flops,
               "algorithmic_bytes": byt, "mean_taps_inside": round(_taps_inside(h, w, d), 2)}
        for key in ("kernel", "torch"):
            _spread(row, key, times[key])
        med = row["kernel_us_median"]
        row["kernel_TFLOPs"] = round(flops / med / 1e6, 2)
        row["kernel_GBps"] = round(byt / med / 1e3, 1)
        row["kernel_fraction_of_matrix_peak"] = round(flops / (med * 1e-6) / PEAK_FLOPS, 5)
        row["kernel_fraction_of_hbm_peak"] = round(byt / (med * 1e-6) / PEAK_BYTES, 5)
        row["kernel_over_torch"] = round(med / row["torch_us_median"], 3)
        row["kernel_max_abs_diff_over_max"] = round(err, 5)
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
    row = {"cfg": os.path.basename(args.e2e), "N": args.batch, "dtype": args.dtype, "repeat": args.repeat}
    keep = {k: os.environ.get(k) for k in ("SSDK_DCONV", "SSDK_FUSED_CONV")}
    try:
        for key, env in (("plan", {"SSDK_DCONV": "1"}), ("module_path", {"SSDK_FUSED_CONV": "0"}), ("dconv0", {"SSDK_DCONV": "0"})):
            os.environ.update(env)
            model.invalidate_plans()  # (the plan is recorded under the switch's value)
            runs = FC.STATS["plan_runs"]
            with torch.no_grad():
                t = _timed({key: lambda: model(x)})[key]
            if key == "plan":
                plans = model.__dict__.get("_plans") or model.__dict__.get("_neck_plans")
                (plan,) = [p for p in plans.values() if isinstance(p, FC.ConvPlan)]
                row["plan_dilated_ops"] = sum(1 for L in plan.layers if L.get("kind") is None and L["pack"].kind == "dilated")
                assert FC.STATS["plan_runs"] > runs and row["plan_dilated_ops"] > 0
            elif key == "module_path":
                assert FC.STATS["plan_runs"] == runs
            else:
                row["dconv0_plan_runs"] = FC.STATS["plan_runs"] - runs  # (a neck plan on backbone maps would still count)
            _spread(row, key, t)
            row[key + "_img_per_s"] = round(args.batch / (t[len(t) // 2] * 1e-6), 1)
            row[key + "_img_per_s_min"] = round(args.batch / (t[-1] * 1e-6), 1)
            row[key + "_img_per_s_max"] = round(args.batch / (t[0] * 1e-6), 1)
            for k in env:
                os.environ.pop(k)
    finally:
        for k, v in keep.items():
            if v is not None:
                os.environ[k] = v
    row["plan_slowest_beats_module_fastest"] = row["plan_us_max"] < row["module_path_us_min"]
    line = json.dumps(row)
    print(line, flush=True)
    if out:
        out.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp16"])
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--cases", default=None, help="comma-separated indices into CASES (default: all)")
    ap.add_argument("--e2e", default=None, metavar="CFG", help="time the whole detector of this config instead of the layers")
    ap.add_argument("--repeat", type=int, default=1, help="label of this run among identical ones")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    assert torch.cuda.is_available(), "dconv_probe needs a HIP device"
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float16
    out = open(args.out, "a") if args.out else None
    (probe_e2e if args.e2e else probe_layers)(args, dtype, out)
    if out:
        out.close()


if __name__ == "__main__":
    main()
