"""``ssdk_shuffle_unit`` / ``ssdk_shuffle_down`` (csrc/ssdk_shuffle.hip: a ShuffleNetV2 unit as one launch that reads x once and writes
the interleaved y once) against the torch expression -- the module's ``InvertedResidual`` in eval mode on PyTorch-ROCm, channels_last,
same dtype (chunk, three convolutions with their BatchNorms, cat and the five-dimensional transpose of the channel shuffle).  The shapes
are the first (stride 2) and the last (stride 1) unit of each stage of experiments/cfgs/fpn_shufflenetv2_x1_512.yml, and of stage 4 of
experiments/cfgs/yolov3_shufflenetv2_x2_416.yml (the widest units: Cb = 488, the middle channels in eight chunks), at batch 32.  Per
shape every contender runs WARMUP times, then REPS times between two device events, ROUNDS rounds; one JSON line per shape with the
median and the spread in us of each, the algorithmic FLOPs and bytes of the unit (x in, y out, the weights once) and the FLOP/s and
bytes/s the launch achieves.

    python tools/shufflenet_probe.py [--dtype bf16] [--batch 32] [--cases 0,1] [--repeat K] [--out FILE.jsonl]

``--e2e CFG`` instead times the forward of a whole detector of a config by device events: the recorded plan (SSDK_SHUFFLEUNIT=1), the
detector with SSDK_SHUFFLEUNIT=0 (no plan: the backbone's 116- / 244-channel map is no input for a neck plan) and the module path
(SSDK_FUSED_CONV=0).
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "ssds.pytorch_amd")]

PEAK_FLOPS = 2.5e15  # MI355X dense bf16 / fp16 matrix peak
PEAK_BYTES = 8.0e12  # HBM3E

# (input channels, output channels, stride, input H = W): x1 @512 stages 2, 3, 4 first / last unit; x2 @416 stage 4 first / last unit
CASES = [(24, 116, 2, 128), (116, 116, 1, 64), (116, 232, 2, 64), (232, 232, 1, 32), (232, 464, 2, 32), (464, 464, 1, 16),
         (488, 976, 2, 26), (976, 976, 1, 13)]
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


def probe_units(args, dtype, out):
    import torch
    from ssds.modeling.layers import fused_conv as FC
    from ssds.modeling.nets.shufflenet import InvertedResidual

    for ci in (range(len(CASES)) if args.cases is None else [int(v) for v in args.cases.split(",")]):
        cin, cout, stride, h = CASES[ci]
        w, n, cb = h, args.batch, cout // 2
        torch.manual_seed(ci)
        unit = InvertedResidual(cin, cout, stride).cuda().eval()
        with torch.no_grad():
            for m in unit.modules():
                if isinstance(m, torch.nn.BatchNorm2d):
                    m.running_var.uniform_(0.5, 1.0)
                    m.weight.uniform_(0.5, 1.5)
                    m.bias.normal_(0, 0.1)
        down = stride == 2
        pk = (FC.ShuffleDownPack if down else FC.ShuffleUnitPack)(unit, dtype)
        unit = unit.to(dtype).to(memory_format=torch.channels_last)
        ld = FC.pad8(cin)
        xp = torch.zeros((n, h, w, ld), device="cuda", dtype=dtype)
        xp[..., :cin] = (torch.randn(n, h, w, cin, device="cuda") * 0.7).to(dtype)
        x = xp[..., :cin].permute(0, 3, 1, 2).contiguous(memory_format=torch.channels_last)  # what the module is fed: dense, real channels
        native = FC.shuffle_down_native if down else FC.shuffle_unit_native
        ho = (h - 1) // stride + 1
        y = torch.empty((n, ho, ho, FC.pad8(cout)), device="cuda", dtype=dtype)
        with torch.no_grad():
            ref = unit(x).float()
            native(xp, pk, y=y)
            got = y[..., :cout].permute(0, 3, 1, 2).float()
            err = float((got - ref).abs().max()) / max(float(ref.abs().max()), 1e-6)
            times = _timed({"fused": lambda: native(xp, pk, y=y), "torch": lambda: unit(x)})
        if down:
            macs = n * (h * w * cin * cb + ho * ho * (9 * cb + cb * cb + 9 * cin + cin * cb))
            byt = 2 * (n * (h * w * cin + ho * ho * cout) + 2 * cin * cb + cb * cb + 9 * (cin + cb)) + 4 * (2 * cin + 8 * cb)
        else:
            macs = n * h * w * (2 * cb * cb + 9 * cb)
            byt = 2 * (n * h * w * 2 * cout + 2 * cb * cb + 9 * cb) + 4 * 6 * cb
        row = {"Cin": cin, "Cout": cout, "stride": stride, "H": h, "W": w, "N": n, "dtype": args.dtype, "repeat": args.repeat,
               "flops": 2.0 * macs, "algorithmic_bytes": byt}
        for key in ("fused", "torch"):
            _spread(row, key, times[key])
        med = row["fused_us_median"]
        row["fused_TFLOPs"] = round(2.0 * macs / med / 1e6, 1)
        row["fused_GBps"] = round(byt / med / 1e3, 1)
        row["fused_fraction_of_matrix_peak"] = round(2.0 * macs / (med * 1e-6) / PEAK_FLOPS, 4)
        row["fused_fraction_of_hbm_peak"] = round(byt / (med * 1e-6) / PEAK_BYTES, 4)
        row["fused_over_torch"] = round(med / row["torch_us_median"], 3)
        row["fused_max_abs_diff_over_max"] = round(err, 5)
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
    keep = {k: os.environ.get(k) for k in ("SSDK_SHUFFLEUNIT", "SSDK_FUSED_CONV")}
    try:
        for key, env in (("plan", {"SSDK_SHUFFLEUNIT": "1"}), ("shuffleunit_0", {"SSDK_SHUFFLEUNIT": "0"}),
                         ("module_path", {"SSDK_FUSED_CONV": "0"})):
            for k in keep:
                os.environ.pop(k, None)
            os.environ.update(env)
            model.invalidate_plans()  # (the plan is recorded under the switch's value)
            runs = FC.STATS["plan_runs"]
            with torch.no_grad():
                t = _timed({key: lambda: model(x)})[key]
            assert (FC.STATS["plan_runs"] > runs) == (key == "plan"), key
            if key == "plan":
                (plan,) = [p for p in model.__dict__["_neck_plans"].values() if isinstance(p, FC.ConvPlan)]
                row["plan_shuffle_ops"] = sum(r["name"].startswith("shuffle") for r in plan.layer_table())
            _spread(row, key, t)
            row[key + "_img_per_s"] = round(args.batch / (t[len(t) // 2] * 1e-6), 1)
            row[key + "_img_per_s_slowest"] = round(args.batch / (t[-1] * 1e-6), 1)
            row[key + "_img_per_s_fastest"] = round(args.batch / (t[0] * 1e-6), 1)
    finally:
        for k, v in keep.items():
            os.environ.pop(k, None)
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
    ap.add_argument("--e2e", default=None, metavar="CFG", help="time the whole detector of this config instead of the units")
    ap.add_argument("--repeat", type=int, default=0, help="written into every line (the identical command is run several times)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    assert torch.cuda.is_available(), "shufflenet_probe needs a HIP device"
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float16
    out = open(args.out, "a") if args.out else None
    (probe_e2e if args.e2e else probe_units)(args, dtype, out)
    if out:
        out.close()


if __name__ == "__main__":
    main()
