"""``ssdk_dense_layer`` (csrc/ssdk_denselayer.hip: a DenseNet dense layer as one launch that reads channels [0, Cin) of its block's
buffer and writes the next 32, the middle map in LDS) against the torch expression -- the module's ``_DenseLayer`` in eval mode on
PyTorch-ROCm, fed the already concatenated channels_last tensor of the same dtype (so the concatenation itself is NOT in the torch
column: it is the layer alone).  The shapes are the first and the last layer of each dense block of
experiments/cfgs/fpn_densenet121_640.yml at batch 32.  Per shape every contender runs WARMUP times, then REPS times between two device
events, ROUNDS rounds; one JSON line per shape with the median and the spread in us of each, the algorithmic FLOPs and bytes of the
layer (Cin channels in, 32 out, the weights once) and the FLOP/s and bytes/s the launch achieves.

    python tools/densenet_probe.py [--dtype bf16] [--batch 32] [--cases 0,1] [--repeat K] [--out FILE.jsonl]

``--e2e CFG`` instead times the forward of a whole detector of a config by device events: the recorded plan (SSDK_DENSELAYER=1), the
plan with the backbone on PyTorch-ROCm (SSDK_DENSELAYER=0) and the module path (SSDK_FUSED_CONV=0).
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "ssds.pytorch_amd")]

PEAK_FLOPS = 2.5e15  # MI355X dense bf16 / fp16 matrix peak
PEAK_BYTES = 8.0e12  # HBM3E

# Cin, Ctot of the block (the buffer's pixel stride), H = W: first and last layer of blocks 1 .. 4 at 640 x 640
CASES = [(64, 256, 160), (224, 256, 160), (128, 512, 80), (480, 512, 80), (256, 1024, 40), (992, 1024, 40), (512, 1024, 20),
         (992, 1024, 20)]
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


def probe_layers(args, dtype, out):
    import torch
    from ssds.modeling.layers import fused_conv as FC
    from ssds.modeling.nets.densenet import _DenseLayer

    for ci in (range(len(CASES)) if args.cases is None else [int(v) for v in args.cases.split(",")]):
        cin, ld, h = CASES[ci]
        w, n = h, args.batch
        torch.manual_seed(ci)
        layer = _DenseLayer(cin, 32, 4, 0).cuda().eval()
        with torch.no_grad():
            for m in layer.modules():
                if isinstance(m, torch.nn.BatchNorm2d):
                    m.running_var.uniform_(0.5, 1.0)
                    m.weight.uniform_(0.5, 1.5)
                    m.bias.normal_(0, 0.1)
        pk = FC.DenseLayerPack(layer, dtype)
        layer = layer.to(dtype).to(memory_format=torch.channels_last)
        buf = torch.zeros((n, h, w, ld), device="cuda", dtype=dtype)
        buf[..., :cin] = (torch.randn(n, h, w, cin, device="cuda") * 0.7).to(dtype)
        x = buf[..., :cin].permute(0, 3, 1, 2).contiguous(memory_format=torch.channels_last)  # the concatenated tensor, dense
        with torch.no_grad():
            ref = layer(x).float()
            FC.dense_layer_native(buf, pk)
            got = buf[..., cin:cin + 32].permute(0, 3, 1, 2).float()
            err = float((got - ref).abs().max()) / max(float(ref.abs().max()), 1e-6)
            times = _timed({"fused": lambda: FC.dense_layer_native(buf, pk), "torch": lambda: layer(x)})
        flops = 2.0 * n * h * w * (cin * 128 + 9 * 128 * 32)
        byt = 2 * (n * h * w * (cin + 32) + cin * 128 + 9 * 128 * 32) + 4 * (2 * cin + 256)
        row = {"Cin": cin, "ld": ld, "H": h, "W": w, "N": n, "dtype": args.dtype, "repeat": args.repeat, "flops": flops,
               "algorithmic_bytes": byt}
        for key in ("fused", "torch"):
            _spread(row, key, times[key])
        med = row["fused_us_median"]
        row["fused_TFLOPs"] = round(flops / med / 1e6, 1)
        row["fused_GBps"] = round(byt / med / 1e3, 1)
        row["fused_fraction_of_matrix_peak"] = round(flops / (med * 1e-6) / PEAK_FLOPS, 4)
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
    keep = {k: os.environ.get(k) for k in ("SSDK_DENSELAYER", "SSDK_FUSED_CONV")}
    try:
        for key, env in (("plan", {"SSDK_DENSELAYER": "1"}), ("plan_backbone_on_torch", {"SSDK_DENSELAYER": "0"}),
                         ("module_path", {"SSDK_FUSED_CONV": "0"})):
            os.environ.update(env)
            model.invalidate_plans()  # (the plan is recorded under the switch's value)
            runs = FC.STATS["plan_runs"]
            with torch.no_grad():
                t = _timed({key: lambda: model(x)})[key]
            assert (FC.STATS["plan_runs"] > runs) == key.startswith("plan"), key
            if key.startswith("plan"):
                (plan,) = [p for p in model.__dict__["_neck_plans"].values() if isinstance(p, FC.ConvPlan)]
                row[key + "_dense_ops"] = sum(r["name"].startswith("dense ") for r in plan.layer_table())
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
    ap.add_argument("--e2e", default=None, metavar="CFG", help="time the whole detector of this config instead of the layers")
    ap.add_argument("--repeat", type=int, default=0, help="written into every line (the identical command is run several times)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    assert torch.cuda.is_available(), "densenet_probe needs a HIP device"
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float16
    out = open(args.out, "a") if args.out else None
    (probe_e2e if args.e2e else probe_layers)(args, dtype, out)
    if out:
        out.close()


if __name__ == "__main__":
    main()
