"""Forward + backward of ONE dense layer, the kernels of csrc/ssdk_densetrain.hip (ssds/modeling/layers/densetrain.py layer_forward /
layer_backward on a block's buffer) against ``_DenseLayer`` on PyTorch-ROCm with the Solver's other swaps (FastBatchNorm2d,
PointwiseConv2d with the statistics hand-off, DenseConv3x3) under bf16 autocast: the first and the last layer of each of the four
blocks of fpn_densenet121_640 at batch 32.

    native   finalize of norm1 from the block's sums, 1x1 with norm1 + relu1 on load, norm2 + relu2, 3x3, place;
             3x3 gradients, norm2 backward, 1x1 weight gradient (op on load), W1^T dm, bn1_reduce, bn1_apply into G[:, :K]
    module   torch.cat of the j + 1 feature tensors, BatchNorm over K channels (statistics, apply, stored output), ReLU, 1x1,
             BatchNorm + ReLU, 3x3; autograd's backward with the gradient of the concatenation split into j + 1 slices
Per (case, side): CALLS calls between two device events after a warm-up, the two sides alternating, ROUNDS rounds; one JSON line
each with the median and the spread (min, max) in us per call, and the peak allocation of one call above what was allocated before
it.  Both sides include their launch gaps, as they do in the step.

    python tools/densetrain_probe.py [--dtype bf16] [--batch 32] [--out FILE.jsonl]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "ssds.pytorch_amd")]

# (block, layer, side of the map, C0 of the block, j = layers before this one): fpn_densenet121_640, blocks of 6 / 12 / 24 / 16 layers
CASES = [(1, "first", 160, 64, 0), (1, "last", 160, 64, 5), (2, "first", 80, 128, 0), (2, "last", 80, 128, 11),
         (3, "first", 40, 256, 0), (3, "last", 40, 256, 23), (4, "first", 20, 512, 0), (4, "last", 20, 512, 15)]
CALLS, WARMUP, ROUNDS = 10, 3, 5


def _time(fns):
    """{key: callable} -> {key: sorted us per call}: the callables alternate, ROUNDS rounds of CALLS calls between two events."""
    import torch

    for fn in fns.values():
        for _ in range(WARMUP):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(ROUNDS):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(CALLS):
                fn()
            b.record()
            b.synchronize()
            out[k].append(a.elapsed_time(b) * 1e3 / CALLS)
    return {k: sorted(v) for k, v in out.items()}


def _peak(fn):
    """MiB one call allocates at its peak above what is allocated when it starts."""
    import torch

    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="bf16", choices=("bf16", "fp16"))
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    from ssds import _native as N
    from ssds.modeling.layers import densetrain as DT
    from ssds.modeling.layers.batchnorm import fuse_bn_activations, use_fast_batchnorm
    from ssds.modeling.layers.denseconv import use_native_dense3x3
    from ssds.modeling.layers.pointwise import fuse_conv_bn_statistics, use_pointwise_gemm
    from ssds.modeling.nets.densenet import _DenseLayer

    if not torch.cuda.is_available():
        raise SystemExit("densetrain_probe: needs a HIP device (there is no CPU path to time)")
    dt = torch.bfloat16 if args.dtype == "bf16" else torch.float16
    dev = torch.device("cuda")
    n = args.batch
    lines = []
    for block, which, side, c0, j in CASES:
        k, hw = c0 + 32 * j, side * side
        g = torch.Generator(device="cuda").manual_seed(100 * block + j)
        layer = _DenseLayer(k, 32, 4, 0).to(dev).train()
        use_fast_batchnorm(layer)
        fuse_bn_activations(layer)
        use_pointwise_gemm(layer)
        fuse_conv_bn_statistics(layer)
        use_native_dense3x3(layer)
        params = [layer.norm1.weight, layer.norm1.bias, layer.conv1.weight, layer.norm2.weight, layer.norm2.bias, layer.conv2.weight]
        F = torch.randn(n, k + 32, side, side, device=dev, generator=g).to(dt)
        G = torch.randn(n, k + 32, side, side, device=dev, generator=g).to(dt)
        bsums = torch.empty(k + 32, 2, device=dev)
        DT.place(F[:, :k].contiguous(), F.data_ptr(), (k + 32) * hw, bsums.data_ptr(), n, k, hw, N.dtype_code(F), dev)
        scratch = torch.empty(n, k, hw, device=dev, dtype=dt)
        feats = [F[:, :c0].contiguous().requires_grad_(True)] + [F[:, c0 + 32 * i:c0 + 32 * i + 32].contiguous().requires_grad_(True)
                                                                for i in range(j)]
        gy = G[:, k:].contiguous()

        def native():
            saved = DT.layer_forward(F, bsums, k, layer, params, momenta=(0.1, 0.1))
            DT.layer_backward(F, G, scratch, k, saved, params, (True,) * 6, True)

        def module():
            with torch.autocast("cuda", dtype=dt):
                y = layer(feats)
            torch.autograd.grad(y, feats + params, gy)

        t = _time({"native": native, "module": module})
        peaks = {"native": _peak(native), "module": _peak(module)}
        for path, us in t.items():
            rec = dict(cfg="fpn_densenet121_640", block=block, layer=which, side=side, cin=k, batch=n, dtype=args.dtype,
                       call="layer fwd+bwd", path=path, us_median=round(us[len(us) // 2], 2), us_min=round(us[0], 2),
                       us_max=round(us[-1], 2), peak_MiB=peaks[path], calls=CALLS, rounds=ROUNDS)
            lines.append(rec)
            print(json.dumps(rec), flush=True)
        del F, G, feats, scratch, gy
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
