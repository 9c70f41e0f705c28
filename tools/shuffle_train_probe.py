"""The ShuffleNetV2 training kernels (csrc/ssdk_shuffletrain.hip) against what runs for the same layer without them, per (unit, call):
the first and the last unit of each stage of fpn_shufflenetv2_x1_512 and yolov3_shufflenetv2_x2_416 at batch 32.

    slice forward      ssdk_pws_forward on x[:, Cb:] where it lies     |  F.conv2d on the ``chunk`` view (bf16 weight)
    slice dgrad        ssdk_pws_forward into the right half of a buffer |  torch.matmul(W^T, gy) of layers/pointwise._Pointwise
    odd 1x1 fwd + bwd  layers/pointwise marked layer (ssdk_pws_*)       |  the ``_Pointwise`` path (library GEMMs)
    weight gradient    ssdk_pws_wgrad                                   |  bmm(gy, x^T, out_dtype=float32).sum(0)
    join forward       ssdk_shuffle_join_fwd                            |  cat + channel_shuffle
    join backward      ssdk_shuffle_join_bwd                            |  their autograd backward
Per (case, call, side): CALLS calls between two device events after a warm-up, the two sides alternating, ROUNDS rounds; one JSON
line each with the median and the spread (min, max) in us per call.  The eager side includes its launch gaps, as it does in the step.

    python tools/shuffle_train_probe.py [--dtype bf16] [--batch 32] [--out FILE.jsonl]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "ssds.pytorch_amd")]

# (config, stage, unit, stride, input channels, output channels, side of the unit's OUTPUT map)
CASES = []
for _cfg, _size, _widths in (("fpn_shufflenetv2_x1_512", 512, (24, 116, 232, 464)), ("yolov3_shufflenetv2_x2_416", 416, (24, 244, 488, 976))):
    for _s in range(3):
        _side = _size // (8 << _s)
        CASES.append((_cfg, _s + 2, "first", 2, _widths[_s], _widths[_s + 1], _side))
        CASES.append((_cfg, _s + 2, "last", 1, _widths[_s + 1], _widths[_s + 1], _side))
CALLS, WARMUP, ROUNDS = 20, 5, 5


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="bf16", choices=("bf16", "fp16"))
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    import torch.nn.functional as F
    from ssds import _native as N
    from ssds.modeling.layers import pointwise as PW
    from ssds.modeling.layers import shuffletrain as ST
    from ssds.modeling.nets.shufflenet import channel_shuffle

    if not torch.cuda.is_available():
        raise SystemExit("shuffle_train_probe: needs a HIP device (there is no CPU path to time)")
    dt = torch.bfloat16 if args.dtype == "bf16" else torch.float16
    dev = torch.device("cuda")
    lines = []
    b = args.batch
    for cfg, stage, unit, stride, cin, cout, side in CASES:
        cb, hw = cout // 2, side * side
        g = torch.Generator(device="cuda").manual_seed(stage * 10 + stride)
        rnd = lambda *s: torch.randn(*s, device=dev, generator=g).to(dt)  # noqa: E731
        code = N.BF16 if dt == torch.bfloat16 else N.F16
        calls = {}
        if stride == 1:
            x, w32, gy = rnd(b, 2 * cb, side, side), torch.randn(cb, cb, 1, 1, device=dev, generator=g) / cb ** 0.5, rnd(b, cb, side, side)
            w16, wt16 = ST.prepare_weights(w32, dt)
            wd = w32.to(dt)
            y = torch.empty(b, cb, side, side, device=dev, dtype=dt)
            gx = torch.empty_like(x)
            off, xs = ST.slice_geometry(x.shape, cb)
            x2 = x.chunk(2, 1)[1]
            x2c = x2.contiguous()
            calls["slice forward"] = (lambda: ST.pws_forward(x.data_ptr() + 2 * off, xs, w16, None, y.data_ptr(), cb * hw, b, cb, cb, hw, code, dev),
                                      lambda: F.conv2d(x2, wd))
            calls["slice dgrad"] = (lambda: ST.pws_forward(gy.data_ptr(), cb * hw, wt16, None, gx.data_ptr() + 2 * off, xs, b, cb, cb, hw, code, dev),
                                    lambda: torch.matmul(wd.view(cb, cb).t(), gy.view(b, cb, hw)))
            calls["slice wgrad"] = (lambda: ST.pws_wgrad(gy, x.data_ptr() + 2 * off, xs, b, cb, cb, hw, code, dev),
                                    lambda: torch.bmm(gy.view(b, cb, hw), x2c.view(b, cb, hw).transpose(1, 2), out_dtype=torch.float32).sum(0))
            left, lhalf = x, True
            k_in = cb
        else:
            x, w32 = rnd(b, cin, 2 * side, 2 * side), torch.randn(cb, cin, 1, 1, device=dev, generator=g) / cin ** 0.5
            left, lhalf = rnd(b, cb, side, side), False
            k_in = cin
        # the unit's contiguous 1x1 of width k_in -> Cb (stride 1: the LAST 1x1 of branch2; stride 2: the first), forward + backward
        xi = (x2c if stride == 1 else x).detach().requires_grad_(True)
        wp = w32.detach().requires_grad_(True)
        gyo = rnd(b, cb, *xi.shape[2:])

        def layer(native):
            if native:
                yy = PW._PointwiseNative.apply(xi, wp, None, False, True)
            else:
                yy = PW._Pointwise.apply(xi, wp.to(dt), None)
            torch.autograd.grad(yy, (xi, wp), gyo)

        if k_in % 8 or cb % 8:
            calls["odd 1x1 fwd+bwd %d->%d" % (k_in, cb)] = (lambda: layer(True), lambda: layer(False))
        right, gout = rnd(b, cb, side, side), rnd(b, 2 * cb, side, side)
        yj = torch.empty(b, 2 * cb, side, side, device=dev, dtype=dt)
        gl = torch.empty_like(left)
        gr = torch.empty_like(right)
        ls = (2 if lhalf else 1) * cb * hw
        sp = lambda: N.stream_ptr(dev)  # noqa: E731
        la = (left.chunk(2, 1)[0] if lhalf else left).detach().requires_grad_(True)
        ra = right.detach().requires_grad_(True)
        eager_out = channel_shuffle(torch.cat((la, ra), 1), 2)
        calls["join forward"] = (lambda: N.check(N.lib.ssdk_shuffle_join_fwd(left.data_ptr(), ls, right.data_ptr(), yj.data_ptr(), b, cb, hw, code, sp()), "join"),
                                 lambda: channel_shuffle(torch.cat((la.detach(), ra.detach()), 1), 2))
        calls["join backward"] = (lambda: N.check(N.lib.ssdk_shuffle_join_bwd(gout.data_ptr(), gl.data_ptr(), ls, gr.data_ptr(), b, cb, hw, code, sp()), "join"),
                                  lambda: torch.autograd.grad(eager_out, (la, ra), gout, retain_graph=True))
        for what, (native, eager) in calls.items():
            t = _time({"native": native, "eager": eager})
            for sidek, us in t.items():
                rec = dict(cfg=cfg, stage=stage, unit=unit, stride=stride, cin=cin, cout=cout, side=side, batch=b, dtype=args.dtype, call=what,
                           path=sidek, us_median=round(us[len(us) // 2], 2), us_min=round(us[0], 2), us_max=round(us[-1], 2), calls=CALLS,
                           rounds=ROUNDS)
                lines.append(rec)
                print(json.dumps(rec), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
