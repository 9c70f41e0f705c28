"""The EfficientNet MBConv tail on the GPU (csrc/ssdk_mbse.hip): each stage of ``ssdk_mbse`` on inputs of its own against fp64
from the operands as stored (tests/mbseaudit.py holds the bars and how they are derived), determinism, the chained call, and
the three EfficientNet detector cases as recorded plans.

Which instance or branch every layer takes (B0 @512 batch 32 and B0 @128; every one appears in the cases below):
  mbse_dw_kernel<DT, K>   K = 3: stages 1, 2, 4, 7; K = 5: stages 3, 5, 6.  Channel slices: C <= 256 is one slice of C / 8 octets
                          (32, 96, 144, 240: cases C = 8 ... 144); C = 480, 672, 1152 are 2, 3, 5 slices of 30, 28, 29 octets (case
                          C = 1152).  Maps: 256 x 256 ... 16 x 16 are whole tiles (cases 16 x 16, 67 x 35: several tiles with
                          tails; 15, 17: one under / over the tile); @128 the deep maps are 8 x 8 and 4 x 4, smaller than the
                          5 x 5 window's reach (cases 1 x 1, 2 x 3, 7 x 7).  Stride 2 on even and odd sizes (cases 7 x 7, 9 x 5, 67 x 35).
  mbse_gate_kernel        one instance.  T = 1 (all maps up to 16 x 16) and T > 1 (case (3, 16, 4) on the 67 x 35 partials: T = 15,
                          quarters of 4, 4, 4, 3); C <= 64 (one pass) and C = 1152 (18 passes); R = 1 ... 48.
  mbse_proj_kernel<DT, PT>  PT = 2 with 8 blocks of 16 output channels per wave where that grid fills the chip -- @512 batch 32
                          the stages 1 ... 5 (case 16 x 64 x 64: M = 65536 pixels); PT = 1 with 2 blocks everywhere else (all of
                          @128, stages 6, 7 of @512: cases 1 x 1, 7 x 7, 5 x 3, 33 x 31, 16 x 16).  K tails: C = 144 (16), 240 (16), 8 (8), 1152 / 96 / 32 (none); Cout tails: 40, 24
                          (8), 16 / 320 (none); fragments that straddle images: 7 x 7 and 5 x 3 maps; the pixel tail: 33 x 31.
"""
import os
import subprocess
import sys

import pytest
import torch

import cases_effnet
import mbseaudit
import nethelp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [torch.bfloat16, torch.float16]


def _pack(cin, cout, expand, k, stride, dtype, seed):
    from ssds.modeling.layers.fused_conv import MbSePack

    blk = mbseaudit.make_block(cin, cout, expand, k, stride, seed).cuda()
    return MbSePack(blk, dtype)


def _nhwc(t):
    return t.contiguous(memory_format=torch.channels_last)


def _judge(pk, x, res, out, dtype, stages):
    lines = []
    bad = mbseaudit.judge(pk, x, res, out, dtype, stages=stages, lines=lines)
    print("; ".join(lines))
    assert not bad, bad


# (N, C, H, W, k, stride); the last three: one under, at and one over the 16-pixel tile in both dimensions
STAGE1 = [(1, 8, 1, 1, 3, 1), (1, 8, 1, 1, 5, 2), (2, 40, 2, 3, 5, 1), (2, 24, 7, 7, 5, 2), (3, 144, 9, 5, 3, 2),
          (2, 1152, 7, 7, 5, 1), (1, 16, 67, 35, 5, 1), (1, 16, 67, 35, 3, 2), (1, 8, 15, 15, 3, 1), (2, 8, 16, 16, 5, 1),
          (1, 8, 17, 17, 5, 1)]


@pytest.mark.parametrize("i", range(len(STAGE1)))
def test_stage1_depthwise_and_pool_partials(i):
    from ssds import _native as N
    from ssds.modeling.layers import fused_conv as FC

    n, c, h, w, k, s = STAGE1[i]
    dtype = DTYPES[i % 2]
    pk = _pack(c, 8, 1, k, s, dtype, seed=100 + i)
    x = _nhwc(torch.randn(n, c, h, w, generator=torch.Generator().manual_seed(i)).cuda().to(dtype))
    a = FC.mbse_native(x, pk, stages=N.MBSE_DW)
    b = FC.mbse_native(x, pk, stages=N.MBSE_DW)
    torch.cuda.synchronize()
    assert N.last_kernel() == "mbse_dw_kernel"
    assert a["pool_partial"].shape[1] == N.lib.ssdk_mbse_pool_tiles(h, w, k, s)
    assert torch.equal(a["t"], b["t"]) and torch.equal(a["pool_partial"], b["pool_partial"])
    _judge(pk, x, None, a, dtype, 1)


# (N, C, R) and the map the partials come from
STAGE2 = [(1, 8, 1, (5, 4)), (3, 16, 4, (67, 35)), (2, 144, 6, (9, 5)), (2, 240, 10, (7, 7)), (2, 1152, 48, (7, 7))]


@pytest.mark.parametrize("i", range(len(STAGE2)))
def test_stage2_gate(i):
    from ssds import _native as N
    from ssds.modeling.layers import fused_conv as FC

    n, c, r, (h, w) = STAGE2[i]
    dtype = DTYPES[(i + 1) % 2]
    cin, expand = {8: (4, 2), 16: (16, 1), 144: (24, 6), 240: (40, 6), 1152: (192, 6)}[c]
    pk = _pack(cin, 8, expand, 5, 1, dtype, seed=200 + i)
    assert (pk.cin, pk.r) == (c, r)
    x = _nhwc(torch.randn(n, c, h, w, generator=torch.Generator().manual_seed(20 + i)).cuda().to(dtype))
    out = FC.mbse_native(x, pk, stages=N.MBSE_DW)
    if (h, w) == (67, 35):
        assert out["pool_partial"].shape[1] == 15
    gates = []
    for _ in range(2):
        out["gate"] = torch.full((n, c), -1.0, device="cuda")
        FC.mbse_native(x, pk, stages=N.MBSE_GATE, t=out["t"], pool_partial=out["pool_partial"], gate=out["gate"])
        gates.append(out["gate"])
    torch.cuda.synchronize()
    assert N.last_kernel() == "mbse_gate_kernel" and torch.equal(gates[0], gates[1])
    _judge(pk, x, None, out, dtype, 2)


# (N, H, W, C, Cout, residual); the last one reaches the 32-pixel x 128-channel instance (M = 65536 pixels)
STAGE3 = [(1, 1, 1, 8, 8, False), (3, 7, 7, 240, 40, True), (2, 5, 3, 144, 24, True), (2, 7, 7, 1152, 320, False),
          (1, 33, 31, 32, 16, False), (2, 16, 16, 96, 24, False), (16, 64, 64, 32, 16, False)]


@pytest.mark.parametrize("i", range(len(STAGE3)))
def test_stage3_gated_projection(i):
    from ssds import _native as N
    from ssds.modeling.layers import fused_conv as FC

    n, h, w, c, cout, residual = STAGE3[i]
    dtype = DTYPES[i % 2]
    cin, expand = {8: (4, 2), 240: (40, 6), 144: (24, 6), 1152: (192, 6), 32: (32, 1), 96: (16, 6)}[c]
    pk = _pack(cin, cout, expand, 3, 1, dtype, seed=300 + i)
    assert (pk.cin, pk.cout, pk.residual) == (c, cout, residual)
    g = torch.Generator().manual_seed(30 + i)
    t = _nhwc(torch.randn(n, c, h, w, generator=g).cuda().to(dtype))
    res = _nhwc(torch.randn(n, cout, h, w, generator=g).cuda().to(dtype)) if residual else None
    # a hand-made gate that differs strongly between images: image j's gate is scaled by 1 / (j + 1), image 0 also reversed
    gate = torch.rand(n, c, generator=g) * 0.9 + 0.05
    gate = gate / torch.arange(1, n + 1).view(-1, 1).float()
    gate[0] = gate[0].flip(0)
    gate = gate.cuda().contiguous()
    ys = []
    for _ in range(2):
        y = torch.full((n, cout, h, w), float("nan"), device="cuda", dtype=dtype).contiguous(memory_format=torch.channels_last)
        FC.mbse_native(t, pk, residual=res, stages=N.MBSE_PROJ, t=t, gate=gate, y=y)
        ys.append(y)
    torch.cuda.synchronize()
    assert N.last_kernel() == "mbse_proj_kernel" and torch.equal(ys[0], ys[1])
    _judge(pk, t, res, dict(t=t, gate=gate, y=ys[0]), dtype, 4)


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_chained_call_equals_the_three_stages(dtype):
    from ssds import _native as N
    from ssds.modeling.layers import fused_conv as FC

    pk = _pack(40, 40, 6, 5, 1, dtype, seed=7)
    g = torch.Generator().manual_seed(8)
    x = _nhwc(torch.randn(3, 240, 19, 17, generator=g).cuda().to(dtype))
    res = _nhwc(torch.randn(3, 40, 19, 17, generator=g).cuda().to(dtype))
    whole = FC.mbse_native(x, pk, residual=res)
    torch.cuda.synchronize()
    assert N.last_kernel() == "mbse_dw_kernel+mbse_gate_kernel+mbse_proj_kernel"
    parts = FC.mbse_native(x, pk, stages=N.MBSE_DW)
    FC.mbse_native(x, pk, stages=N.MBSE_GATE, t=parts["t"], pool_partial=parts["pool_partial"], gate=parts["gate"])
    FC.mbse_native(x, pk, residual=res, stages=N.MBSE_PROJ, t=parts["t"], gate=parts["gate"], y=parts["y"])
    torch.cuda.synchronize()
    for k in ("t", "pool_partial", "gate", "y"):
        assert torch.equal(whole[k], parts[k]), k
    _judge(pk, x, res, whole, dtype, 7)


# ---- whole nets ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["bfloat16", "float16"])
@pytest.mark.parametrize("name", list(cases_effnet.NET_CASES))
def test_plan_matches_reference_module(name, dtype):
    from test_gpu_nets import POOL_DRAWS, SMALL, _check_against_floor, check_small_levels_pooled, floor_runs

    from ssds.modeling.layers import fused_conv as FC

    tdt = getattr(torch, dtype)
    model, x, fx = mbseaudit.build_case(name)
    wl, wc = nethelp.want(fx)
    model = model.cuda().to(tdt)
    xd = x.cuda().to(tdt)
    before, plans, fallback = FC.STATS["native_layers"], FC.STATS["plan_runs"], FC.STATS["torch_fallback_layers"]
    with torch.no_grad():
        loc, conf = model(xd)
        loc2, conf2 = model(xd)
    assert FC.STATS["native_layers"] > before, "nothing ran on the HIP kernels"
    assert FC.STATS["plan_runs"] >= plans + 2, "the forward did not run as a recorded plan"
    assert FC.STATS["torch_fallback_layers"] == fallback == 0
    for i in range(len(loc)):
        assert loc[i].is_contiguous() and conf[i].is_contiguous() and loc[i].dtype == tdt
        assert torch.equal(loc[i], loc2[i]) and torch.equal(conf[i], conf2[i]), "replay is not deterministic"
    n0 = FC.STATS["native_layers"]
    floor = floor_runs(model, xd)
    assert FC.STATS["native_layers"] == n0
    report = _check_against_floor({"loc": loc, "conf": conf}, floor, {"loc": wl, "conf": wc}, name, dtype)
    print(name, dtype, "; ".join(report))
    if any(w.numel() < SMALL for w in wl + wc):
        cpu_model, _, _ = mbseaudit.build_case(name)
        cpu = lambda t: t.float().cpu()  # noqa: E731
        plans, floors, wants = [{"loc": [cpu(t) for t in loc], "conf": [cpu(t) for t in conf]}], [
            {"loc": [cpu(t) for t in floor[0]["loc"]], "conf": [cpu(t) for t in floor[0]["conf"]]}], [{"loc": wl, "conf": wc}]
        g = torch.Generator().manual_seed(4711)
        for _ in range(POOL_DRAWS):
            xi = torch.rand(x.shape, generator=g)
            with torch.no_grad():
                cl, cc = cpu_model(xi)
                pl, pc = model(xi.cuda().to(tdt))
            fl = floor_runs(model, xi.cuda().to(tdt), runs=1)[0]
            wants.append({"loc": list(cl), "conf": list(cc)})
            plans.append({"loc": [cpu(t) for t in pl], "conf": [cpu(t) for t in pc]})
            floors.append({"loc": [cpu(t) for t in fl["loc"]], "conf": [cpu(t) for t in fl["conf"]]})
        assert check_small_levels_pooled(plans, floors, wants, name, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_every_mbse_op_of_the_plan_is_at_its_rounding_level(dtype):
    import planaudit

    model, x, _ = mbseaudit.build_case("bifpn_effb0")
    model = model.cuda().to(dtype)
    xd = x.cuda().to(dtype)
    with torch.no_grad():
        plan = model._build_neck_plan(None, image=xd)
    rows = mbseaudit.audit_plan(plan, [xd])
    print(planaudit.format_rows(rows))
    assert len(rows) == 16 and all(r["kernel"] == "mbse_dw+mbse_gate+mbse_proj" for r in rows)
    assert not planaudit.failures(rows, dtype), planaudit.failures(rows, dtype)
    # the plan's own single call names the three kernels for every block
    ctx = plan.ctx
    ctx.set_side_lane(False)
    ctx.set_op_profiling(True)
    try:
        plan.launch()
        torch.cuda.synchronize()
        names = [k for k, _ in ctx.op_timings()]
    finally:
        ctx.set_op_profiling(False)
        ctx.set_side_lane(None)
    joined = " ".join(names)
    assert all(k in joined for k in ("mbse_dw_kernel", "mbse_gate_kernel", "mbse_proj_kernel", "conv_first_kernel")), names


def test_graphed_inference_replays_eager_bit_for_bit():
    from collections import OrderedDict

    from ssds.modeling.layers import box
    from ssds.modeling.layers.decoder import Decoder
    from ssds.utils.graph import GraphedInference

    model, x, _ = mbseaudit.build_case("bifpn_effb0")
    model = model.cuda().to(torch.float16)
    anchors = OrderedDict((s, box.generate_anchors(s, [1, 2, 0.5], [2.0, 2.52, 3.175])) for s in (8, 16, 32, 64, 128))
    dec = Decoder(0.005, 0.6, 50, 100, True, True)
    x0 = x.cuda().to(torch.float16)
    g = GraphedInference(model, dec, anchors, x0)
    torch.manual_seed(1)
    xi = torch.rand(x.shape, device="cuda").to(torch.float16)
    got = [t.clone() for t in g(xi)]
    with torch.no_grad():
        want = dec(*model(xi), anchors)
    for a, b in zip(got, want):
        assert torch.equal(a, b)


def test_ssd_detector_on_uint8_images():
    from ssds.ssds import SSDDetector

    det = SSDDetector(os.path.join(ROOT, "experiments", "cfgs", "bifpn_efficientnetb0_512.yml"))
    import numpy as np

    from ssds.modeling.layers import fused_conv as FC

    imgs = np.random.RandomState(0).randint(0, 256, (2, 512, 512, 3)).astype(np.uint8)

    runs = FC.STATS["plan_runs"]
    out = det(imgs)
    assert FC.STATS["plan_runs"] == runs + 1 and FC.STATS["torch_fallback_layers"] == 0
    assert len(out) == 3 and out[0].shape == (2, 100) and out[1].shape == (2, 100, 4)


# ---- training ------------------------------------------------------------------------------------------------------------------
_TRAIN = r"""
import sys, torch
sys.path[:0] = [%(root)r, %(pkg)r]
from ssds.core import config
from ssds.utils import train_ddp
cfg = config.cfg_from_file(%(cfg)r)
s = train_ddp.Solver(cfg, 0, torch.device("cuda", 0))
net = s.model
net.train()
# drop-connect (rate 0.2) draws one keep / drop per sample and residual block: with a batch of 2 a block loses BOTH samples with
# probability 0.04, and its parameters then have gradients of exactly zero.  The seed is the first under which every one of the
# nine residual blocks keeps a sample (the same draws in the same order as the forward below makes them).
def draws(seed):
    torch.manual_seed(seed)
    x = torch.randn(2, 3, 128, 128, device="cuda")
    return x, [float((0.8 + torch.rand(2, 1, 1, 1, device="cuda")).floor().sum()) for _ in range(9)]
seed = next(sd for sd in range(64) if min(draws(sd)[1]) > 0)
x, _ = draws(seed)
torch.manual_seed(seed)
torch.randn(2, 3, 128, 128, device="cuda")
with torch.autocast("cuda", dtype=torch.bfloat16):
    outs = net(x)
flat = []
def walk(o):
    if torch.is_tensor(o):
        flat.append(o)
    elif isinstance(o, (list, tuple)):
        for v in o:
            walk(v)
    elif isinstance(o, dict):
        for v in o.values():
            walk(v)
walk(outs)
loss = sum(o.float().pow(2).mean() for o in flat if o.requires_grad)
loss.backward()
torch.cuda.synchronize()
scope = [s.strip() for s in cfg.TRAIN.TRAINABLE_SCOPE.replace(";", ",").split(",") if s.strip()]
params = [(k, p) for k, p in net.named_parameters() if any(k.startswith(sc + ".") for sc in scope)]
missing = [k for k, p in params if p.grad is None]
bad = [k for k, p in params if p.grad is not None and not (bool(torch.isfinite(p.grad).all()) and float(p.grad.float().norm()) > 0)]
nbackbone = sum(1 for k, _ in params if k.startswith("backbone."))
print("RESULT", int(bool(torch.isfinite(loss))), len(params), len(list(net.parameters())), nbackbone, len(missing), len(bad),
      (missing + bad)[:6])
"""


def test_one_training_step_through_the_solver():
    code = _TRAIN % dict(root=ROOT, pkg=os.path.join(ROOT, "ssds.pytorch_amd"),
                         cfg=os.path.join(ROOT, "experiments", "cfgs", "bifpn_efficientnetb0_512.yml"))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    line = [l for l in out.stdout.splitlines() if l.startswith("RESULT")][-1].split(None, 7)
    finite, nparams, ntotal, nbackbone, missing, bad = (int(v) for v in line[1:7])
    # the scope names every top-level module, so it selects every parameter of the detector.  B0's backbone alone has 208: the
    # stem 3, the expand-free first block 10 (depthwise 1 + BN 2, SE 4, projection 1 + BN 2), the other 15 blocks 13 each
    assert nparams == ntotal and nbackbone == 3 + 10 + 15 * 13, line
    assert finite == 1 and missing == 0 and bad == 0, line
