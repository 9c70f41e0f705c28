"""The channel concatenation and the SPP block (csrc/ssdk_cat.hip behind fused_conv.cat_native / spp_native) and the YOLO detectors'
plans on the GPU.

Kernels: both are data movement and comparison, so every case is ``torch.equal`` against the torch expression it replaces on the
same channels_last tensors -- ``torch.cat((a, F.interpolate(b, scale_factor=2)), 1)`` / ``torch.cat((a, b), 1)`` and the four-way
cat of ``F.max_pool2d``.  The SPP inputs are ``randn - 3``: a padding value of 0 or a window that is not clipped to the map would win.

Models: the recorded plan against the reference's fp32 outputs (tests/golden/net_yolo*.npz) by the rule of tests/test_gpu_nets.py --
the floor of PyTorch-ROCm running the same module in the same dtype; there is no tolerance of this file's own."""
import pytest

import cases_yolo
import guardband as G
import nethelp

pytestmark = pytest.mark.gpu

UP2, SAME = True, False
# N, H, W, C1, C2, mode
CAT_CASES = [
    (1, 2, 2, 8, 8, UP2),         # one parent pixel
    (2, 6, 10, 24, 40, UP2),
    (3, 5, 7, 16, 8, SAME),       # odd sizes are fine at the same size
    (2, 16, 12, 32, 16, UP2),     # the golden stub's largest level
    (2, 2, 34, 8, 136, UP2),      # a pixel's octets straddle waves
    (1, 40, 40, 256, 128, UP2),   # yolov3_resnet18_320's largest level: many workgroups
]
# N, H, W, C
SPP_CASES = [
    (1, 1, 1, 8),       # a map of one pixel: every window is that pixel
    (2, 4, 3, 64),      # the golden stub's map, smaller than every window; two channel slices per image
    (1, 5, 3, 256),     # the golden ResNet18 case's map
    (2, 13, 13, 8),     # exactly the largest window
    (1, 16, 20, 24),    # 320 pixels: channel slices of 2 octets, the second one half empty
    (1, 7, 29, 16),
    (1, 40, 36, 8),     # more than one tile: halos cross tile borders in both directions
    (1, 10, 10, 256),
]
DTYPES = ["bfloat16", "float16"]


def _cl(t):
    import torch

    return t.contiguous(memory_format=torch.channels_last)


def _cat_operands(case, dtype, seed=0):
    import torch

    n, h, w, c1, c2, up2 = case
    g = torch.Generator().manual_seed(1000 * c1 + 10 * c2 + 7 * h + 3 * w + n + seed)
    a = torch.randn(n, c1, h, w, generator=g).to(dtype)
    b = torch.randn((n, c2, h // 2, w // 2) if up2 else (n, c2, h, w), generator=g).to(dtype)
    return _cl(a.cuda()), _cl(b.cuda())


def _cat_want(a, b, up2):
    import torch
    import torch.nn.functional as F

    return torch.cat((a, F.interpolate(b, scale_factor=2)), 1) if up2 else torch.cat((a, b), 1)


def _spp_operand(case, dtype, seed=0):
    import torch

    n, h, w, c = case
    g = torch.Generator().manual_seed(100 * c + 7 * h + 3 * w + n + seed)
    return _cl((torch.randn(n, c, h, w, generator=g) - 3.0).to(dtype).cuda())


def _spp_want(x):
    import torch
    import torch.nn.functional as F

    return torch.cat([x] + [F.max_pool2d(x, k, stride=1, padding=k // 2) for k in (5, 9, 13)], 1)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("i", range(len(CAT_CASES)))
def test_cat2_equals_the_torch_expression(i, dtype):
    import torch
    from ssds import _native as N
    from ssds.modeling.layers import fused_conv as FC

    n, h, w, c1, c2, up2 = CAT_CASES[i]
    a, b = _cat_operands(CAT_CASES[i], getattr(torch, dtype))
    want = _cat_want(a, b, up2)
    y = FC.cat_native(a, b, up2=up2)
    assert N.last_kernel() == "cat2_kernel"
    torch.cuda.synchronize()
    assert tuple(y.shape) == (n, c1 + c2, h, w) and y.dtype == a.dtype and y.is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(y, want), "cat2 %s %s" % (CAT_CASES[i], dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("i", range(len(SPP_CASES)))
def test_spp_equals_the_torch_expression(i, dtype):
    import torch
    from ssds import _native as N
    from ssds.modeling.layers import fused_conv as FC

    n, h, w, c = SPP_CASES[i]
    x = _spp_operand(SPP_CASES[i], getattr(torch, dtype))
    want = _spp_want(x)
    assert float(x.float().mean()) < -2.5  # (negative almost everywhere: a zero from the padding would be a maximum)
    y = FC.spp_native(x)
    assert N.last_kernel() == "spp_kernel"
    torch.cuda.synchronize()
    assert tuple(y.shape) == (n, 4 * c, h, w) and y.dtype == x.dtype and y.is_contiguous(memory_format=torch.channels_last)
    for s, k in enumerate((1, 5, 9, 13)):
        assert torch.equal(y[:, s * c:(s + 1) * c], want[:, s * c:(s + 1) * c]), "spp %s %s window %d" % (SPP_CASES[i], dtype, k)


@pytest.mark.parametrize("i,dtype", [(1, "bfloat16"), (2, "float16"), (4, "float16")])
def test_cat2_writes_y_and_nothing_else(i, dtype):
    """a, b and y sit between NaN guards: every element of y is written, nothing outside it, the sources are not written, and
    no guard is read (one NaN read would show in y)."""
    import torch
    from ssds.modeling.layers import fused_conv as FC

    tdt = getattr(torch, dtype)
    n, h, w, c1, c2, up2 = CAT_CASES[i]
    a, b = _cat_operands(CAT_CASES[i], tdt, seed=9)
    gs = G.GuardSet("cuda")  # (tests/guardband.py: views between NaN guards; inputs are snapshotted)
    cl = lambda t: t.cuda().contiguous(memory_format=torch.channels_last)  # noqa: E731
    ag, bg = gs.inp("a", cl(a)), gs.inp("b", cl(b))
    y = gs.out("y", (n, c1 + c2, h, w), tdt, torch.channels_last)
    gs.arm()
    out = FC.cat_native(ag, bg, up2=up2, y=y)
    torch.cuda.synchronize()
    assert out.data_ptr() == y.data_ptr()
    assert gs.problems() == [], "a source or a guard was written"
    assert not torch.isnan(y).any(), "an element of y was not written, or a guard was read"
    assert torch.equal(y, _cat_want(a, b, up2))


@pytest.mark.parametrize("i,dtype", [(1, "float16"), (4, "bfloat16"), (6, "bfloat16")])
def test_spp_writes_y_and_nothing_else(i, dtype):
    import torch
    from ssds.modeling.layers import fused_conv as FC

    tdt = getattr(torch, dtype)
    n, h, w, c = SPP_CASES[i]
    x = _spp_operand(SPP_CASES[i], tdt, seed=9)
    gs = G.GuardSet("cuda")
    xg = gs.inp("x", x.cuda().contiguous(memory_format=torch.channels_last))
    y = gs.out("y", (n, 4 * c, h, w), tdt, torch.channels_last)
    gs.arm()
    out = FC.spp_native(xg, y=y)
    torch.cuda.synchronize()
    assert out.data_ptr() == y.data_ptr()
    assert gs.problems() == [], "x or a guard was written"
    assert not torch.isnan(y).any(), "an element of y was not written, or a guard was read"
    assert torch.equal(y, _spp_want(x))


def _capture(fn):
    import torch

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()  # (warm-up outside the capture)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fn()
    return graph


def test_cat2_capture_and_replay_through_a_graph():
    import torch
    from ssds.modeling.layers import fused_conv as FC

    case = CAT_CASES[3]
    a, b = _cat_operands(case, torch.bfloat16, seed=3)
    eager = FC.cat_native(a, b, up2=case[5])
    y = torch.zeros_like(eager)
    graph = _capture(lambda: FC.cat_native(a, b, up2=case[5], y=y))
    y.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(y, eager)
    a.copy_(torch.flip(a, dims=[0]).clone())  # new contents in the captured buffers
    b.copy_((b * 2).clone())
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(y, _cat_want(a, b, case[5])) and not torch.equal(y, eager)


def test_spp_capture_and_replay_through_a_graph():
    import torch
    from ssds.modeling.layers import fused_conv as FC

    x = _spp_operand(SPP_CASES[4], torch.float16, seed=3)
    eager = FC.spp_native(x)
    y = torch.zeros_like(eager)
    graph = _capture(lambda: FC.spp_native(x, y=y))
    y.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(y, eager)
    x.copy_(torch.flip(x, dims=[2, 3]).clone())  # new contents in the captured buffer
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(y, _spp_want(x)) and not torch.equal(y, eager)


# ---- the detectors -------------------------------------------------------------------------------------------------------------
ROWS = {"yolov3_stub": (2, 0), "yolov4_stub": (8, 1), "yolov3_r18": (2, 0), "yolov4_r18": (4, 1)}  # cat, spp rows of the plan


def _build(name, monkeypatch):
    monkeypatch.setattr(nethelp, "cases", cases_yolo)
    return nethelp.build(name)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(cases_yolo.NET_CASES))
def test_plan_matches_reference_module(name, dtype, monkeypatch):
    import torch
    from ssds.modeling.layers import fused_conv as FC
    from test_gpu_nets import POOL_DRAWS, SMALL, _check_against_floor, check_small_levels_pooled, floor_runs

    tdt = getattr(torch, dtype)
    model, x, fx = _build(name, monkeypatch)
    wl, wc = nethelp.want(fx)
    model = model.cuda().to(tdt)
    xd = x.cuda().to(tdt)
    runs = FC.STATS["plan_runs"]
    with torch.no_grad():
        loc, conf = model(xd)
        loc2, conf2 = model(xd)
    assert FC.STATS["plan_runs"] == runs + 2, "the forward did not run as a recorded plan"
    plans = {k: p for k, p in model.__dict__["_neck_plans"].items() if isinstance(p, FC.ConvPlan)}
    assert len(plans) == 1
    (key, plan), = plans.items()
    refused = [p for p in model.__dict__["_neck_plans"].values() if isinstance(p, str)]
    print(name, dtype, "plan:", "image -> heads" if key[0] == "image" else "neck only", "| refused:", refused)
    if name.endswith("_r18"):
        assert key[0] == "image", "the ResNet18 backbone was not part of the plan: %s" % refused
    table = plan.layer_table()
    assert len(table) == len(plan.layers)
    assert (len([r for r in table if r["name"].startswith("cat ")]), len([r for r in table if r["name"].startswith("spp ")])) == ROWS[name]
    for a, b in zip(loc + conf, loc2 + conf2):
        assert a.is_contiguous() and a.dtype == tdt and torch.equal(a, b), "replay is not deterministic"
    # SSDK_FUSED_CONV=0 gives the module path (floor_runs sets it): no plan, no HIP kernel of this library
    n0, p0 = FC.STATS["native_layers"], FC.STATS["plan_runs"]
    floor = floor_runs(model, xd)
    assert FC.STATS["native_layers"] == n0 and FC.STATS["plan_runs"] == p0
    report = _check_against_floor({"loc": loc, "conf": conf}, floor, {"loc": wl, "conf": wc}, name, dtype)
    print(name, dtype, "; ".join(report))
    # small levels: pooled over POOL_DRAWS more inputs, as tests/test_gpu_nets.py does it
    assert any(t.numel() < SMALL for t in wl + wc)
    cpu_model, _, _ = _build(name, monkeypatch)
    cpu = lambda t: t.float().cpu()
    plans_o, floors, wants = [{"loc": [cpu(t) for t in loc], "conf": [cpu(t) for t in conf]}], [
        {"loc": [cpu(t) for t in floor[0]["loc"]], "conf": [cpu(t) for t in floor[0]["conf"]]}], [{"loc": wl, "conf": wc}]
    g = torch.Generator().manual_seed(4711)
    stub = isinstance(cpu_model.backbone, nethelp.StubBackbone)
    for _ in range(POOL_DRAWS):
        xi = torch.rand(x.shape, generator=g)
        if stub:  # (a stub backbone ignores the image: draw its feature maps instead)
            feats = [torch.randn(f.shape, generator=g) * 0.7 for f in cpu_model.backbone.feats]
            cpu_model.backbone.feats = feats
            model.backbone.feats = feats
        with torch.no_grad():
            cl_, cc_ = cpu_model(xi)
            pl, pc = model(xi.cuda().to(tdt))
        fl = floor_runs(model, xi.cuda().to(tdt), runs=1)[0]
        wants.append({"loc": list(cl_), "conf": list(cc_)})
        plans_o.append({"loc": [cpu(t) for t in pl], "conf": [cpu(t) for t in pc]})
        floors.append({"loc": [cpu(t) for t in fl["loc"]], "conf": [cpu(t) for t in fl["conf"]]})
    assert check_small_levels_pooled(plans_o, floors, wants, name, dtype)


@pytest.mark.parametrize("name", ["yolov3_stub", "yolov4_stub"])
def test_op_profiling_names_the_kernels(name, monkeypatch):
    import torch
    from ssds.modeling.layers import fused_conv as FC

    model, x, _ = _build(name, monkeypatch)
    model = model.cuda().to(torch.bfloat16)
    with torch.no_grad():
        model(x.cuda().to(torch.bfloat16))
        (plan,) = [p for p in model.__dict__["_neck_plans"].values() if isinstance(p, FC.ConvPlan)]
        plan.ctx.set_op_profiling(True)
        model(x.cuda().to(torch.bfloat16))
        torch.cuda.synchronize()
        timings = plan.ctx.op_timings()
        plan.ctx.set_op_profiling(False)
    assert len(timings) == len(plan.layers)
    seen = set()
    for (kern, ms), row in zip(timings, plan.layer_table()):
        assert (kern == "cat2_kernel") == row["name"].startswith("cat "), (kern, row["name"])
        assert (kern == "spp_kernel") == row["name"].startswith("spp "), (kern, row["name"])
        assert ms >= 0
        seen.add(kern)
    assert "cat2_kernel" in seen and ("spp_kernel" in seen) == (name == "yolov4_stub")
