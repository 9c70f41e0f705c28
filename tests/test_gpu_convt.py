"""The transposed 3x3 / stride 2 / pad 1 convolution (csrc/ssdk_convt.hip behind fused_conv.ConvTPack / convt_native) and the
Shelf detector's plans on the GPU.

Kernel: every case per element against ``F.conv_transpose2d`` (+ bias + skip) in fp64 on the CPU from the operands as stored
(16-bit x, weights and skip, fp32 bias).  The kernel accumulates in fp32 and rounds ONCE, after the skip add, so the bar is
the repository's one-rounding bar |err| <= eps |want| + 4 eps rms(want), eps = 2^-8 (bf16) | 2^-10 (fp16)
(test_gpu_dense3_train._rounding_bar).

Model: the recorded plan against the reference's fp32 outputs (tests/golden/net_shelf_*.npz) by the rule of
tests/test_gpu_nets.py -- the floor of PyTorch-ROCm running the same module in the same dtype."""
import pytest

import cases_shelf
import guardband as G
import nethelp

pytestmark = pytest.mark.gpu

# N, Cin, Cout, H, W, skip, bias
CASES = [
    (1, 8, 8, 1, 1, False, True),        # one class only, K = 8 < 32, Cout tail
    (2, 8, 24, 1, 3, True, True),        # a single row
    (2, 24, 8, 3, 1, True, False),       # a single column
    (3, 40, 24, 2, 2, True, True),       # fragments straddle images; k-steps straddle taps
    (2, 64, 40, 5, 4, True, True),
    (1, 512, 256, 5, 5, True, True),     # K = 2048 in the four-tap class
    (2, 256, 128, 17, 13, False, True),
    (1, 16, 16, 33, 31, True, True),     # several tiles with tails
    # the launch's other forms (the cases above are short of 256 workgroups: one class and 1, 2 or 4 channel blocks each):
    # 32 pixels per workgroup once that still gives 256 workgroups -- 66 150 pixels, with a pixel tail, rows of odd width and
    # two channel blocks of which the second is half empty -- and 16 pixels per workgroup walking all four classes
    (3, 8, 24, 150, 147, True, True),
    (2, 16, 8, 50, 47, True, True),    # 4 700 pixels: 294 workgroups of 16, 147 of 32
]
EPS = {"bfloat16": 2.0 ** -8, "float16": 2.0 ** -10}


def _dtype_of(i):
    return ("bfloat16", "float16")[i % 2]


def _operands(n, cin, cout, h, w, skip, bias, dtype, seed=0):
    """x, skip ~ N(0, 1), w ~ N(0, 1 / (2.25 Cin)) (2.25 taps per output pixel on average), bias ~ N(0, 1); module + tensors on
    the CPU, x / skip / weight holding values of ``dtype``."""
    import torch

    g = torch.Generator().manual_seed(1000 * cin + 10 * cout + 7 * h + 3 * w + n + seed)
    m = torch.nn.ConvTranspose2d(cin, cout, 3, stride=2, padding=1, bias=bias)
    with torch.no_grad():
        m.weight.copy_((torch.randn(m.weight.shape, generator=g) * (2.25 * cin) ** -0.5).to(dtype).float())
        if bias:
            m.bias.copy_(torch.randn(cout, generator=g))
    x = torch.randn(n, cin, h, w, generator=g).to(dtype)
    s = torch.randn(n, cout, 2 * h - 1, 2 * w - 1, generator=g).to(dtype) if skip else None
    return m, x, s


def _want(m, x, s):
    import torch.nn.functional as F

    y = F.conv_transpose2d(x.double(), m.weight.detach().double(), m.bias.detach().double() if m.bias is not None else None,
                           stride=2, padding=1)
    return y + s.double() if s is not None else y


def _run(m, x, s, **kw):
    import torch
    from ssds.modeling.layers import fused_conv as FC

    pk = FC.ConvTPack(m.cuda(), x.dtype)
    cl = lambda t: t.cuda().contiguous(memory_format=torch.channels_last)
    return FC.convt_native(cl(x), pk, cl(s) if s is not None else None, **kw), pk


@pytest.mark.parametrize("i", range(len(CASES)))
def test_kernel_against_fp64(i):
    import torch
    from ssds import _native as N
    from test_gpu_dense3_train import _rounding_bar

    n, cin, cout, h, w, skip, bias = CASES[i]
    dtype = _dtype_of(i)
    m, x, s = _operands(n, cin, cout, h, w, skip, bias, getattr(torch, dtype))
    want = _want(m, x, s)
    y, _ = _run(m, x, s)
    assert N.last_kernel() == "convt3x3s2_kernel"
    y2, _ = _run(m, x, s)
    torch.cuda.synchronize()
    assert tuple(y.shape) == (n, cout, 2 * h - 1, 2 * w - 1) and y.is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(y, y2), "two runs differ"
    _rounding_bar(y, want, EPS[dtype], "convt %s %s" % (CASES[i], dtype))


@pytest.mark.parametrize("act", ["relu", "sigmoid"])
def test_activation_goes_before_the_skip(act):
    """``act`` as in ssdk_conv_desc without res_mode: y = act(convT + bias) + skip."""
    import torch
    from test_gpu_dense3_train import _rounding_bar

    m, x, s = _operands(2, 24, 16, 4, 3, True, True, torch.bfloat16, seed=5)
    pre = _want(m, x, None)
    want = (torch.relu(pre) if act == "relu" else torch.sigmoid(pre)) + s.double()
    y, _ = _run(m, x, s, act=act)
    _rounding_bar(y, want, EPS["bfloat16"], "convt act " + act)


@pytest.mark.parametrize("i,with_skip", [(2, True), (7, True), (7, False), (4, False)])
def test_nothing_outside_the_output_is_written(i, with_skip):
    """y and skip sit between canary words: the kernel writes every element of y and nothing else, reads skip only inside its
    N (2H - 1) (2W - 1) Cout elements (the guards are NaN: one of them read would show in y) and not at all when it is NULL."""
    import torch
    from ssds.modeling.layers import fused_conv as FC
    from test_gpu_dense3_train import _rounding_bar

    n, cin, cout, h, w, _, bias = CASES[i]
    dtype = torch.float16 if i % 2 else torch.bfloat16
    m, x, s = _operands(n, cin, cout, h, w, with_skip, bias, dtype, seed=9)
    want = _want(m, x, s)
    ho, wo = 2 * h - 1, 2 * w - 1
    gs = G.GuardSet("cuda")  # (tests/guardband.py: views between NaN guards; inputs are snapshotted)
    y = gs.out("y", (n, cout, ho, wo), dtype, torch.channels_last)
    sk = gs.inp("skip", s.cuda().contiguous(memory_format=torch.channels_last)) if with_skip else None
    gs.arm()
    pk = FC.ConvTPack(m.cuda(), dtype)
    out = FC.convt_native(x.cuda().contiguous(memory_format=torch.channels_last), pk, sk, y=y)
    torch.cuda.synchronize()
    assert out.data_ptr() == y.data_ptr()
    assert gs.problems() == [], "a guard of y or of skip, or skip itself, was written"
    assert not torch.isnan(y).any(), "an element of y was not written, or a skip guard was read"
    _rounding_bar(y, want, 2.0 ** -10 if i % 2 else 2.0 ** -8, "guarded convt %s" % (CASES[i],))


def test_capture_and_replay_through_a_graph():
    import torch
    from ssds.modeling.layers import fused_conv as FC

    n, cin, cout, h, w, _, _ = CASES[4]
    m, x, s = _operands(n, cin, cout, h, w, True, True, torch.bfloat16, seed=3)
    eager, pk = _run(m, x, s)
    cl = lambda t: t.cuda().contiguous(memory_format=torch.channels_last)
    xs, ss, y = cl(x), cl(s), torch.zeros_like(eager)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        FC.convt_native(xs, pk, ss, y=y)  # (warm-up outside the capture)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        FC.convt_native(xs, pk, ss, y=y)
    y.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(y, eager)
    xs.copy_(cl(torch.flip(x, dims=[0])))  # new contents in the captured buffers
    graph.replay()
    torch.cuda.synchronize()
    again, _ = _run(m, torch.flip(x, dims=[0]), s)
    assert torch.equal(y, again)


# ---- the detector --------------------------------------------------------------------------------------------------------------
def _build(name, monkeypatch):
    monkeypatch.setattr(nethelp, "cases", cases_shelf)
    return nethelp.build(name)


@pytest.mark.parametrize("dtype", ["bfloat16", "float16"])
@pytest.mark.parametrize("name", list(cases_shelf.NET_CASES))
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
    which = "image -> heads" if key[0] == "image" else "neck only (backbone on PyTorch-ROCm)"
    refused = [p for p in model.__dict__["_neck_plans"].values() if isinstance(p, str)]
    print(name, dtype, "plan:", which, "| refused:", refused)
    rows = [r for r in plan.layer_table() if r["name"].startswith("convt ")]
    assert len(rows) == 4 and len(plan.layer_table()) == len(plan.layers)
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


def test_op_profiling_names_the_kernel(monkeypatch):
    import torch
    from ssds.modeling.layers import fused_conv as FC

    model, x, _ = _build("shelf_stub", monkeypatch)
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
    for (kern, ms), row in zip(timings, plan.layer_table()):
        assert (kern == "convt3x3s2_kernel") == row["name"].startswith("convt "), (kern, row["name"])
        assert ms >= 0
