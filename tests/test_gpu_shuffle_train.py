"""The ShuffleNetV2 training step on the GPU (csrc/ssdk_shuffletrain.hip, ssds/modeling/layers/shuffletrain.py): the 1x1 kernels on
channel slices of any width against fp64 per element, guard bands around every buffer, the join against torch's expressions bit
for bit, whole units in train mode under bf16 autocast against the fp64 CPU unit, graph capture, and the Solver's switch.

Bars.  Outputs and input gradients (tests/dwjudge.py): |err| <= eps |want| + 4 eps rms(want), eps 2^-8 (bf16) | 2^-10 (fp16), per
element.  Weight gradient: |err| <= D u M per element, u = 2^-24, M the fp64 mass sum |dy| |x|, D = shuffletrain.wgrad_sum_depth
(derived from the kernels' summation structure next to that function).  Statistics: the form of dwjudge's bars with the depths
of THESE kernels (shuffletrain.stats_sum_depth, gemm_sum_depth): |sum err| <= Ds u S|y| + Dy u S(My), |sumsq err| <= Ds u S(y^2) +
2 Dy u S(|y| My), My the fp64 mass of an output."""
import copy
import functools
import os
import subprocess
import sys

import pytest

import guardband as G
import shufflejudge as SJ

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
EPS = {"bf16": 2.0 ** -8, "f16": 2.0 ** -10}
DTYPE_NAMES = ("bf16", "f16")
# (B, C_total, first channel of the slice, K, M, H, W)
SLICES = [
    (2, 116, 58, 58, 58, 7, 9),       # short K, K tail 2, pixel tail, 4-byte-aligned slice base
    (3, 244, 122, 122, 122, 13, 13),  # long K, K tail 2, odd plane
    (2, 232, 116, 116, 116, 5, 5),    # K tail 4
    (2, 48, 24, 24, 24, 5, 5),        # no tail; the slice alone; the streaming weight-gradient kernel
    (2, 116, 0, 116, 116, 10, 10),    # contiguous: a stride-2 unit's layers
    (2, 24, 0, 24, 58, 9, 9),         # contiguous, M tail
    (1, 464, 232, 232, 232, 16, 8),   # exactly one 128-pixel group, no tails anywhere
]


def _dt(name):
    import torch

    return {"bf16": torch.bfloat16, "f16": torch.float16}[name]


def _id(case):
    return "x".join(str(v) for v in case)


@functools.lru_cache(maxsize=None)
def _reference(case, name):
    """Operands (CPU, in the dtype; weights as fp32 masters of rounded values) and the fp64 truth of one slice case, computed once."""
    import torch
    import torch.nn.functional as F

    b, c, off, k, m, h, w = case
    dt = _dt(name)
    seed = 1000 * c + 10 * h + w + (0 if name == "bf16" else 5)
    x = SJ.tensor((b, c, h, w), dt, seed)
    wt = SJ.weights(m, k, dt, seed + 1)
    dy = SJ.tensor((b, m, h, w), dt, seed + 2)
    xs = x[:, off:off + k].double()
    w64 = wt.double()
    y = F.conv2d(xs, w64)
    my = F.conv2d(xs.abs(), w64.abs())
    dx = torch.einsum("mk,bmp->bkp", w64.view(m, k), dy.double().view(b, m, -1)).view(b, k, h, w)
    dw = torch.einsum("bmp,bkp->mk", dy.double().view(b, m, -1), xs.reshape(b, k, -1))
    mw = torch.einsum("bmp,bkp->mk", dy.double().abs().view(b, m, -1), xs.abs().reshape(b, k, -1))
    dims = (0, 2, 3)
    return dict(x=x, w=wt, dy=dy, y=y, dx=dx, dw=dw, Mw=mw, sums=torch.stack([y.sum(dims), y.pow(2).sum(dims)], 1),
                S_abs=y.abs().sum(dims), S_sq=y.pow(2).sum(dims), S_My=my.sum(dims), S_yMy=(y.abs() * my).sum(dims))


def _judge16(what, got, want, name):
    err = (got.double().cpu() - want).abs()
    bar = EPS[name] * want.abs() + 4 * EPS[name] * float(want.pow(2).mean().sqrt())
    print("%s: worst |err| / bar = %.3f" % (what, float((err / bar).max())))
    assert bool((err <= bar).all()), (what, int((~(err <= bar)).sum()))


def _judge_abs(what, got, want, bar):
    err = (got.double().cpu() - want).abs()
    print("%s: worst |err| / bar = %.3f" % (what, float((err / bar.clamp(min=1e-300)).max())))
    assert bool((err <= bar).all()), (what, int((~(err <= bar)).sum()))


def _bits(t):
    import torch

    return t.contiguous().view(torch.int16)


# ---- single kernels ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", DTYPE_NAMES)
@pytest.mark.parametrize("cout,cin", SJ.PREPARE_SHAPES)
def test_prepare_writes_the_padded_images(cout, cin, name):
    import torch
    from ssds.modeling.layers import shuffletrain as ST

    w = SJ.weights(cout, cin, _dt(name), 7 * cout + cin)
    want16, wantt16 = SJ.prepare_oracle(w.view(cout, cin).numpy())
    w16, wt16 = ST.prepare_weights(w.cuda(), _dt(name))
    torch.cuda.synchronize()
    assert tuple(w16.shape) == want16.shape and tuple(wt16.shape) == wantt16.shape and w16.dtype == wt16.dtype == _dt(name)
    assert torch.equal(w16.float().cpu(), torch.from_numpy(want16)) and torch.equal(wt16.float().cpu(), torch.from_numpy(wantt16))
    assert not w16[:, cin:].view(torch.int16).any() and not wt16[:, cout:].view(torch.int16).any()  # +0 bits in the padding


@pytest.mark.parametrize("name", DTYPE_NAMES)
@pytest.mark.parametrize("case", SLICES, ids=_id)
def test_forward_on_a_slice_and_its_statistics(case, name):
    import torch
    from ssds import _native as N
    from ssds.modeling.layers import shuffletrain as ST

    b, c, off, k, m, h, w = case
    r = _reference(case, name)
    hw, dev = h * w, torch.device("cuda")
    x = r["x"].cuda()
    code = N.dtype_code(x)
    w16, _ = ST.prepare_weights(r["w"].cuda(), x.dtype)
    eoff, stride = ST.slice_geometry(x.shape, off)
    ys = []
    for want_sums in (False, True, True):
        y = torch.full((b, m, h, w), float("nan"), device=dev, dtype=x.dtype)
        sums = ST.pws_forward(x.data_ptr() + 2 * eoff, stride, w16, None, y.data_ptr(), m * hw, b, k, m, hw, code, dev, want_sums)
        ys.append((y, sums))
    torch.cuda.synchronize()
    _judge16("y %s %s" % (_id(case), name), ys[0][0], r["y"], name)
    assert torch.equal(_bits(ys[0][0]), _bits(ys[1][0])), "the outputs with and without statistics differ"
    assert torch.equal(ys[1][1], ys[2][1]), "the statistics of two runs differ"
    assert b * ((hw + 127) // 128) <= 6  # one group per wave: stats_sum_depth(1)
    ds, dy_ = ST.stats_sum_depth(1), ST.gemm_sum_depth(k)
    sums = ys[1][1]
    assert tuple(sums.shape) == (m, 2)
    _judge_abs("sum", sums[:, 0], r["sums"][:, 0], ds * U * r["S_abs"] + dy_ * U * r["S_My"])
    _judge_abs("sumsq", sums[:, 1], r["sums"][:, 1], ds * U * r["S_sq"] + 2 * dy_ * U * r["S_yMy"])


@pytest.mark.parametrize("name", DTYPE_NAMES)
@pytest.mark.parametrize("case", SLICES, ids=_id)
def test_input_gradient_into_a_slice(case, name):
    import torch
    from ssds import _native as N
    from ssds.modeling.layers import shuffletrain as ST

    b, c, off, k, m, h, w = case
    r = _reference(case, name)
    hw, dev = h * w, torch.device("cuda")
    dy = r["dy"].cuda()
    _, wt16 = ST.prepare_weights(r["w"].cuda(), dy.dtype)
    gx = torch.full((b, c, h, w), -7.0, device=dev, dtype=dy.dtype)
    eoff, stride = ST.slice_geometry(gx.shape, off)
    ST.pws_forward(dy.data_ptr(), m * hw, wt16, None, gx.data_ptr() + 2 * eoff, stride, b, m, k, hw, N.dtype_code(dy), dev)
    torch.cuda.synchronize()
    _judge16("dx %s %s" % (_id(case), name), gx[:, off:off + k], r["dx"], name)
    rest = torch.cat((gx[:, :off], gx[:, off + k:]), 1)
    assert bool((rest == -7.0).all()), "channels outside the slice were written"


@pytest.mark.parametrize("name", DTYPE_NAMES)
@pytest.mark.parametrize("case", SLICES, ids=_id)
def test_weight_gradient_of_a_slice(case, name):
    import torch
    from ssds import _native as N
    from ssds.modeling.layers import shuffletrain as ST

    b, c, off, k, m, h, w = case
    r = _reference(case, name)
    hw, dev = h * w, torch.device("cuda")
    x, dy = r["x"].cuda(), r["dy"].cuda()
    eoff, stride = ST.slice_geometry(x.shape, off)
    tiled, _, cps = ST.wgrad_plan(b, m, k, hw)
    assert tiled == (case != (2, 48, 24, 24, 24, 5, 5) and case != (2, 24, 0, 24, 58, 9, 9)) and cps == 1
    runs = [ST.pws_wgrad(dy, x.data_ptr() + 2 * eoff, stride, b, m, k, hw, N.dtype_code(x), dev) for _ in range(2)]
    torch.cuda.synchronize()
    assert tuple(runs[0].shape) == (m, k, 1, 1) and runs[0].dtype == torch.float32
    assert torch.equal(runs[0].view(torch.int32), runs[1].view(torch.int32)), "two calls differ"
    _judge_abs("dW %s %s" % (_id(case), name), runs[0].view(m, k), r["dw"], ST.wgrad_sum_depth(cps) * U * r["Mw"])


@pytest.mark.parametrize("name", DTYPE_NAMES)
@pytest.mark.parametrize("case", SLICES[:2], ids=_id)
def test_guard_bands_of_the_slice_kernels(case, name):
    """x is a slice of a guarded tensor whose last image ends where the allocation's NaN guard begins, and its other half is NaN
    too: no NaN reaches y, sums or dW.  The input gradient writes the right half of a 0xFF-filled buffer only."""
    import torch
    from ssds import _native as N
    from ssds.modeling.layers import shuffletrain as ST

    b, c, off, k, m, h, w = case
    r = _reference(case, name)
    hw, dev = h * w, torch.device("cuda")
    gs = G.GuardSet(dev)
    xh = r["x"].clone()
    xh.view(torch.int16)[:, :off] = -1  # 0xFFFF: NaN in the half the kernels must not read
    x = gs.inp("x", xh)
    dy = gs.inp("dy", r["dy"])
    w16s, wt16s = ST.prepare_weights(r["w"].cuda(), x.dtype)
    w16, wt16 = gs.inp("w16", w16s), gs.inp("wt16", wt16s)
    y = gs.out("y", (b, m, h, w), x.dtype)
    gx = gs.out("gx", (b, c, h, w), x.dtype)
    dw = gs.out("dw", (m, k), torch.float32)
    sums = gs.out("sums", (m, 2), torch.float32)
    need_s = int(N.lib.ssdk_pws_stats_workspace_bytes(b, k, m, hw))
    need_w = int(N.lib.ssdk_pws_wgrad_workspace_bytes(b, m, k, hw))
    ws_s = gs.out("stats workspace", (need_s,), torch.uint8)
    ws_w = gs.out("wgrad workspace", (need_w,), torch.uint8)
    gs.arm()
    code, sp = N.dtype_code(x), N.stream_ptr(dev)
    eoff, stride = ST.slice_geometry(x.shape, off)
    L = N.lib
    N.check(L.ssdk_pws_forward(x.data_ptr() + 2 * eoff, stride, w16.data_ptr(), int(w16.shape[1]), None, y.data_ptr(), m * hw, sums.data_ptr(),
                               ws_s.data_ptr(), need_s, b, k, m, hw, code, sp), "pws_forward")
    N.check(L.ssdk_pws_forward(dy.data_ptr(), m * hw, wt16.data_ptr(), int(wt16.shape[1]), None, gx.data_ptr() + 2 * eoff, stride, None, None, 0,
                               b, m, k, hw, code, sp), "pws_forward (input gradient)")
    N.check(L.ssdk_pws_wgrad(dy.data_ptr(), x.data_ptr() + 2 * eoff, stride, dw.data_ptr(), ws_w.data_ptr(), need_w, b, m, k, hw, code, sp),
            "pws_wgrad")
    torch.cuda.synchronize()
    assert gs.problems() == []
    assert not G.has_nan(y) and not G.has_nan(sums) and not G.has_nan(dw) and not G.has_nan(gx[:, off:])
    assert bool((gx[:, :off].contiguous().view(torch.int16) == -1).all()), "the left half of the gradient buffer was written"
    _judge16("y", y, r["y"], name)
    _judge16("dx", gx[:, off:], r["dx"], name)


@pytest.mark.parametrize("hw", [(7, 9), (13, 13), (4, 4)], ids=lambda p: "%dx%d" % p)
@pytest.mark.parametrize("cb", [58, 122, 232])
def test_join_is_the_shuffle_of_the_concatenation(cb, hw):
    """join_fwd against channel_shuffle(cat((l, r), 1), 2) and join_bwd against the strided views of gy, bit for bit, left
    contiguous and as the first half of x, both dtypes, NaN and signed zeros among the values; guards around every buffer, and the
    backward into a half writes that half only."""
    import torch
    from ssds import _native as N
    from ssds.modeling.nets.shufflenet import channel_shuffle

    h, w = hw
    n, dev = 2, torch.device("cuda")
    for name in DTYPE_NAMES:
        dt = _dt(name)
        x = SJ.tensor((n, 2 * cb, h, w), dt, cb + h)
        right = SJ.tensor((n, cb, h, w), dt, cb + h + 1)
        gy = SJ.tensor((n, 2 * cb, h, w), dt, cb + h + 2)
        for t in (x, right, gy):
            flat = t.view(-1)
            flat[0], flat[1], flat[2], flat[-1], flat[-2] = float("nan"), -0.0, 0.0, float("nan"), -0.0
            flat[5] = float("inf")
        code = N.dtype_code(x.cuda())
        for half in (False, True):
            gs = G.GuardSet(dev)
            xs = gs.inp("x", x if half else x[:, :cb].contiguous())
            rs, gys = gs.inp("right", right), gs.inp("gy", gy)
            y = gs.out("y", (n, 2 * cb, h, w), dt)
            gl = gs.out("gleft", (n, 2 * cb if half else cb, h, w), dt)
            gr = gs.out("gright", (n, cb, h, w), dt)
            gr2 = gs.out("gright (no gleft)", (n, cb, h, w), dt)
            gs.arm()
            ls = (2 if half else 1) * cb * h * w
            sp = N.stream_ptr(dev)
            N.check(N.lib.ssdk_shuffle_join_fwd(xs.data_ptr(), ls, rs.data_ptr(), y.data_ptr(), n, cb, h * w, code, sp), "join_fwd")
            N.check(N.lib.ssdk_shuffle_join_bwd(gys.data_ptr(), gl.data_ptr(), ls, gr.data_ptr(), n, cb, h * w, code, sp), "join_bwd")
            N.check(N.lib.ssdk_shuffle_join_bwd(gys.data_ptr(), None, 0, gr2.data_ptr(), n, cb, h * w, code, sp), "join_bwd (no gleft)")
            torch.cuda.synchronize()
            assert gs.problems() == [], (name, half)
            want = channel_shuffle(torch.cat((x[:, :cb], right), 1), 2)
            assert torch.equal(_bits(y.cpu()), _bits(want)), (name, half, "forward")
            assert torch.equal(_bits(gl[:, :cb].cpu()), _bits(gy[:, 0::2])), (name, half, "gleft")
            assert torch.equal(_bits(gr.cpu()), _bits(gy[:, 1::2])) and torch.equal(_bits(gr2.cpu()), _bits(gy[:, 1::2])), (name, half, "gright")
            if half:
                assert bool((gl[:, cb:].contiguous().view(torch.int16) == -1).all()), "join_bwd wrote the right half"


# ---- units -------------------------------------------------------------------------------------------------------------------------
UNITS = [((116, 116, 1), (2, 116, 9, 7)), ((244, 244, 1), (2, 244, 5, 5)), ((24, 116, 2), (2, 24, 10, 10)), ((232, 464, 2), (2, 232, 6, 6))]


def _rel(a, b):
    return float((a.double().cpu() - b.double()).norm() / b.double().norm().clamp(min=1e-12))


def _swapped(unit, native):
    """The Solver's swaps on a copy of ``unit`` on the GPU, in its order; ``native``: with use_native_shuffle."""
    from ssds.modeling.layers import shuffletrain as ST
    from ssds.modeling.layers.batchnorm import fuse_bn_activations, use_fast_batchnorm
    from ssds.modeling.layers.pointwise import fuse_conv_bn_statistics, use_pointwise_gemm

    m = copy.deepcopy(unit).float().cuda().train()
    use_fast_batchnorm(m)
    fuse_bn_activations(m)
    if native:
        ST.use_native_shuffle(m)
    use_pointwise_gemm(m)
    fuse_conv_bn_statistics(m)
    return m


def _unit_run(m, x, device, requires_grad=True):
    import torch

    x = x.to(device).to(torch.float32 if device == "cuda" else torch.float64).requires_grad_(requires_grad)
    ctx = torch.autocast("cuda", dtype=torch.bfloat16) if device == "cuda" else torch.autocast("cpu", enabled=False)
    with ctx:
        y = m(x * 1.0)  # (the unit's input is not a leaf: a leaf's gradient is accumulated by a copy)
    (y.float() if device == "cuda" else y).pow(2).mean().backward()
    if device == "cuda":
        torch.cuda.synchronize()
    res = {"output": y.detach()}
    if requires_grad:
        res["input.grad"] = x.grad
    res.update({k + ".grad": p.grad for k, p in m.named_parameters() if p.requires_grad})
    return res


@pytest.mark.parametrize("cfg,shape", UNITS, ids=lambda v: "-".join(str(i) for i in v))
def test_unit_in_train_mode(cfg, shape):
    """A flagged unit with the Solver's swaps, train mode, bf16 autocast, against the fp64 CPU unit: per tensor (output, input
    gradient, every parameter gradient) rel(native) <= 2 rel(floor) + 0.02, the floor being the same autocast unit as it runs
    without use_native_shuffle (the rule of tests/test_gpu_yolo_train.py::test_whole_neck_in_train_mode)."""
    import torch
    from ssds.modeling.layers import shuffletrain as ST
    from ssds.modeling.nets.shufflenet import InvertedResidual

    torch.manual_seed(11)
    unit = InvertedResidual(*cfg).train()
    image = torch.randn(*shape)
    want = _unit_run(copy.deepcopy(unit).double(), image, "cpu")
    native = _swapped(unit, True)
    assert native.native_shuffle
    calls = dict(ST.STATS)
    got = _unit_run(native, image, "cuda")
    delta = {k: ST.STATS[k] - calls[k] for k in calls if k.endswith("ward")}
    s1 = 1 if cfg[2] == 1 else 0
    assert delta == dict(slice_forward=s1, slice_backward=s1, join_forward=1, join_backward=1), "the native path did not run"
    calls = dict(ST.STATS)
    floor = _unit_run(_swapped(unit, False), image, "cuda")
    assert dict(ST.STATS) == calls
    assert set(got) == set(want) == set(floor)
    bad = []
    for k in sorted(want):
        rn, rf = _rel(got[k], want[k]), _rel(floor[k], want[k])
        print("%s %-28s rel native %.5f floor %.5f" % (cfg, k, rn, rf))
        if not rn <= 2.0 * rf + 0.02:
            bad.append((k, rn, rf))
    assert not bad, bad


def test_unit_variants():
    """A stride-1 unit whose input needs no gradient (no buffer, gleft NULL), whose first 1x1 weight is frozen, and two forward
    passes before the two backward passes: the gradients are those of the plain unit run the same way, under the rule above."""
    import torch
    from ssds.modeling.layers import shuffletrain as ST
    from ssds.modeling.nets.shufflenet import InvertedResidual

    torch.manual_seed(12)
    unit = InvertedResidual(116, 116, 1).train()
    image = torch.randn(2, 116, 9, 7)

    def check(got, want, floor, what):
        assert set(got) == set(want) == set(floor), what
        for k in sorted(want):
            rn, rf = _rel(got[k], want[k]), _rel(floor[k], want[k])
            print("%s %-28s rel native %.5f floor %.5f" % (what, k, rn, rf))
            assert rn <= 2.0 * rf + 0.02, (what, k, rn, rf)

    # the input needs no gradient
    calls = dict(ST.STATS)
    got = _unit_run(_swapped(unit, True), image, "cuda", requires_grad=False)
    assert ST.STATS["join_backward"] == calls["join_backward"] + 1 and ST.STATS["slice_backward"] == calls["slice_backward"] + 1
    check(got, _unit_run(copy.deepcopy(unit).double(), image, "cpu", False), _unit_run(_swapped(unit, False), image, "cuda", False), "no input grad")
    # the first 1x1's weight frozen
    frozen = copy.deepcopy(unit)
    frozen.branch2[0].weight.requires_grad_(False)
    got = _unit_run(_swapped(frozen, True), image, "cuda")
    assert "branch2.0.weight.grad" not in got and "input.grad" in got
    check(got, _unit_run(copy.deepcopy(frozen).double(), image, "cpu"), _unit_run(_swapped(frozen, False), image, "cuda"), "frozen weight")

    # two forward passes, then two backward passes
    def twice(m, device):
        dt = torch.float32 if device == "cuda" else torch.float64
        xs = [(image * s).to(device).to(dt).requires_grad_(True) for s in (1.0, 0.5)]
        ctx = torch.autocast("cuda", dtype=torch.bfloat16) if device == "cuda" else torch.autocast("cpu", enabled=False)
        with ctx:
            ys = [m(x * 1.0) for x in xs]
        for y in ys:
            y.double().pow(2).mean().backward()
        res = {"input%d.grad" % i: x.grad for i, x in enumerate(xs)}
        res.update({"output%d" % i: y.detach() for i, y in enumerate(ys)})
        res.update({k + ".grad": p.grad for k, p in m.named_parameters()})
        return res

    calls = dict(ST.STATS)
    got = twice(_swapped(unit, True), "cuda")
    assert {k: ST.STATS[k] - calls[k] for k in calls if k.endswith("ward")} == dict(slice_forward=2, slice_backward=2, join_forward=2, join_backward=2)
    check(got, twice(copy.deepcopy(unit).double(), "cpu"), twice(_swapped(unit, False), "cuda"), "two forwards")


def test_graph_capture_replays_a_unit():
    """Forward + backward of one flagged stride-1 unit captured in a torch.cuda.graph and replayed with two inputs: outputs and
    gradients equal the eager runs bit for bit."""
    import torch
    from ssds.modeling.nets.shufflenet import InvertedResidual

    torch.manual_seed(13)
    m = _swapped(InvertedResidual(116, 116, 1).train(), True)
    for mod in m.modules():
        if hasattr(mod, "momentum") and hasattr(mod, "running_mean"):
            mod.momentum = 0.0  # (the running statistics are not part of what is compared; they stay put across the runs)
    params = [p for p in m.parameters()]
    inputs = [torch.randn(2, 116, 9, 7, generator=torch.Generator().manual_seed(s)).bfloat16() for s in (1, 2)]
    x = inputs[0].clone().cuda().requires_grad_(True)

    def step():
        with torch.autocast("cuda", dtype=torch.bfloat16):
            y = m(x)
        grads = torch.autograd.grad(y.float().pow(2).mean(), [x] + params)
        return (y,) + tuple(grads)

    eager = []
    for inp in inputs:
        with torch.no_grad():
            x.copy_(inp)
        eager.append([t.detach().clone() for t in step()])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up on a side stream, as torch.cuda.graph asks
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step()
    for i in (1, 0):
        with torch.no_grad():
            x.copy_(inputs[i])
        graph.replay()
        torch.cuda.synchronize()
        for j, (got, want) in enumerate(zip(outs, eager[i])):
            same = torch.equal(got.view(torch.int16 if got.element_size() == 2 else torch.int32),
                               want.view(torch.int16 if want.element_size() == 2 else torch.int32))
            assert same, (i, j)


# ---- the switch ----------------------------------------------------------------------------------------------------------------------
_SWITCH = r"""
import sys, math, torch
sys.path[:0] = [%(root)r, %(pkg)r]
from ssds.core import config
from ssds.utils import train_ddp
from ssds.modeling.layers import shuffletrain as ST
cfg = config.cfg_from_file(%(cfg)r)
s = train_ddp.Solver(cfg, 0, torch.device("cuda", 0))
net = s.model
net.train()
x = torch.randn(2, 3, 128, 128, device="cuda")
with torch.autocast("cuda", dtype=torch.bfloat16):
    loc, conf = net(x)
loss = sum(o.float().pow(2).mean() for o in tuple(loc) + tuple(conf))
s.optimizer.zero_grad()
loss.backward()
s.optimizer.step()
torch.cuda.synchronize()
grads = [p.grad for p in net.parameters() if p.grad is not None]
finite = math.isfinite(float(loss)) and all(bool(torch.isfinite(g).all()) for g in grads)
print("RESULT", ST.STATS["units"], ST.STATS["depthwise"], ST.STATS["pointwise"], ST.STATS["slice_forward"], ST.STATS["slice_backward"],
      ST.STATS["join_forward"], ST.STATS["join_backward"], int(finite), len(grads))
"""


@pytest.mark.parametrize("cfg_name", ["fpn_shufflenetv2_x1_512.yml", "yolov3_shufflenetv2_x2_416.yml"])
@pytest.mark.parametrize("switch", ["0", "1"])
def test_the_switch(cfg_name, switch):
    """The Solver-built model of each shipped ShuffleNetV2 config takes one training step (forward, backward, optimizer) at batch 2
    and image size 128, in a subprocess: with SSDK_SHUFFLE_TRAIN=1 the kernels run (16 joins, 13 slice convolutions, as many backward
    as forward calls) and the loss and gradients are finite; with 0 every counter is zero."""
    env = dict(os.environ, SSDK_SHUFFLE_TRAIN=switch)
    code = _SWITCH % dict(root=ROOT, pkg=os.path.join(ROOT, "ssds.pytorch_amd"), cfg=os.path.join(ROOT, "experiments", "cfgs", cfg_name))
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    res = [int(v) for v in [l for l in out.stdout.splitlines() if l.startswith("RESULT")][-1].split()[1:]]
    units, dw, pw, sf, sb, jf, jb, finite, ngrads = res
    assert finite == 1 and ngrads > 0
    if switch == "0":
        assert res[:7] == [0] * 7
    else:
        assert (units, dw) == (16, 19) and pw >= 35 and sf == sb == 13 and jf == jb == 16
