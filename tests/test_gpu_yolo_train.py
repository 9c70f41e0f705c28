"""The YOLO-only operations of the TRAINING step on the GPU (csrc/ssdk_cattrain.hip behind ssds/modeling/layers/cattrain.py): channel
concatenation (with nearest x2) and the SPP block, forward and backward, per element against the eager torch expression under autograd
in fp64 on the CPU on the same 16-bit-rounded operands; exact integer and signed-zero routing cases; NaN; bit-reproducibility; hipGraph
capture; the autocast contract; operands the kernels decline; whole YOLOv3 / YOLOv4 necks in train mode against the PyTorch-ROCm floor;
and the switch.

Sources are relu(randn) rounded to the dtype: about half the elements are exact zeros, so window ties are everywhere (torch's fp64 CPU
backward of max_pool2d gives the first maximum in row-major window order, the kernels' rule); gy ~ N(0, 1).  Bars: everything that is
a copy is bit-equal; a sum of n fp32 terms rounded once is within eps |want| + n 2^-24 mass per element, mass being the same fp64
backward applied to |gy| (eps = 2^-8 bf16, 2^-10 f16; n = 4 for the 2 x 2 block of an UP2 source, n = 276 = 1 + 25 + 81 + 169 for the
longest SPP sum).  At (2, 8, 16, 16) bf16 the SPP bar spans 1e-6 ... 0.14 and bf16 eager autograd misses it by up to 92 x: the eager
path is no stand-in for the kernel here."""
import copy
import functools
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAME, UP2 = 0, 1

# (N, C1, C2, H, W); the last two are the configs' own concatenations at N = 2
CAT_SHAPES = [(1, 1, 1, 2, 2), (2, 3, 5, 6, 10), (1, 3, 2, 5, 7), (2, 5, 3, 2, 34), (2, 5, 3, 4, 66), (2, 128, 64, 40, 40), (2, 128, 128, 32, 32)]
CAT_CASES = [(s, m) for s in CAT_SHAPES for m in (SAME, UP2) if m == SAME or (s[3] % 2 == 0 and s[4] % 2 == 0)]
_cat_ids = ["%s-%s" % ("x".join(map(str, s)), "up2" if m else "same") for s, m in CAT_CASES]


def _max_side():
    from ssds import _native as N

    return N.SPP_TRAIN_MAX_SIDE


# (N, C, H, W); None: the stated plane limit itself at N = C = 1
SPP_SHAPES = [(1, 1, 1, 1), (2, 5, 4, 9), (1, 3, 13, 13), (1, 3, 14, 15), (2, 8, 16, 16), (1, 4, 20, 20), (1, 2, 33, 34), None]
_spp_ids = ["x".join(map(str, s)) if s else "limit" for s in SPP_SHAPES]


def _spp_shape(shape):
    return (1, 1, _max_side(), _max_side()) if shape is None else shape


def _dtype(name):
    import torch

    return (torch.bfloat16, 2.0 ** -8) if name == "bf16" else (torch.float16, 2.0 ** -10)


def _R(b, mode):
    import torch.nn.functional as F

    return F.interpolate(b, scale_factor=2, mode="nearest") if mode == UP2 else b


def _spp_eager(x):
    import torch
    import torch.nn.functional as F

    return torch.cat([x] + [F.max_pool2d(x, kernel_size=k, stride=1, padding=k // 2) for k in (5, 9, 13)], dim=1)


@functools.lru_cache(maxsize=4)
def _cat_case(shape, mode, dtype_name):
    """operands (a, b, gy) and the fp64 CPU truth (y, ga, gb, mass of gb); computed once per case, never modified."""
    import torch

    dtype, _ = _dtype(dtype_name)
    n, c1, c2, h, w = shape
    g = torch.Generator().manual_seed(1000 * h + 10 * w + c1 + 7 * mode)
    a = torch.relu(torch.randn(n, c1, h, w, generator=g)).to(dtype)
    b = torch.relu(torch.randn((n, c2, h // 2, w // 2) if mode == UP2 else (n, c2, h, w), generator=g)).to(dtype)
    gy = torch.randn(n, c1 + c2, h, w, generator=g).to(dtype)
    a64, b64 = a.double().requires_grad_(True), b.double().requires_grad_(True)
    y = torch.cat((a64, _R(b64, mode)), dim=1)
    ga, gb = torch.autograd.grad(y, (a64, b64), gy.double(), retain_graph=True)
    (mass,) = torch.autograd.grad(y, (b64,), gy.double().abs())
    return (a, b, gy), (y.detach(), ga, gb, mass)


def _cat_native(a, b, gy, mode):
    import torch
    from ssds.modeling.layers import cattrain as CT

    ad, bd = a.cuda().requires_grad_(True), b.cuda().requires_grad_(True)
    y = CT.cat2(ad, bd, mode)
    y.backward(gy.cuda())
    torch.cuda.synchronize()
    return y.detach(), ad.grad, bd.grad


def _bits(t):
    import torch

    return t.detach().cpu().contiguous().view(torch.int16)


def _sum_bar(got, want, mass, eps, terms, what):
    """A sum of ``terms`` fp32 terms rounded once: |got - want| <= eps |want| + terms 2^-24 mass per element."""
    err = (got.double().cpu() - want).abs()
    bar = eps * want.abs() + terms * 2.0 ** -24 * mass
    worst = float((err / bar.clamp(min=1e-300)).max())
    print("%s: worst |err| / bar = %.3f, bar %.3g ... %.3g" % (what, worst, float(bar.min()), float(bar.max())))
    assert bool((err <= bar).all()), "%s: %d elements outside the bar, worst %.3g of it" % (what, int((err > bar).sum()), worst)


@pytest.mark.parametrize("shape,mode", CAT_CASES, ids=_cat_ids)
@pytest.mark.parametrize("dtype_name", ["bf16", "f16"])
def test_cat(shape, mode, dtype_name):
    import torch
    from ssds import _native as N

    dtype, eps = _dtype(dtype_name)
    (a, b, gy), (y64, ga64, gb64, mass) = _cat_case(shape, mode, dtype_name)
    y, ga, gb = _cat_native(a, b, gy, mode)
    assert "cat_train" in N.last_kernel(), N.last_kernel()
    for t, s in ((y, y64), (ga, a), (gb, b)):
        assert t.dtype == dtype and t.is_contiguous() and tuple(t.shape) == tuple(s.shape)
    tag = "%s mode %d %s" % (shape, mode, dtype_name)
    assert torch.equal(_bits(y), _bits(y64.to(dtype))), "y " + tag  # (the truth is a copy of 16-bit values: its rounding is exact)
    assert torch.equal(_bits(ga), _bits(ga64.to(dtype))), "ga " + tag
    if mode == SAME:
        assert torch.equal(_bits(gb), _bits(gb64.to(dtype))), "gb " + tag
    else:
        _sum_bar(gb, gb64, mass, eps, 4, "gb " + tag)
    y2, ga2, gb2 = _cat_native(a, b, gy, mode)  # two runs: the same bits
    assert torch.equal(_bits(y), _bits(y2)) and torch.equal(_bits(ga), _bits(ga2)) and torch.equal(_bits(gb), _bits(gb2)), tag


def test_cat_backward_with_one_gradient():
    """Either output of the backward may be left out: the other one is unchanged."""
    import torch
    from ssds.modeling.layers import cattrain as CT

    (a, b, gy), _ = _cat_case((2, 3, 5, 6, 10), UP2, "bf16")
    _, ga, gb = _cat_native(a, b, gy, UP2)
    for which in (0, 1):
        ad, bd = a.cuda().requires_grad_(which == 0), b.cuda().requires_grad_(which == 1)
        CT.cat2(ad, bd, UP2).backward(gy.cuda())
        torch.cuda.synchronize()
        assert (ad.grad is None) == (which == 1) and (bd.grad is None) == (which == 0)
        assert torch.equal(ad.grad, ga) if which == 0 else torch.equal(bd.grad, gb)


@functools.lru_cache(maxsize=4)
def _spp_case(shape, dtype_name):
    """operands (x, gy) and the fp64 CPU truth (y, gx, mass); computed once per case, never modified."""
    import torch

    dtype, _ = _dtype(dtype_name)
    n, c, h, w = shape
    g = torch.Generator().manual_seed(1000 * h + 10 * w + c)
    x = torch.relu(torch.randn(n, c, h, w, generator=g)).to(dtype)
    gy = torch.randn(n, 4 * c, h, w, generator=g).to(dtype)
    return (x, gy), _spp_truth(x, gy)


def _spp_truth(x, gy):
    import torch

    x64 = x.double().requires_grad_(True)
    y = _spp_eager(x64)
    (gx,) = torch.autograd.grad(y, (x64,), gy.double(), retain_graph=True)
    (mass,) = torch.autograd.grad(y, (x64,), gy.double().abs())
    return y.detach(), gx, mass


def _spp_native(x, gy):
    import torch
    from ssds.modeling.layers import cattrain as CT

    xd = x.cuda().requires_grad_(True)
    y = CT.spp(xd)
    y.backward(gy.cuda())
    torch.cuda.synchronize()
    return y.detach(), xd.grad


def _same_numbers(got, want):
    """== per element in fp64, NaN positions equal."""
    got, want = got.double().cpu(), want.double()
    return bool(((got == want) | (got.isnan() & want.isnan())).all())


@pytest.mark.parametrize("shape", SPP_SHAPES, ids=_spp_ids)
@pytest.mark.parametrize("dtype_name", ["bf16", "f16"])
def test_spp(shape, dtype_name):
    import torch
    from ssds import _native as N

    shape = _spp_shape(shape)
    dtype, eps = _dtype(dtype_name)
    (x, gy), (y64, gx64, mass) = _spp_case(shape, dtype_name)
    y, gx = _spp_native(x, gy)
    assert "spp_train" in N.last_kernel(), N.last_kernel()
    assert y.dtype == gx.dtype == dtype and y.is_contiguous() and gx.is_contiguous()
    assert tuple(y.shape) == tuple(y64.shape) and tuple(gx.shape) == tuple(x.shape)
    tag = "%s %s" % (shape, dtype_name)
    assert _same_numbers(y, y64), "y " + tag
    _sum_bar(gx, gx64, mass, eps, 276, "gx " + tag)
    y2, gx2 = _spp_native(x, gy)  # two runs: the same bits
    assert torch.equal(_bits(y), _bits(y2)) and torch.equal(_bits(gx), _bits(gx2)), tag


@pytest.mark.parametrize("dtype_name", ["bf16", "f16"])
def test_spp_constant_plane_gives_exact_integers(dtype_name):
    """Every window of a constant plane sends its gradient to its first element: with gy = 1 the counts are exact integers."""
    import torch

    dtype, _ = _dtype(dtype_name)
    x = torch.full((1, 1, 6, 7), 1.5).to(dtype)
    gy = torch.ones(1, 4, 6, 7).to(dtype)
    _, gx64, _ = _spp_truth(x, gy)
    want = torch.tensor([[77, 9, 9, 4, 4, 1, 1], [9, 3, 3, 2, 2, 1, 1], [4, 2, 2, 2, 2, 1, 1], [4, 2, 2, 2, 2, 1, 1],
                         [1, 1, 1, 1, 1, 1, 1], [1, 1, 1, 1, 1, 1, 1]], dtype=torch.float64)
    assert torch.equal(gx64[0, 0], want)  # what torch's fp64 backward gives
    y, gx = _spp_native(x, gy)
    assert torch.equal(gx.double().cpu()[0, 0], want) and bool((y == 1.5).all())


@pytest.mark.parametrize("dtype_name", ["bf16", "f16"])
def test_spp_signed_zeros_compare_equal(dtype_name):
    """-0 == +0: the first zero of the window wins whatever its sign (an ordering with -0 < +0 would pick another element)."""
    import torch

    dtype, _ = _dtype(dtype_name)
    gy = torch.arange(1, 13, dtype=torch.float32).reshape(1, 4, 1, 3).to(dtype)
    for zeros in ([-0.0, 0.0, 0.0], [0.0, -0.0, 0.0]):
        x = torch.tensor(zeros).reshape(1, 1, 1, 3).to(dtype)
        _, gx64, _ = _spp_truth(x, gy)
        assert gx64.flatten().tolist() == [73.0, 2.0, 3.0]
        y, gx = _spp_native(x, gy)
        assert gx.double().cpu().flatten().tolist() == [73.0, 2.0, 3.0], zeros
        assert bool((y == 0).all())


@pytest.mark.parametrize("dtype_name", ["bf16", "f16"])
def test_spp_one_nan(dtype_name):
    """One NaN in x: every window that holds it is NaN, the others are equal to the truth; its gradient stays finite elsewhere."""
    import torch

    (x, gy), _ = _spp_case((1, 4, 20, 20), dtype_name)
    x = x.clone()
    x[0, 2, 7, 11] = float("nan")
    y64, gx64, _ = _spp_truth(x, gy)
    assert int(y64.isnan().sum()) == 1 + 25 + 81 + 169
    y, gx = _spp_native(x, gy)
    assert _same_numbers(y, y64)
    other = [0, 1, 3]
    assert bool(torch.isfinite(gx[0, other]).all()) and bool(torch.isfinite(gx[0, 2]).all())


def test_graph_capture_replays_both_ops():
    """Forward + backward of cat2 (UP2) and spp captured into one torch.cuda.graph on one stream: replay equals the eager call."""
    import torch
    from ssds.modeling.layers import cattrain as CT

    sets = []
    for seed in (1, 2):
        g = torch.Generator().manual_seed(seed)
        a, b = torch.relu(torch.randn(2, 3, 6, 10, generator=g)).bfloat16(), torch.relu(torch.randn(2, 5, 3, 5, generator=g)).bfloat16()
        gy = torch.randn(2, 8, 6, 10, generator=g).bfloat16()
        x = torch.relu(torch.randn(2, 5, 14, 15, generator=g)).bfloat16()
        gs = torch.randn(2, 20, 14, 15, generator=g).bfloat16()
        sets.append((a, b, gy, x, gs))
    eager = [(_cat_native(s[0], s[1], s[2], UP2), _spp_native(s[3], s[4])) for s in sets]
    bufs = [t.cuda() for t in sets[0]]
    for t in (bufs[0], bufs[1], bufs[3]):
        t.requires_grad_(True)
    a, b, gy, x, gs = bufs

    def step():
        y = CT.cat2(a, b, UP2)
        ga, gb = torch.autograd.grad(y, (a, b), gy)
        sy = CT.spp(x)
        (gx,) = torch.autograd.grad(sy, (x,), gs)
        return (y, ga, gb), (sy, gx)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up on a side stream, as torch.cuda.graph asks
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cat_out, spp_out = step()
    for i in (1, 0):
        with torch.no_grad():
            for dst, new in zip(bufs, sets[i]):
                dst.copy_(new)
        for t in cat_out + spp_out:
            t.detach().zero_()
        graph.replay()
        torch.cuda.synchronize()
        for got, want, what in zip(cat_out + spp_out, eager[i][0] + eager[i][1], ("y", "ga", "gb", "spp y", "gx")):
            assert torch.equal(_bits(got), _bits(want)), (i, what)


def test_autocast_contract():
    """fp32 operands under bf16 autocast take the kernels (after the cast); outside autocast they take the eager expressions."""
    import torch
    from ssds import _native as N
    from ssds.modeling.layers import cattrain as CT

    torch.manual_seed(0)
    a = torch.randn(2, 6, 8, 8, device="cuda", requires_grad=True)
    b = torch.randn(2, 4, 4, 4, device="cuda", requires_grad=True)
    x = torch.randn(2, 3, 8, 8, device="cuda", requires_grad=True)
    calls = dict(CT.STATS)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        y = CT.try_cat2(a, b, UP2)
        assert "cat_train_fwd" in N.last_kernel()
        s = CT.try_spp(x)
        assert "spp_train_fwd" in N.last_kernel()
    assert y is not None and s is not None and y.dtype == s.dtype == torch.bfloat16
    assert tuple(y.shape) == (2, 10, 8, 8) and tuple(s.shape) == (2, 12, 8, 8)
    want = torch.cat((a.detach().bfloat16(), torch.nn.functional.interpolate(b.detach().bfloat16(), scale_factor=2)), 1)
    assert torch.equal(y.detach(), want) and torch.equal(s.detach(), _spp_eager(x.detach().bfloat16()))
    (y.float().pow(2).mean() + s.float().pow(2).mean()).backward()
    torch.cuda.synchronize()
    assert {k: CT.STATS[k] - calls[k] for k in calls} == dict({k: 0 for k in calls}, cat_forward=1, cat_backward=1, spp_forward=1,
                                                                spp_backward=1)
    assert all(t.grad is not None and t.grad.dtype == torch.float32 and bool(torch.isfinite(t.grad).all()) for t in (a, b, x))
    calls = dict(CT.STATS)
    assert CT.try_cat2(a.detach(), b.detach(), UP2) is None and CT.try_spp(x.detach()) is None  # fp32 outside autocast
    assert dict(CT.STATS) == calls


def test_declined_operands_take_the_eager_path():
    """Non-contiguous inputs, an odd map under UP2 and a plane over the SPP limit: flagged modules compute the eager expression, with
    STATS unchanged."""
    import torch
    import torch.nn.functional as F
    from ssds.modeling.layers import cattrain as CT
    from ssds.modeling.ssds import yolo

    torch.manual_seed(1)
    cl = [torch.randn(2, 8, s, s, device="cuda").bfloat16().to(memory_format=torch.channels_last) for s in (8, 4)]
    assert not cl[0].is_contiguous()
    odd = [torch.randn(2, 8, 6, 5, device="cuda").bfloat16(), torch.randn(2, 8, 3, 2, device="cuda").bfloat16()]
    big = torch.randn(1, 2, CT.MAX_SIDE + 1, 8, device="cuda").bfloat16()
    m = CT.use_native_cat(torch.nn.Sequential(yolo.SPPModule(3)))[0]
    before = dict(CT.STATS)
    assert CT.try_cat2(cl[0], cl[1], UP2) is None and CT.try_cat2(cl[0], cl[0], SAME) is None
    assert CT.try_cat2(odd[0], odd[1], UP2) is None and CT.try_spp(cl[0]) is None and CT.try_spp(big) is None
    assert torch.equal(yolo._cat(True, cl[0], cl[1], True), torch.cat((cl[0], F.interpolate(cl[1], scale_factor=2)), 1))
    assert torch.equal(yolo._cat(True, cl[0], cl[0], False), torch.cat((cl[0], cl[0]), 1))
    assert m.native_cat and torch.equal(m(cl[0]), _spp_eager(cl[0])) and torch.equal(m(big), _spp_eager(big))
    with pytest.raises(ValueError):
        CT.cat2(odd[0], odd[1], UP2)
    with pytest.raises(ValueError):
        CT.spp(big)
    with pytest.raises(ValueError):
        CT.spp(cl[0])
    assert dict(CT.STATS) == before


# ---- whole necks in train mode ------------------------------------------------------------------------------------------------------
def _rel(a, b):
    return float((a.double().cpu() - b.double()).norm() / b.double().norm().clamp(min=1e-12))


def _yolo(kind):
    import torch.nn as nn
    from ssds.modeling.ssds.yolo import YOLOV3, YOLOV4

    class Stub(nn.Module):
        """Three maps of 32 / 48 / 64 channels at 32 / 16 / 8 pixels of a 64 x 64 image."""

        def __init__(self):
            super(Stub, self).__init__()
            self.c = nn.ModuleList([nn.Conv2d(3, ch, 1, stride=s) for ch, s in ((32, 2), (48, 4), (64, 8))])

        def initialize(self):
            return None

        def forward(self, x):
            return [c(x) for c in self.c]

    cls = YOLOV3 if kind == "yolov3" else YOLOV4
    _, extras, head = cls.add_extras([[0, 1, 2], [32, 48, 64]], [2, 2, 2], 3)
    return cls(Stub(), extras, head, 3)


def _neck_run(module, image, native, device):
    """One train-mode forward + backward -> {name: tensor} of outputs, the input gradient and every parameter gradient."""
    import torch
    from ssds.modeling.layers import cattrain as CT

    m = copy.deepcopy(module).to(device).train()
    if native:
        CT.use_native_cat(m)
    x = image.to(device).to(torch.float32 if device == "cuda" else torch.float64).requires_grad_(True)
    ctx = torch.autocast("cuda", dtype=torch.bfloat16) if device == "cuda" else torch.autocast("cpu", enabled=False)
    with ctx:
        loc, conf = m(x)
    outs = list(loc) + list(conf)
    sum(o.float().pow(2).mean() if device == "cuda" else o.pow(2).mean() for o in outs).backward()
    if device == "cuda":
        torch.cuda.synchronize()
    res = {"output%d" % i: o.detach() for i, o in enumerate(outs)}
    res["input.grad"] = x.grad
    res.update({k + ".grad": p.grad for k, p in m.named_parameters()})
    return res


@pytest.mark.parametrize("kind", ["yolov3", "yolov4"])
def test_whole_neck_in_train_mode(kind):
    """YOLOV3 (two concatenations) and YOLOV4 (SPP + one PANModule: four concatenations) on a three-map stub backbone, N = 2, train
    mode, bf16 autocast, with use_native_cat, against the fp64 CPU model: per tensor (outputs, input gradient, every parameter gradient)
    rel(native) <= 2 rel(floor) + 0.02, the floor being the same bf16-autocast module with the flag off (the rule of
    tests/test_gpu_necktrain.py::test_whole_neck_in_train_mode)."""
    import torch
    from ssds.modeling.layers import cattrain as CT

    torch.manual_seed(6)
    module = _yolo(kind)
    image = torch.randn(2, 3, 64, 64)
    want = _neck_run(module.double(), image, False, "cpu")
    module = module.float()
    calls = dict(CT.STATS)
    got = _neck_run(module, image, True, "cuda")
    n_cat, n_spp = (2, 0) if kind == "yolov3" else (4, 1)
    delta = {k: CT.STATS[k] - calls[k] for k in calls if k.endswith("ward")}
    assert delta == dict(cat_forward=n_cat, cat_backward=n_cat, spp_forward=n_spp, spp_backward=n_spp), "the native path did not run"
    calls = dict(CT.STATS)
    floor = _neck_run(module, image, False, "cuda")
    assert dict(CT.STATS) == calls
    assert set(got) == set(want) == set(floor)
    bad = []
    for k in sorted(want):
        rn, rf = _rel(got[k], want[k]), _rel(floor[k], want[k])
        print("%s %-44s rel native %.5f floor %.5f" % (kind, k, rn, rf))
        if not rn <= 2.0 * rf + 0.02:
            bad.append((k, rn, rf))
    assert not bad, bad


_SWITCH = r"""
import sys, math, torch
sys.path[:0] = [%(root)r, %(pkg)r]
from ssds.core import config
from ssds.utils import train_ddp
from ssds.modeling.layers import cattrain as CT
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
print("RESULT", CT.STATS["yolov3_models"], CT.STATS["pan_modules"], CT.STATS["spp_modules"], CT.STATS["cat_forward"], CT.STATS["cat_backward"],
      CT.STATS["spp_forward"], CT.STATS["spp_backward"], int(finite), len(grads))
"""


@pytest.mark.parametrize("cfg_name", ["yolov3_resnet18_320.yml", "yolov4_resnet18_512.yml"])
@pytest.mark.parametrize("switch", ["0", "1"])
def test_the_switch(cfg_name, switch):
    """The Solver-built model of each shipped YOLO config takes one training step (forward, backward, optimizer) at batch 2 and image
    size 128, in a subprocess: with SSDK_CAT_TRAIN=1 the kernels run (cat counts, and SPP counts for YOLOv4, non-zero; as many
    backward as forward calls) and the loss and gradients are finite; with 0 every count is zero."""
    env = dict(os.environ, SSDK_CAT_TRAIN=switch)
    code = _SWITCH % dict(root=ROOT, pkg=os.path.join(ROOT, "ssds.pytorch_amd"), cfg=os.path.join(ROOT, "experiments", "cfgs", cfg_name))
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    res = [int(v) for v in [l for l in out.stdout.splitlines() if l.startswith("RESULT")][-1].split()[1:]]
    n3, npan, nspp, cf, cb, sf, sb, finite, ngrads = res
    assert finite == 1 and ngrads > 0
    if switch == "0":
        assert res[:7] == [0] * 7
    elif cfg_name.startswith("yolov3"):
        assert (n3, npan, nspp) == (1, 0, 0) and cf == cb == 2 and (sf, sb) == (0, 0)
    else:
        assert (n3, npan, nspp) == (0, 1, 1) and cf == cb == 4 and (sf, sb) == (1, 1)
