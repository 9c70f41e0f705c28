"""The neck operations of the TRAINING step on the GPU (csrc/ssdk_necktrain.hip behind ssds/modeling/layers/neckfuse.py): the weighted
fusions / upsample-add and the stem max-pool, forward and backward, per element against the eager torch expression under autograd in
fp64 on the CPU on the same 16-bit-rounded operands and the same fp32 weights; exact weight gradients of one-hot and all-ones
gradients; bit-reproducibility; NaN; hipGraph capture; the autocast contract; non-contiguous inputs; whole necks in train mode
against the PyTorch-ROCm floor; and the switch.

Inputs are relu(randn) rounded to the dtype: about half the elements are exact zeros, so pooling-window ties are everywhere (torch's
fp64 CPU backward of max_pool2d gives the first maximum in row-major window order, the kernels' rule).  Bars: y and the tensor
gradients per element within eps |want| + 4 eps rms(want) (eps = 2^-8 bf16, 2^-10 fp16: one rounding, the bar of
tests/test_gpu_dense3_train.py); gw[k] within WSUM_DEPTH 2^-24 sum |gy R_k(x_k)| -- the products are exact in fp32 and no summation
order of that depth can do worse."""
import copy
import functools
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAME, UP2, POOL2 = 0, 1, 2
FORMS = ("up_null", "up_w", "pool_w", "pool_same_w")

# output shape [N, C, H, W] -> the source sizes a POOL2 source is pooled from (None: 2H x 2W)
SHAPES = [
    ((2, 8, 6, 10), [None]),
    ((1, 4, 3, 4), [(7, 9)]),
    ((1, 3, 1, 1), [(2, 2), (3, 3)]),
    ((2, 5, 2, 34), [None]),
    ((2, 5, 4, 66), [None]),
    ((2, 256, 40, 40), [None]),
    ((1, 256, 112, 112), [None]),
    ((3, 7, 14, 14), [(28, 28), (29, 29)]),
]


def _cases():
    out = []
    for shape, pooled in SHAPES:
        if shape[2] % 2 == 0 and shape[3] % 2 == 0:
            out += [(shape, "up_null", None), (shape, "up_w", None)]
        for src in pooled:
            src = (2 * shape[2], 2 * shape[3]) if src is None else src
            out += [(shape, "pool_w", src), (shape, "pool_same_w", src)]
    return out


CASES = _cases()
_ids = ["%s-%s-%s" % ("x".join(map(str, s)), f, "x".join(map(str, p)) if p else "up") for s, f, p in CASES]


def _dtype(name):
    import torch

    return (torch.bfloat16, 2.0 ** -8) if name == "bf16" else (torch.float16, 2.0 ** -10)


def _modes(form):
    return (UP2 if form.startswith("up") else POOL2), SAME


def _R(x, mode):
    import torch.nn.functional as F

    if mode == UP2:
        return F.interpolate(x, scale_factor=2, mode="nearest")
    if mode == POOL2:
        return F.max_pool2d(x, kernel_size=2)
    return x


@functools.lru_cache(maxsize=4)
def _operands(shape, form, src, dtype_name):
    """a, b, c | None, weights [K, 3] fp32 | None (column 1 is used), gy: relu(randn) sources and gy ~ N(0, 1), rounded."""
    import torch

    dtype, _ = _dtype(dtype_name)
    n, c, h, w = shape
    g = torch.Generator().manual_seed(1000 * h + 10 * w + c + len(form) + (src[0] if src else 0))
    a = torch.relu(torch.randn(n, c, h, w, generator=g)).to(dtype)
    bshape = (n, c, h // 2, w // 2) if form.startswith("up") else (n, c) + tuple(src)
    b = torch.relu(torch.randn(bshape, generator=g)).to(dtype)
    cc = torch.relu(torch.randn(n, c, h, w, generator=g)).to(dtype) if form == "pool_same_w" else None
    wt = None
    if form != "up_null":
        k = 3 if cc is not None else 2
        wt = torch.rand(k, 3, generator=g) + 0.1
        wt = wt / (wt.sum(0) + 1e-6)
    gy = torch.randn(n, c, h, w, generator=g).to(dtype)
    return a, b, cc, wt, gy


def _truth_from(a, b, cc, wt, gy, form):
    """The eager expression under autograd in fp64 on the CPU -> y, ga, gb, gc, gw [K], sum |gy R_k(x_k)| [K]."""
    import torch

    mode_b, mode_c = _modes(form)
    a64, b64 = a.double().requires_grad_(True), b.double().requires_grad_(True)
    c64 = None if cc is None else cc.double().requires_grad_(True)
    w64 = None if wt is None else wt[:, 1].double().requires_grad_(True)
    terms = [a64, _R(b64, mode_b)] + ([] if c64 is None else [_R(c64, mode_c)])
    y = sum(t if w64 is None else w64[k] * t for k, t in enumerate(terms))
    y.backward(gy.double())
    mass = [float((gy.double() * t.detach()).abs().sum()) for t in terms]
    return (y.detach(), a64.grad, b64.grad, None if c64 is None else c64.grad, None if w64 is None else w64.grad, mass)


@functools.lru_cache(maxsize=4)
def _truth(shape, form, src, dtype_name):
    return _truth_from(*_operands(shape, form, src, dtype_name), form)


def _native_from(a, b, cc, wt, gy, form):
    import torch
    from ssds.modeling.layers import neckfuse as NF

    mode_b, mode_c = _modes(form)
    ad, bd = a.cuda().requires_grad_(True), b.cuda().requires_grad_(True)
    cd = None if cc is None else cc.cuda().requires_grad_(True)
    wd = None if wt is None else wt.cuda().requires_grad_(True)
    y = NF.neck_fuse(ad, bd, cd, wd, 1, mode_b, mode_c)
    y.backward(gy.cuda())
    torch.cuda.synchronize()
    return y.detach(), ad.grad, bd.grad, None if cd is None else cd.grad, None if wd is None else wd.grad


def _rounding_bar(got, want, eps, what):
    """A result rounded once: |got - want| <= eps |want| + 4 eps rms(want) per element."""
    err = (got.double().cpu() - want).abs()
    bar = eps * want.abs() + 4 * eps * float(want.pow(2).mean().sqrt())
    worst = float((err / bar.clamp(min=1e-300)).max())
    print("%s: worst |err| / bar = %.3f" % (what, worst))
    assert bool((err <= bar).all()), "%s: %d elements outside the rounding bar, worst %.3g of it" % (what, int((err > bar).sum()), worst)


@pytest.mark.parametrize("shape,form,src", CASES, ids=_ids)
@pytest.mark.parametrize("dtype_name", ["bf16", "f16"])
def test_single_fusion(shape, form, src, dtype_name):
    import torch
    from ssds import _native as N
    from ssds.modeling.layers import neckfuse as NF

    assert NF.WSUM_DEPTH <= 512
    dtype, eps = _dtype(dtype_name)
    ops = _operands(shape, form, src, dtype_name)
    y64, ga64, gb64, gc64, gw64, mass = _truth(shape, form, src, dtype_name)
    y, ga, gb, gc, gw = _native_from(*ops, form)
    assert "neck_fuse" in N.last_kernel(), N.last_kernel()
    tag = "%s %s %s %s" % (shape, form, src, dtype_name)
    for t, ref in ((y, ops[0]), (ga, ops[0]), (gb, ops[1])):
        assert t.dtype == dtype and t.is_contiguous() and tuple(t.shape) == tuple(ref.shape)
    _rounding_bar(y, y64, eps, "y " + tag)
    _rounding_bar(ga, ga64, eps, "ga " + tag)
    _rounding_bar(gb, gb64, eps, "gb " + tag)
    if form.startswith("pool"):  # the gradient lands on the arg-max of every window and nowhere else
        # (a value below the dtype's smallest subnormal rounds to zero under one rounding: fp16 only, and not a position error)
        differ = ((gb.cpu() != 0) != (gb64 != 0)) & ~((gb64 != 0) & (gb64.abs() < torch.finfo(dtype).smallest_normal * 2.0 ** -10))
        assert not bool(differ.any()), "gb %s: %d positions differ" % (tag, int(differ.sum()))
    if gc64 is not None:
        _rounding_bar(gc, gc64, eps, "gc " + tag)
    if gw64 is None:
        assert gw is None
        return
    assert gw.dtype == torch.float32 and tuple(gw.shape) == tuple(ops[3].shape)
    assert bool((gw[:, 0] == 0).all()) and bool((gw[:, 2] == 0).all()), "zeros outside the addressed column"
    for k in range(gw.shape[0]):
        err, bar = abs(float(gw[k, 1].double()) - float(gw64[k])), NF.WSUM_DEPTH * 2.0 ** -24 * mass[k]
        print("gw[%d] %s: |err| / bar = %.4f (want %.6g)" % (k, tag, err / max(bar, 1e-300), float(gw64[k])))
        assert err <= bar, "gw[%d] %s: err %.3g, bar %.3g" % (k, tag, err, bar)


def _positions(shape):
    n, c, h, w = shape
    pos = [(0, 0, 0, 0), (n - 1, c - 1, h - 1, w - 1), (0, 0, h - 1, 0), (0, c - 1, 0, w - 1), (n - 1, 0, h - 1, w // 2),
           (n - 1, c // 2, h // 2, w - 1), (0, c // 2, h // 2, w // 2), (n - 1, c - 1, max(h - 2, 0), max(w - 2, 0))]
    return sorted(set(pos))


@pytest.mark.parametrize("shape,form,src", [c for c in CASES if c[1] in ("up_w", "pool_same_w")],
                         ids=[i for i, c in zip(_ids, CASES) if c[1] in ("up_w", "pool_same_w")])
@pytest.mark.parametrize("dtype_name", ["bf16", "f16"])
def test_weight_gradient_of_a_one_hot_gradient_is_exact(shape, form, src, dtype_name):
    """gy one-hot: gw[k] == float32(gy R_k(x_k)) exactly -- one dropped or doubled element anywhere would show."""
    import torch
    from ssds.modeling.layers import neckfuse as NF

    dtype, _ = _dtype(dtype_name)
    a, b, cc, wt, _ = _operands(shape, form, src, dtype_name)
    mode_b, mode_c = _modes(form)
    terms = [a.double(), _R(b.double(), mode_b)] + ([] if cc is None else [_R(cc.double(), mode_c)])
    ad, bd, wd = a.cuda(), b.cuda(), wt.cuda().requires_grad_(True)
    cd = None if cc is None else cc.cuda()
    y = NF.neck_fuse(ad, bd, cd, wd, 1, mode_b, mode_c)
    gy = torch.zeros(shape, dtype=dtype, device="cuda")
    value = torch.tensor(-1.3125, dtype=dtype)
    for pos in _positions(shape):
        gy.zero_()
        gy[pos] = value
        (gw,) = torch.autograd.grad(y, (wd,), gy, retain_graph=True)
        want = torch.stack([float(value) * t[pos] for t in terms])
        assert torch.equal(gw[:, 1].double().cpu(), want), (pos, gw[:, 1].tolist(), want.tolist())
        assert bool((gw[:, 0] == 0).all()) and bool((gw[:, 2] == 0).all())


@pytest.mark.parametrize("form,src", [("up_w", None), ("pool_same_w", (80, 80)), ("pool_same_w", (81, 81))])
def test_weight_gradient_of_ones_counts_every_element(form, src):
    """gy == 1 and sources == 1 at [2, 256, 40, 40]: gw[k] == N C H W exactly (integers below 2^24 add exactly in fp32)."""
    import torch
    from ssds.modeling.layers import neckfuse as NF

    shape = (2, 256, 40, 40)
    mode_b, mode_c = _modes(form)
    a = torch.ones(shape, dtype=torch.bfloat16, device="cuda")
    b = torch.ones((2, 256, 20, 20) if src is None else (2, 256) + src, dtype=torch.bfloat16, device="cuda")
    cc = torch.ones_like(a) if form == "pool_same_w" else None
    wt = torch.full((2 if cc is None else 3, 3), 0.25, device="cuda", requires_grad=True)
    y = NF.neck_fuse(a, b, cc, wt, 1, mode_b, mode_c)
    (gw,) = torch.autograd.grad(y, (wt,), torch.ones_like(a))
    assert gw[:, 1].tolist() == [float(2 * 256 * 40 * 40)] * gw.shape[0], gw.tolist()


# ---- the stem max-pool ------------------------------------------------------------------------------------------------------------
POOL_SHAPES = [(2, 4, 7, 9), (1, 3, 1, 1), (1, 3, 2, 2), (2, 5, 8, 34), (2, 64, 40, 40), (1, 64, 160, 160)]


def _pool_truth(x, gy):
    import torch.nn.functional as F

    x64 = x.double().requires_grad_(True)
    y = F.max_pool2d(x64, 3, 2, 1)
    y.backward(gy.double())
    return y.detach(), x64.grad


def _pool_native(x, gy):
    import torch
    from ssds.modeling.layers import neckfuse as NF

    xd = x.cuda().requires_grad_(True)
    y = NF.maxpool3x3s2(xd)
    y.backward(gy.cuda())
    torch.cuda.synchronize()
    return y.detach(), xd.grad


@pytest.mark.parametrize("shape", POOL_SHAPES, ids=["x".join(map(str, s)) for s in POOL_SHAPES])
@pytest.mark.parametrize("dtype_name", ["bf16", "f16"])
def test_maxpool_forward_and_backward(shape, dtype_name):
    import torch
    import torch.nn.functional as F
    from ssds import _native as N

    dtype, eps = _dtype(dtype_name)
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.relu(torch.randn(shape, generator=g)).to(dtype)
    n, c, h, w = shape
    gy = torch.randn(n, c, (h - 1) // 2 + 1, (w - 1) // 2 + 1, generator=g).to(dtype)
    y64, gx64 = _pool_truth(x, gy)
    y, gx = _pool_native(x, gy)
    assert "maxpool_train" in N.last_kernel(), N.last_kernel()
    assert y.dtype == dtype and gx.dtype == dtype and tuple(gx.shape) == shape and tuple(y.shape) == tuple(gy.shape)
    assert torch.equal(y, F.max_pool2d(x.cuda(), 3, 2, 1)), "forward is not bit-equal to F.max_pool2d"
    assert torch.equal(y.double().cpu(), y64)
    _rounding_bar(gx, gx64, eps, "gx %s %s" % (shape, dtype_name))
    assert torch.equal(gx.cpu() != 0, gx64 != 0)


@pytest.mark.parametrize("value", [0.0, 1.5, float("-inf")])
def test_maxpool_of_a_constant_plane_sends_the_gradient_to_the_first_window_positions(value):
    import torch

    shape = (2, 3, 9, 12)
    x = torch.full(shape, value).to(torch.bfloat16)
    gy = torch.randn(2, 3, 5, 6, generator=torch.Generator().manual_seed(4)).to(torch.bfloat16)
    y64, gx64 = _pool_truth(x, gy)
    y, gx = _pool_native(x, gy)
    assert torch.equal(y.double().cpu(), y64)
    _rounding_bar(gx, gx64, 2.0 ** -8, "gx constant %s" % value)
    assert torch.equal(gx.cpu() != 0, gx64 != 0)
    # first in-range element of every window: row / column 0, then the odd ones
    assert bool((gx[:, :, 2::2, :] == 0).all()) and bool((gx[:, :, :, 2::2] == 0).all())


def test_bit_reproducibility():
    import torch

    shape, form, src = (2, 256, 40, 40), "pool_same_w", (80, 80)
    ops = _operands(shape, form, src, "bf16")
    r1, r2 = _native_from(*ops, form), _native_from(*ops, form)
    for u, v, what in zip(r1, r2, ("y", "ga", "gb", "gc", "gw")):
        assert torch.equal(u, v), what
    g = torch.Generator().manual_seed(9)
    x = torch.relu(torch.randn(2, 64, 40, 40, generator=g)).to(torch.bfloat16)
    gy = torch.randn(2, 64, 20, 20, generator=g).to(torch.bfloat16)
    p1, p2 = _pool_native(x, gy), _pool_native(x, gy)
    assert torch.equal(p1[0], p2[0]) and torch.equal(p1[1], p2[1])


def test_nan_goes_where_torch_puts_it():
    import torch
    import torch.nn.functional as F
    from ssds.modeling.layers import neckfuse as NF

    shape, form, src = (2, 8, 6, 10), "pool_w", (12, 20)
    a, b, _, wt, _ = _operands(shape, form, src, "bf16")
    clean = NF.neck_fuse(a.cuda(), b.cuda(), None, wt.cuda(), 1, POOL2)
    b = b.clone()
    b[1, 3, 7, 9] = float("nan")  # window (3, 4), its last element
    y = NF.neck_fuse(a.cuda(), b.cuda(), None, wt.cuda(), 1, POOL2)
    want = wt[0, 1] * a.float() + wt[1, 1] * F.max_pool2d(b.float(), 2)
    assert torch.equal(torch.isnan(y).cpu(), torch.isnan(want)) and int(torch.isnan(want).sum()) == 1 and bool(torch.isnan(want[1, 3, 3, 4]))
    keep = ~torch.isnan(want)
    assert torch.equal(y.cpu()[keep], clean.cpu()[keep])
    x = torch.relu(torch.randn(2, 4, 7, 9, generator=torch.Generator().manual_seed(2))).to(torch.bfloat16)
    clean = NF.maxpool3x3s2(x.cuda())
    x[1, 2, 3, 4] = float("nan")
    y = NF.maxpool3x3s2(x.cuda())
    want = F.max_pool2d(x.cuda(), 3, 2, 1)
    assert torch.equal(torch.isnan(y), torch.isnan(want)) and int(torch.isnan(want).sum()) >= 1
    keep = ~torch.isnan(want)
    assert torch.equal(y[keep], clean[keep]) and torch.equal(y[keep], want[keep])


def test_forward_and_backward_capture_into_a_graph():
    """Forward + backward of a three-source fusion and of the pool, captured once after a warm-up and replayed twice with new input
    values in the same buffers: each replay equals the eager native call bit for bit (single stream; the queue count is the
    machine's default)."""
    import torch
    from ssds.modeling.layers import neckfuse as NF

    shape, form, src = (2, 8, 6, 10), "pool_same_w", (13, 21)
    sets = []
    for seed in (1, 2):
        g = torch.Generator().manual_seed(seed)
        fuse = [torch.relu(torch.randn(s, generator=g)).bfloat16() for s in (shape, (2, 8) + src, shape)]
        wt = torch.rand(3, 3, generator=g) + 0.1
        gy = torch.randn(shape, generator=g).bfloat16()
        x = torch.relu(torch.randn(2, 4, 7, 9, generator=g)).bfloat16()
        gp = torch.randn(2, 4, 4, 5, generator=g).bfloat16()
        sets.append((fuse[0], fuse[1], fuse[2], wt, gy, x, gp))
    eager = [(_native_from(*s[:5], form), _pool_native(s[5], s[6])) for s in sets]
    bufs = [t.cuda() for t in sets[0]]
    for t in bufs[:4] + bufs[5:6]:
        t.requires_grad_(True)
    a, b, cc, wt, gy, x, gp = bufs

    def step():
        y = NF.neck_fuse(a, b, cc, wt, 1, POOL2, SAME)
        grads = torch.autograd.grad(y, (a, b, cc, wt), gy)
        py = NF.maxpool3x3s2(x)
        (gx,) = torch.autograd.grad(py, (x,), gp)
        return (y,) + tuple(grads), (py, gx)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up on a side stream, as torch.cuda.graph asks
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fused, pooled = step()
    for i in (1, 0):
        with torch.no_grad():
            for dst, new in zip(bufs, sets[i]):
                dst.copy_(new)
        for t in fused + pooled:
            t.detach().zero_()
        graph.replay()
        torch.cuda.synchronize()
        for got, want, what in zip(fused, eager[i][0], ("y", "ga", "gb", "gc", "gw")):
            assert torch.equal(got.detach(), want), (i, what)
        assert torch.equal(pooled[0].detach(), eager[i][1][0]) and torch.equal(pooled[1], eager[i][1][1]), i


def _bifpn(levels=4, channels=256):
    import torch
    from ssds.modeling.ssds.bifpn import BiFPNModule

    m = BiFPNModule(channels, levels)
    with torch.no_grad():
        m.w1.copy_(torch.rand_like(m.w1) + 0.1)
        m.w2.copy_(torch.rand_like(m.w2) + 0.1)
    return m


def test_autocast_contract():
    import torch
    from ssds import _native as N
    from ssds.modeling.layers import neckfuse as NF

    torch.manual_seed(0)
    m = _bifpn(3, 16).cuda().train()
    NF.use_native_neck(m)
    assert m.native_neck and m.w1.dtype == torch.float32
    xs = [torch.randn(2, 16, s, s, device="cuda", requires_grad=True) for s in (16, 8, 4)]
    calls = dict(NF.STATS)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out = m(list(xs))
    assert NF.STATS["fuse_forward"] - calls["fuse_forward"] == 4  # two top-down, one bottom-up with skip, the last bottom-up
    assert all(o.dtype == torch.bfloat16 for o in out) and "neck_fuse" in N.last_kernel()
    sum(o.float().pow(2).mean() for o in out).backward()
    assert NF.STATS["fuse_backward"] - calls["fuse_backward"] == 4
    assert m.w1.grad.dtype == torch.float32 and m.w1.grad.shape == m.w1.shape and bool(torch.isfinite(m.w1.grad).all())
    assert m.w2.grad.dtype == torch.float32 and m.w2.grad.shape == m.w2.shape and bool((m.w2.grad != 0).any())
    assert all(x.grad is not None and x.grad.dtype == torch.float32 for x in xs)
    # fp32 tensors outside autocast: the eager expressions
    calls = dict(NF.STATS)
    m([x.detach() for x in xs])
    assert dict(NF.STATS) == calls


def test_non_contiguous_input_takes_the_eager_path():
    import torch
    from ssds.modeling.layers import neckfuse as NF

    torch.manual_seed(1)
    m = _bifpn(3, 16).cuda().to(torch.bfloat16).eval()
    ref = copy.deepcopy(m)
    NF.use_native_neck(m)
    xs = [torch.randn(2, 16, s, s, device="cuda").to(torch.bfloat16).to(memory_format=torch.channels_last) for s in (16, 8, 4)]
    assert not xs[0].is_contiguous()
    before = dict(NF.STATS)
    with torch.no_grad():  # (every fusion of a 3-level layer reads at least one of the inputs)
        got, want = m(list(xs)), ref(list(xs))
    assert all(torch.equal(u, v) for u, v in zip(got, want))
    assert NF.try_fuse(xs[0], xs[1], mode_b=UP2) is None
    y = NF.TrainMaxPool3x3s2(3, 2, 1)(xs[0])
    assert torch.equal(y, torch.nn.functional.max_pool2d(xs[0], 3, 2, 1))
    assert dict(NF.STATS) == before


# ---- whole necks in train mode ------------------------------------------------------------------------------------------------------
def _rel(a, b):
    return float((a.double().cpu() - b.double()).norm() / b.double().norm().clamp(min=1e-12))


class _TopDown(object):
    @staticmethod
    def build():
        import torch.nn as nn
        from ssds.modeling.ssds.fpn import SSDFPN

        class Stub(nn.Module):
            """Three maps of 32 / 48 / 64 channels at 32 / 16 / 8 pixels."""

            def __init__(self):
                super(Stub, self).__init__()
                self.c = nn.ModuleList([nn.Conv2d(3, ch, 1, stride=s) for ch, s in ((32, 2), (48, 4), (64, 8))])

            def initialize(self):
                return None

            def forward(self, x):
                return [c(x) for c in self.c]

        _, extras, head = SSDFPN.add_extras([[0, 1, 2], [32, 48, 64]], [2, 2, 2], 3)
        return SSDFPN(Stub(), extras, head, 3)


def _neck_run(kind, module, inputs, native, device, dtype):
    """One train-mode forward + backward -> {name: tensor} of outputs, input gradients and every parameter gradient."""
    import torch
    from ssds.modeling.layers import neckfuse as NF

    m = copy.deepcopy(module).to(device).train()
    if native:
        NF.use_native_neck(m)
    xs = [x.to(device).to(dtype).requires_grad_(True) for x in inputs]
    ctx = torch.autocast("cuda", dtype=torch.bfloat16) if device == "cuda" else torch.autocast("cpu", enabled=False)
    with ctx:
        if kind == "bifpn":
            outs = list(m(list(xs)))
        else:
            loc, conf = m(xs[0])
            outs = list(loc) + list(conf)
    sum(o.float().pow(2).mean() if device == "cuda" else o.pow(2).mean() for o in outs).backward()
    if device == "cuda":
        torch.cuda.synchronize()
    res = {"output%d" % i: o.detach() for i, o in enumerate(outs)}
    res.update({"input%d.grad" % i: x.grad for i, x in enumerate(xs)})
    res.update({k + ".grad": p.grad for k, p in m.named_parameters()})
    return res


@pytest.mark.parametrize("kind", ["bifpn", "fpn"])
def test_whole_neck_in_train_mode(kind):
    """Two stacked 4-level BiFPNModule layers (C = 256, 32^2 .. 4^2, N = 2) and the top-down path of an SSDFPN on a stub backbone, train
    mode, bf16 autocast, with use_native_neck, against the fp64 CPU model: per tensor (outputs, input gradients, every parameter
    gradient, w1 / w2 included) rel(native) <= 2 rel(floor) + 0.02, the floor being the same bf16-autocast module with the flag off
    (the rule of tests/test_gpu_dense3_train.py::test_one_block_in_train_mode)."""
    import torch
    import torch.nn as nn
    from ssds.modeling.layers import neckfuse as NF

    torch.manual_seed(6)
    if kind == "bifpn":
        module = nn.Sequential(_bifpn(4, 256), _bifpn(4, 256))
        # every level twice the next (the top-down path); rounded to bf16 and handed over in bf16, as the 1x1 lateral convolutions in
        # front of the layer do under autocast: native, floor and truth read the same operands
        inputs = [torch.relu(torch.randn(2, 256, s, s)).bfloat16().float() for s in (32, 16, 8, 4)]
    else:
        module = _TopDown.build()
        inputs = [torch.randn(2, 3, 64, 64)]
    want = _neck_run(kind, module.double(), inputs, False, "cpu", torch.float64)
    module = module.float()
    calls = dict(NF.STATS)
    gpu_dtype = torch.bfloat16 if kind == "bifpn" else torch.float32  # (the FPN model takes the image: its stub backbone runs under autocast)
    got = _neck_run(kind, module, inputs, True, "cuda", gpu_dtype)
    n_fuse = 2 * 6 if kind == "bifpn" else 2
    assert NF.STATS["fuse_forward"] - calls["fuse_forward"] == n_fuse and NF.STATS["fuse_backward"] - calls["fuse_backward"] == n_fuse, \
        "the native path did not run"
    calls = dict(NF.STATS)
    floor = _neck_run(kind, module, inputs, False, "cuda", gpu_dtype)
    assert dict(NF.STATS) == calls
    assert set(got) == set(want) == set(floor)
    bad = []
    for k in sorted(want):
        rn, rf = _rel(got[k], want[k]), _rel(floor[k], want[k])
        print("%s %-40s rel native %.5f floor %.5f" % (kind, k, rn, rf))
        if not rn <= 2.0 * rf + 0.02:
            bad.append((k, rn, rf))
    assert not bad, bad


_SWITCH = r"""
import sys, math, torch
sys.path[:0] = [%(root)r, %(pkg)r]
from ssds.core import config
from ssds.utils import train_ddp
from ssds.modeling.layers import neckfuse as NF
cfg = config.cfg_from_file(%(cfg)r)
s = train_ddp.Solver(cfg, 0, torch.device("cuda", 0))
net = s.model
net.train()
x = torch.randn(2, 3, %(size)d, %(size)d, device="cuda")
with torch.autocast("cuda", dtype=torch.bfloat16):
    loc, conf = net(x)
loss = sum(o.float().pow(2).mean() for o in tuple(loc) + tuple(conf))
s.optimizer.zero_grad()
loss.backward()
s.optimizer.step()
torch.cuda.synchronize()
grads = [p.grad for p in net.parameters() if p.grad is not None]
finite = math.isfinite(float(loss)) and all(bool(torch.isfinite(g).all()) for g in grads)
print("RESULT", NF.STATS["bifpn_modules"], NF.STATS["fpn_models"], NF.STATS["maxpools"], NF.STATS["fuse_forward"], NF.STATS["fuse_backward"],
      NF.STATS["pool_forward"], NF.STATS["pool_backward"], int(finite), len(grads))
"""


@pytest.mark.parametrize("cfg_name,size", [("bifpn_regnetx008_896.yml", 256), ("fpn_resnet50_640.yml", 128)])
@pytest.mark.parametrize("switch", ["0", "1"])
def test_the_switch(cfg_name, size, switch):
    """The Solver-built model takes one training step (forward, backward, optimizer) at batch 2 and a reduced image size, in a
    subprocess: with SSDK_NECK_TRAIN=1 the neck kernels run (non-zero counts) and the loss and gradients are finite; with 0 every count
    is zero."""
    env = dict(os.environ, SSDK_NECK_TRAIN=switch)
    code = _SWITCH % dict(root=ROOT, pkg=os.path.join(ROOT, "ssds.pytorch_amd"), cfg=os.path.join(ROOT, "experiments", "cfgs", cfg_name),
                          size=size)
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    res = [int(v) for v in [l for l in out.stdout.splitlines() if l.startswith("RESULT")][-1].split()[1:]]
    n_bifpn, n_fpn, n_pool, ff, fb, pf, pb, finite, ngrads = res
    assert finite == 1 and ngrads > 0
    if switch == "0":
        assert res[:7] == [0] * 7
    elif cfg_name.startswith("bifpn"):
        assert n_bifpn >= 1 and (n_fpn, n_pool, pf, pb) == (0, 0, 0, 0) and ff > 0 and fb == ff
    else:
        assert (n_bifpn, n_fpn, n_pool) == (0, 1, 1) and ff > 0 and fb == ff and pf == 1
        assert pb <= 1  # (0 when the config's trainable scope freezes the stem in front of the pool)
