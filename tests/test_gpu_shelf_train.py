"""The transposed 3x3 / stride 2 convolution of the Shelf TRAINING step on the GPU (csrc/ssdk_convttrain.hip behind
ssds/modeling/layers/convttrain.py): forward (+ bias + skip map), input gradient, weight and bias gradient of single layers per
element against ``F.conv_transpose2d(x, w, b, 2, 1) + skip`` autograd in fp64 on the CPU on the same 16-bit-rounded operands,
bit-reproducibility, hipGraph capture, the autocast contract, declined operands, a native optimizer step between two calls, the whole
Shelf neck in train mode against the PyTorch-ROCm floor, and the switch.

The bars are those of tests/test_gpu_dense3_train.py: y and gx per element within eps |want| + 4 eps rms(want) (eps = 2^-8 bf16,
2^-10 fp16), gW and gb per element within 2e-5 max|want| + 1e-6.  gb is an fp32 sum of at most 2 * 65 * 65 N(0, 1) terms here: a
plain sequential fp32 sum of the same operands on the CPU stays within 0.012 of that bar at every listed shape (worst at
(2, 256, 128, 33, 33)), so the bar leaves room for any fixed summation order."""
import copy
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# N, Cin, Cout, H, W, bias, skip
CASES = [
    (2, 16, 16, 1, 1, True, True),  # one parity class only
    (2, 16, 16, 1, 5, True, True), (2, 16, 16, 4, 1, True, False),  # a single row / a single column
    (1, 32, 16, 2, 3, False, True),  # a small map without bias
    (2, 48, 80, 5, 4, True, True),  # channel tails, blocks that are no power of two
    (3, 64, 32, 9, 7, True, True),  # odd, unequal sides
    (2, 512, 256, 17, 17, True, True), (2, 256, 128, 33, 33, True, True),  # the layers of shelf_resnet18_513.yml at N = 2
    (1, 2048, 1024, 3, 3, True, True),  # the longest K: a ResNet-50 Shelf
    (1, 16, 16, 40, 3, False, False),  # many rows, no epilogue
]
CONFIG_CASES = [c for c in CASES if c[1] in (512, 256)]


def _dtype(name):
    import torch

    return (torch.bfloat16, 2.0 ** -8) if name == "bf16" else (torch.float16, 2.0 ** -10)


def _operands(n, cin, cout, h, w, bias, skip, dtype, seed=None):
    """x, gy, skip ~ N(0, 1), w ~ N(0, 2 / (9 Cin)), bias ~ N(0, 1); x, gy, skip, w rounded to ``dtype`` (w kept as the fp32 master
    tensor holding rounded values) -- the draw of tests/test_gpu_dense3_train.py::_operands."""
    import torch

    g = torch.Generator().manual_seed(100000 + 1000 * (cin % 997) + 10 * cout + 7 * h + 3 * w + n if seed is None else seed)
    x = torch.randn(n, cin, h, w, generator=g).to(dtype)
    wt = (torch.randn(cin, cout, 3, 3, generator=g) * (2.0 / (9 * cin)) ** 0.5).to(dtype).float()
    gy = torch.randn(n, cout, 2 * h - 1, 2 * w - 1, generator=g).to(dtype)
    sk = torch.randn(n, cout, 2 * h - 1, 2 * w - 1, generator=g).to(dtype) if skip else None
    b = torch.randn(cout, generator=g) if bias else None
    return x, wt, b, sk, gy


def _truth(x, wt, b, sk, gy):
    """F.conv_transpose2d(x, w, b, 2, 1) + skip under autograd in fp64 on the CPU -> y, gx, gW, gb | None, gskip | None."""
    import torch.nn.functional as F

    x64, w64 = x.double().requires_grad_(True), wt.double().requires_grad_(True)
    b64 = None if b is None else b.double().requires_grad_(True)
    s64 = None if sk is None else sk.double().requires_grad_(True)
    y = F.conv_transpose2d(x64, w64, b64, 2, 1)
    if s64 is not None:
        y = y + s64
    y.backward(gy.double())
    return y.detach(), x64.grad, w64.grad, None if b64 is None else b64.grad, None if s64 is None else s64.grad


def _native(x, wt, b, sk, gy):
    import torch
    from ssds.modeling.layers import convttrain as CT

    xd, wd = x.cuda().requires_grad_(True), wt.cuda().requires_grad_(True)
    bd = None if b is None else b.cuda().requires_grad_(True)
    sd = None if sk is None else sk.cuda().requires_grad_(True)
    gyd = gy.cuda()
    y = CT.convt3x3s2(xd, wd, bd, sd)
    y.backward(gyd)
    torch.cuda.synchronize()
    return y.detach(), xd.grad, wd.grad, None if bd is None else bd.grad, None if sd is None else sd.grad, gyd


def _rounding_bar(got, want, eps, what):
    """A result rounded once: |got - want| <= eps |want| + 4 eps rms(want) per element."""
    err = (got.double().cpu() - want).abs()
    bar = eps * want.abs() + 4 * eps * float(want.pow(2).mean().sqrt())
    worst = float((err / bar).max())
    print("%s: worst |err| / bar = %.3f" % (what, worst))
    assert bool((err <= bar).all()), "%s: %d elements outside the rounding bar, worst %.3g of it" % (what, int((err > bar).sum()), worst)


def _wgrad_bar(got, want, what):
    """|got - want| <= 2e-5 max|want| + 1e-6 per element."""
    err = (got.double().cpu() - want).abs()
    bar = 2e-5 * float(want.abs().max()) + 1e-6
    print("%s: worst |err| / bar = %.3f" % (what, float(err.max()) / bar))
    assert float(err.max()) <= bar, "%s: worst %.3g, bar %.3g" % (what, float(err.max()), bar)


@pytest.mark.parametrize("n,cin,cout,h,w,bias,skip", CASES)
@pytest.mark.parametrize("dtype_name", ["bf16", "f16"])
def test_convt_train_single_layer(n, cin, cout, h, w, bias, skip, dtype_name):
    import torch
    from ssds import _native as N

    dtype, eps = _dtype(dtype_name)
    x, wt, b, sk, gy = _operands(n, cin, cout, h, w, bias, skip, dtype)
    y64, gx64, gw64, gb64, gs64 = _truth(x, wt, b, sk, gy)
    y, gx, gw, gb, gs, gyd = _native(x, wt, b, sk, gy)
    assert "convt_train" in N.last_kernel(), N.last_kernel()
    tag = "%d->%d %dx%d n=%d %s" % (cin, cout, h, w, n, dtype_name)
    assert y.dtype == dtype and y.is_contiguous() and tuple(y.shape) == tuple(y64.shape) == (n, cout, 2 * h - 1, 2 * w - 1)
    assert gx.dtype == dtype and gx.is_contiguous() and tuple(gx.shape) == tuple(x.shape)
    assert gw.dtype == torch.float32 and tuple(gw.shape) == (cin, cout, 3, 3)
    _rounding_bar(y, y64, eps, "y " + tag)
    _rounding_bar(gx, gx64, eps, "gx " + tag)
    _wgrad_bar(gw, gw64, "gW " + tag)
    if bias:
        assert gb.dtype == torch.float32 and tuple(gb.shape) == (cout,)
        _wgrad_bar(gb, gb64, "gb " + tag)
    if skip:  # the skip's gradient is the output gradient itself: the same storage, or its bits
        assert gs.data_ptr() == gyd.data_ptr() or torch.equal(gs.view(torch.int16), gyd.view(torch.int16))
        assert torch.equal(gs.double().cpu(), gs64)


@pytest.mark.parametrize("n,cin,cout,h,w,bias,skip", CONFIG_CASES)
def test_forward_and_backward_are_bit_reproducible(n, cin, cout, h, w, bias, skip):
    import torch

    ops = _operands(n, cin, cout, h, w, bias, skip, torch.bfloat16, seed=7)
    r1, r2 = _native(*ops), _native(*ops)
    for u, v, what in zip(r1[:5], r2[:5], ("y", "gx", "gW", "gb", "gskip")):
        assert torch.equal(u, v), what


def test_forward_and_backward_capture_into_a_graph():
    """Capture forward + backward of one layer after a warm-up, replay twice with the operands refreshed in place: bit-equal to the
    plain calls (the queue count is the machine's default)."""
    import torch
    from ssds.modeling.layers import convttrain as CT

    shape = (2, 48, 32, 9, 7, True, True)
    sets = [_operands(*shape, torch.bfloat16, seed=s) for s in (11, 12)]
    eager = [_native(*s)[:5] for s in sets]
    bufs = [t.cuda() for t in sets[0]]
    for t in bufs[:4]:
        t.requires_grad_(True)
    xs, ws, bs, ss, gys = bufs

    def step():
        y = CT.convt3x3s2(xs, ws, bs, ss)
        return (y,) + torch.autograd.grad(y, (xs, ws, bs, ss), gys)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up on a side stream, as torch.cuda.graph asks
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        outs = step()
    for i in (1, 0):
        with torch.no_grad():
            for dst, new in zip(bufs, sets[i]):
                dst.copy_(new)
        for t in outs[:4]:  # (the skip's gradient may BE the gy buffer: not cleared)
            t.detach().zero_()
        g.replay()
        torch.cuda.synchronize()
        for got, want, what in zip(outs, eager[i], ("y", "gx", "gW", "gb", "gskip")):
            assert torch.equal(got.detach(), want), (i, what)


def test_autocast_contract():
    import torch
    import torch.nn as nn
    import torch.nn.functional as F
    from ssds import _native as N
    from ssds.modeling.layers import convttrain as CT

    torch.manual_seed(0)
    for adt in (torch.bfloat16, torch.float16):
        m = CT.use_native_convt(nn.Sequential(nn.ConvTranspose2d(64, 32, 3, stride=2, padding=1)))[0].cuda()
        assert type(m) is CT.ShelfConvT and m.weight.dtype == torch.float32
        x = torch.randn(2, 64, 9, 7, device="cuda", requires_grad=True)
        sk = torch.randn(2, 32, 17, 13, device="cuda", requires_grad=True)
        calls = dict(CT.STATS)
        with torch.autocast("cuda", dtype=adt):
            y = m(x, skip=sk)
        assert y.dtype == adt and "convt_train_fwd" in N.last_kernel()
        ref = F.conv_transpose2d(x.detach().to(adt).float(), m.weight.detach().to(adt).float(), m.bias.detach(), 2, 1) + sk.detach().to(adt).float()
        assert float((y.detach().float() - ref).abs().max()) <= 2.0 ** -7 * float(ref.abs().max())
        y.float().sum().backward()
        assert m.weight.grad.dtype == torch.float32 and m.weight.grad.shape == m.weight.shape
        assert m.bias.grad.dtype == torch.float32 and m.bias.grad.shape == m.bias.shape
        assert x.grad.dtype == torch.float32 and x.grad.shape == x.shape and sk.grad.dtype == torch.float32
        assert float((m.bias.grad - 2 * 17 * 13).abs().max()) == 0 and float((sk.grad - 1).abs().max()) == 0
        assert [CT.STATS[k] - calls[k] for k in ("native_forward", "native_dgrad", "native_wgrad")] == [1, 1, 1]
        # an input that needs no gradient: no input-gradient call; no skip: the module's plain call
        calls = dict(CT.STATS)
        with torch.autocast("cuda", dtype=adt):
            m(x.detach()).float().sum().backward()
        assert [CT.STATS[k] - calls[k] for k in ("native_forward", "native_dgrad", "native_wgrad")] == [1, 0, 1]
    # 16-bit weights are taken too, and give 16-bit parameter gradients
    m16 = CT.ShelfConvT(64, 32, 3, stride=2, padding=1).cuda().to(torch.bfloat16)
    x16 = torch.randn(2, 64, 5, 5, device="cuda").to(torch.bfloat16).requires_grad_(True)
    y16 = m16(x16)
    assert "convt_train_fwd" in N.last_kernel() and y16.dtype == torch.bfloat16
    y16.float().sum().backward()
    assert m16.weight.grad.dtype == torch.bfloat16 and m16.bias.grad.dtype == torch.bfloat16 and x16.grad.dtype == torch.bfloat16
    ref = F.conv_transpose2d(x16.detach().float(), m16.weight.detach().float(), m16.bias.detach().float(), 2, 1)
    assert float((y16.detach().float() - ref).abs().max()) <= 2.0 ** -7 * float(ref.abs().max())


def test_declined_operands_take_the_module_path():
    """Channels-last, fp32 outside autocast, CPU tensors, channel counts and an output padding the kernels do not take: the swapped
    class computes nn.ConvTranspose2d.forward + the add, with STATS unchanged; the explicit call raises."""
    import torch
    import torch.nn as nn
    import torch.nn.functional as F
    from ssds.modeling.layers import convttrain as CT

    torch.manual_seed(1)
    m = CT.use_native_convt(nn.Sequential(nn.ConvTranspose2d(32, 16, 3, stride=2, padding=1)))[0].cuda()
    x = torch.randn(2, 32, 5, 4, device="cuda")
    sk = torch.randn(2, 16, 9, 7, device="cuda")
    before = dict(CT.STATS)

    def module(mod, xx, ss):
        return F.conv_transpose2d(xx, mod.weight, mod.bias, 2, 1, mod.output_padding[0]) + ss

    with torch.no_grad():
        assert torch.equal(m(x, skip=sk), module(m, x, sk))  # fp32, no autocast
        cl = x.bfloat16().to(memory_format=torch.channels_last)
        assert not cl.is_contiguous()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            assert torch.equal(m(cl, skip=sk), module(m, cl, sk))
            skcl = sk.to(memory_format=torch.channels_last)
            assert torch.equal(m(x, skip=skcl), module(m, x, skcl))
        mc = copy.deepcopy(m).cpu()
        assert torch.equal(mc(x.cpu(), skip=sk.cpu()), module(mc, x.cpu(), sk.cpu()))
        odd = nn.ConvTranspose2d(24, 16, 3, stride=2, padding=1).cuda()
        odd.__class__ = CT.ShelfConvT  # (use_native_convt would not take it)
        x24 = torch.randn(2, 24, 5, 4, device="cuda")
        pad = nn.ConvTranspose2d(32, 16, 3, stride=2, padding=1, output_padding=1).cuda()
        pad.__class__ = CT.ShelfConvT
        sk_pad = torch.randn(2, 16, 10, 8, device="cuda")
        with torch.autocast("cuda", dtype=torch.bfloat16):
            assert torch.equal(odd(x24, skip=sk), module(odd, x24, sk))
            assert torch.equal(pad(x, skip=sk_pad), module(pad, x, sk_pad))
    xb = x.bfloat16()
    for args in ((x, m.weight), (xb.cpu(), m.weight.cpu()), (cl, m.weight), (x24.bfloat16(), odd.weight),
                 (xb, m.weight, None, sk.bfloat16()[:, :, :-1]), (xb, m.weight.double())):
        with pytest.raises(ValueError):
            CT.convt3x3s2(*args)
    assert dict(CT.STATS) == before


def test_a_native_optimizer_step_between_two_calls_is_seen():
    """The images are packed again by every call: after a native SGD step (parameters updated through raw pointers) the next forward
    uses the updated weight and bias."""
    import torch
    import torch.nn.functional as F
    from ssds.core import optimizer as O
    from ssds.modeling.layers import convttrain as CT

    torch.manual_seed(3)
    dtype = torch.bfloat16
    m = CT.ShelfConvT(64, 32, 3, stride=2, padding=1).cuda()
    x = torch.randn(2, 64, 9, 7).to(dtype)
    sk = torch.randn(2, 32, 17, 13).to(dtype)
    xd, sd = x.cuda(), sk.cuda()
    with torch.autocast("cuda", dtype=dtype):
        y_before = m(xd, skip=sd)
    y_before.float().pow(2).mean().backward()
    opt = O.SsdkSGD(list(m.parameters()), lr=0.5, momentum=0.0, weight_decay=0.0)
    w_before = m.weight.detach().clone()
    opt.step()
    torch.cuda.synchronize()
    assert not torch.equal(m.weight.detach(), w_before), "the optimizer did not move the weight"
    with torch.autocast("cuda", dtype=dtype):
        y_after = m(xd, skip=sd).detach()
    want = F.conv_transpose2d(x.double(), m.weight.detach().to(dtype).double().cpu(), m.bias.detach().double().cpu(), 2, 1) + sk.double()
    _rounding_bar(y_after, want, 2.0 ** -8, "y after the optimizer step")
    assert not torch.equal(y_after, y_before.detach())


# ---- the whole neck in train mode -------------------------------------------------------------------------------------------------
def _rel(a, b):
    return float((a.double().cpu() - b.double()).norm() / b.double().norm().clamp(min=1e-12))


def _shelf():
    import torch.nn as nn
    from ssds.modeling.ssds.shelf import SSDShelf

    class Stub(nn.Module):
        """Three maps of 32 / 48 / 64 channels at 17 / 9 / 5 pixels of a 33 x 33 image."""

        def __init__(self):
            super(Stub, self).__init__()
            self.c = nn.ModuleList([nn.Conv2d(3, ch, 1, stride=s) for ch, s in ((32, 2), (48, 4), (64, 8))])

        def initialize(self):
            return None

        def forward(self, x):
            return [c(x) for c in self.c]

    _, extras, head = SSDShelf.add_extras([[0, 1, 2], [32, 48, 64]], [2, 2, 2], 3)
    model = SSDShelf(Stub(), extras, head, 3)
    for m in model.modules():
        if isinstance(m, nn.Dropout2d):
            m.p = 0.0  # the CPU and GPU generators differ
    return model


def _neck_run(module, image, native, device):
    """One train-mode forward + backward -> {name: tensor} of outputs, the input gradient and every parameter gradient."""
    import torch
    from ssds.modeling.layers import convttrain as CT

    m = copy.deepcopy(module).to(device).train()
    if native:
        CT.use_native_convt(m)
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


def test_whole_neck_in_train_mode():
    """SSDShelf on a three-map stub backbone, N = 2, train mode, Dropout2d.p = 0, bf16 autocast, with use_native_convt, against the
    fp64 CPU model: per tensor (outputs, input gradient, every parameter gradient) rel(native) <= 2 rel(floor) + 0.02, the floor
    being the same bf16-autocast module with the swap off (the rule of tests/test_gpu_necktrain.py::test_whole_neck_in_train_mode)."""
    import torch
    from ssds.modeling.layers import convttrain as CT

    torch.manual_seed(6)
    module = _shelf()
    image = torch.randn(2, 3, 33, 33)
    want = _neck_run(module.double(), image, False, "cpu")
    module = module.float()
    calls = dict(CT.STATS)
    got = _neck_run(module, image, True, "cuda")
    delta = {k: CT.STATS[k] - calls[k] for k in calls}
    assert delta == dict(swapped=4, native_forward=4, native_dgrad=4, native_wgrad=4), "the native path did not run"
    calls = dict(CT.STATS)
    floor = _neck_run(module, image, False, "cuda")
    assert dict(CT.STATS) == calls
    assert set(got) == set(want) == set(floor)
    bad = []
    for k in sorted(want):
        rn, rf = _rel(got[k], want[k]), _rel(floor[k], want[k])
        print("shelf %-52s rel native %.5f floor %.5f" % (k, rn, rf))
        if not rn <= 2.0 * rf + 0.02:
            bad.append((k, rn, rf))
    assert not bad, bad


_SWITCH = r"""
import sys, math, torch
sys.path[:0] = [%(root)r, %(pkg)r]
from ssds.core import config
from ssds.utils import train_ddp
from ssds.modeling.layers import convttrain as CT
cfg = config.cfg_from_file(%(cfg)r)
s = train_ddp.Solver(cfg, 0, torch.device("cuda", 0))
net = s.model
net.train()
x = torch.randn(2, 3, 129, 129, device="cuda")
with torch.autocast("cuda", dtype=torch.bfloat16):
    loc, conf = net(x)
loss = sum(o.float().pow(2).mean() for o in tuple(loc) + tuple(conf))
s.optimizer.zero_grad()
loss.backward()
s.optimizer.step()
torch.cuda.synchronize()
grads = [p.grad for p in net.parameters() if p.grad is not None]
finite = math.isfinite(float(loss)) and all(bool(torch.isfinite(g).all()) for g in grads)
print("RESULT", sum(type(m) is CT.ShelfConvT for m in net.modules()), CT.STATS["swapped"], CT.STATS["native_forward"], CT.STATS["native_dgrad"],
      CT.STATS["native_wgrad"], int(finite), len(grads))
"""


@pytest.mark.parametrize("switch", ["0", "1"])
def test_the_switch(switch):
    """The Solver-built model of shelf_resnet18_513.yml takes one training step (forward, backward, optimizer) at batch 2 and image
    size 129, in a subprocess: with SSDK_CONVT_TRAIN=1 four layers are swapped, the kernels run as often backward as forward, and
    the loss and gradients are finite; with 0 every count is zero."""
    env = dict(os.environ, SSDK_CONVT_TRAIN=switch)
    code = _SWITCH % dict(root=ROOT, pkg=os.path.join(ROOT, "ssds.pytorch_amd"),
                          cfg=os.path.join(ROOT, "experiments", "cfgs", "shelf_resnet18_513.yml"))
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    res = [int(v) for v in [l for l in out.stdout.splitlines() if l.startswith("RESULT")][-1].split()[1:]]
    cls, swapped, nf, nd, nw, finite, ngrads = res
    assert finite == 1 and ngrads > 0
    if switch == "0":
        assert res[:5] == [0] * 5
    else:
        assert cls == swapped == 4 and nf == nd == nw == 4
