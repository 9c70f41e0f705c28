"""The 7x7 / stride 2 / pad 3 stem convolution of the ResNet / ResNeXt backbones inside the TRAINING step on the GPU
(csrc/ssdk_stem7train.hip behind ssds/modeling/layers/stemconv.py): forward and weight gradient of single layers per element
against ``F.conv2d`` autograd in fp64 on the CPU on the same 16-bit-rounded operands, exact all-ones and one-hot cases,
bit-reproducibility, misaligned bases, the autocast contract, hipGraph capture, the ResNet stem in train mode against the
PyTorch-ROCm floor, and the switch.

The bars are those of tests/test_gpu_dense3_train.py: y per element within eps |want| + 4 eps rms(want) (eps = 2^-8 bf16,
2^-10 fp16), dW per element within 2e-5 max|want| + 1e-6.  No element is left out."""
import functools
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# N, Cin, H, W, Cout: each the smallest shape that reaches its edge
CASES = [
    (2, 3, 1, 1, 64),     # only the centre tap inside
    (1, 3, 7, 9, 64),     # odd sizes, every window clipped
    (2, 3, 16, 32, 64),   # rows of whole 16-byte groups
    (2, 3, 17, 33, 64),   # one element over
    (1, 3, 64, 64, 64),   # several output rows per wave
    (3, 3, 40, 48, 64),   # several images, more than one workgroup partial
    (1, 1, 12, 16, 64),   # Cin = 1
    (2, 3, 20, 32, 40),   # ragged Cout: no store from padding lanes (guard bands)
    (1, 3, 5, 608, 64),   # wide row
    (1, 2, 9, 30, 16),    # one fragment
]
DTYPES = {"bf16": 2.0 ** -8, "f16": 2.0 ** -10}


def _dtype(name):
    import torch

    return torch.bfloat16 if name == "bf16" else torch.float16


def _seed(n, cin, h, w, cout):
    return 100000 * 2 + 1000 * cin + 10 * cout + 7 * h + 3 * w + n


@functools.lru_cache(maxsize=None)
def _case(n, cin, h, w, cout, dtype_name):
    """x, dy ~ N(0, 1), w ~ N(0, 2 / (49 Cin)); all rounded to the dtype (w kept as the fp32 master tensor holding rounded values),
    with the fp64 CPU truth (y, dW).  Computed once per case and shared; nobody writes to it."""
    import torch
    import torch.nn.functional as F

    dtype = _dtype(dtype_name)
    g = torch.Generator().manual_seed(_seed(n, cin, h, w, cout))
    x = torch.randn(n, cin, h, w, generator=g).to(dtype)
    wt = (torch.randn(cout, cin, 7, 7, generator=g) * (2.0 / (49 * cin)) ** 0.5).to(dtype).float()
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    dy = torch.randn(n, cout, ho, wo, generator=g).to(dtype)
    w64 = wt.double().requires_grad_(True)
    y64 = F.conv2d(x.double(), w64, None, 2, 3)
    y64.backward(dy.double())
    return x, wt, dy, y64.detach(), w64.grad


def _native(x, wt, dy):
    import torch
    from ssds.modeling.layers import stemconv as S

    wd = wt.cuda().requires_grad_(True)
    y = S.stem_conv7x7s2(x.cuda(), wd)
    y.backward(dy.cuda())
    torch.cuda.synchronize()
    return y.detach(), wd.grad


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


def _guarded(shape, dtype):
    """A contiguous view of ``shape`` inside a larger NaN-filled allocation -> view, whole buffer, guard length."""
    import torch

    per = 1
    for v in shape:
        per *= v
    guard = 4096
    big = torch.full((guard + per + guard,), float("nan"), dtype=dtype, device="cuda")
    return big[guard:guard + per].view(shape), big, guard


@pytest.mark.parametrize("n,cin,h,w,cout", CASES)
@pytest.mark.parametrize("dtype_name", sorted(DTYPES))
def test_stem7_train_single_layer(n, cin, h, w, cout, dtype_name):
    import torch
    from ssds import _native as N

    dtype, eps = _dtype(dtype_name), DTYPES[dtype_name]
    x, wt, dy, y64, dw64 = _case(n, cin, h, w, cout, dtype_name)
    tag = "%dx%dx%dx%d->%d %s" % (n, cin, h, w, cout, dtype_name)
    if cout % 16:
        # the entry points themselves with y and dW inside NaN-filled buffers: padding lanes store nothing
        xd, wd, dyd = x.cuda(), wt.cuda(), dy.cuda()
        y, keep_y, gy_ = _guarded(tuple(y64.shape), dtype)
        dw, keep_w, gw_ = _guarded((cout, cin, 7, 7), torch.float32)
        need = int(N.lib.ssdk_stem7x7s2_wgrad_workspace_bytes(n, h, w, cout))
        ws = torch.empty(need + 16, dtype=torch.uint8, device="cuda")
        sp, code = N.stream_ptr(xd.device), N.dtype_code(xd)
        N.check(N.lib.ssdk_stem7x7s2_fwd(xd.data_ptr(), wd.data_ptr(), y.data_ptr(), n, cin, h, w, cout, code, sp), "stem7x7s2_fwd")
        assert "stem7_train" in N.last_kernel(), N.last_kernel()
        N.check(N.lib.ssdk_stem7x7s2_wgrad(xd.data_ptr(), dyd.data_ptr(), dw.data_ptr(), (ws.data_ptr() + 15) & ~15, need, n, cin, h, w, cout,
                                           code, sp), "stem7x7s2_wgrad")
        torch.cuda.synchronize()
        for got, big, guard, what in ((y, keep_y, gy_, "y"), (dw, keep_w, gw_, "dW")):
            per = got.numel()
            assert bool(torch.isnan(big[:guard]).all()) and bool(torch.isnan(big[guard + per:]).all()), what + ": written outside"
            assert not bool(torch.isnan(got).any()), what + ": elements left unwritten"
    else:
        y, dw = _native(x, wt, dy)
    assert "stem7_train" in N.last_kernel(), N.last_kernel()
    assert y.dtype == dtype and y.is_contiguous() and tuple(y.shape) == tuple(y64.shape)
    assert dw.dtype == torch.float32 and tuple(dw.shape) == (cout, cin, 7, 7)
    _rounding_bar(y, y64, eps, "y " + tag)
    _wgrad_bar(dw, dw64, "dW " + tag)


@pytest.mark.parametrize("n,cin,h,w,cout", [(2, 3, 17, 33, 64), (3, 3, 40, 48, 64)])
@pytest.mark.parametrize("dtype_name", sorted(DTYPES))
def test_all_ones_are_exact_counts(n, cin, h, w, cout, dtype_name):
    """x = 1 and w = 1: y is the number of taps inside the image times Cin (<= 147: exact in both dtypes); dy = 1: dW is the number of
    output pixels whose window holds the tap.  No tolerance."""
    import torch
    import torch.nn.functional as F

    dtype = _dtype(dtype_name)
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    x, wt, dy = torch.ones(n, cin, h, w, dtype=dtype), torch.ones(cout, cin, 7, 7), torch.ones(n, cout, ho, wo, dtype=dtype)
    w64 = wt.double().requires_grad_(True)
    y64 = F.conv2d(x.double(), w64, None, 2, 3)
    y64.backward(dy.double())
    assert float(y64.max()) <= 147 and float(y64.min()) >= 16 * cin
    y, dw = _native(x, wt, dy)
    assert torch.equal(y.double().cpu(), y64.detach())
    assert torch.equal(dw.double().cpu(), w64.grad)


@pytest.mark.parametrize("n,cin,h,w,cout", [(2, 3, 17, 33, 64), (1, 3, 64, 64, 64)])
def test_one_hot_dy_is_the_patch(n, cin, h, w, cout):
    """dy a single -1.3125 at one pixel of one channel (the four corners and an interior pixel of the last image, one run each):
    dW of that channel is -1.3125 times the patch of x around the pixel, exactly, and every other channel is zero."""
    import torch
    import torch.nn.functional as F

    x = _case(n, cin, h, w, cout, "bf16")[0]
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    xp = F.pad(x.double(), (3, 3, 3, 3))
    wt = torch.zeros(cout, cin, 7, 7)
    for k, (oy, ox) in enumerate([(0, 0), (0, wo - 1), (ho - 1, 0), (ho - 1, wo - 1), (ho // 2, wo // 2 + 1)]):
        co = (13 * k + 5) % cout
        dy = torch.zeros(n, cout, ho, wo, dtype=torch.bfloat16)
        dy[n - 1, co, oy, ox] = -1.3125
        _, dw = _native(x, wt, dy)
        want = torch.zeros(cout, cin, 7, 7, dtype=torch.float64)
        want[co] = -1.3125 * xp[n - 1, :, 2 * oy:2 * oy + 7, 2 * ox:2 * ox + 7]
        assert torch.equal(dw.double().cpu(), want), (oy, ox, co)


@pytest.mark.parametrize("n,cin,h,w,cout", [(3, 3, 40, 48, 64), (1, 3, 64, 64, 64)])
def test_forward_and_weight_gradient_are_bit_reproducible(n, cin, h, w, cout):
    import torch

    x, wt, dy = _case(n, cin, h, w, cout, "bf16")[:3]
    r1 = _native(x, wt, dy)
    r2 = _native(x, wt, dy)
    for u, v, what in zip(r1, r2, ("y", "dW")):
        assert torch.equal(u, v), what


@pytest.mark.parametrize("n,cin,h,w,cout", [(2, 3, 16, 32, 64), (2, 3, 17, 33, 64), (3, 3, 40, 48, 64)])
def test_misaligned_bases(n, cin, h, w, cout):
    """x, dy and w as views that start 1, 3 and 1 elements into their allocations: bit-equal to the aligned run."""
    import torch
    from ssds.modeling.layers import stemconv as S

    x, wt, dy = _case(n, cin, h, w, cout, "bf16")[:3]
    want = _native(x, wt, dy)

    def view(t, off):
        big = torch.zeros(t.numel() + off + 8, dtype=t.dtype, device="cuda")
        big[off:off + t.numel()] = t.reshape(-1).cuda()
        v = big[off:off + t.numel()].view(t.shape)
        assert v.is_contiguous() and v.data_ptr() == big.data_ptr() + off * t.element_size()
        return v

    xv, dv = view(x, 1), view(dy, 3)
    wv = view(wt, 1).requires_grad_(True)
    y = S.stem_conv7x7s2(xv, wv)
    y.backward(dv)
    torch.cuda.synchronize()
    assert torch.equal(y.detach(), want[0]), "y"
    assert torch.equal(wv.grad, want[1]), "dW"


def test_autocast_contract():
    import torch
    import torch.nn as nn
    import torch.nn.functional as F
    from ssds import _native as N
    from ssds.modeling.layers import stemconv as S

    torch.manual_seed(0)
    seq = nn.Sequential(nn.Conv2d(3, 64, 7, 2, 3, bias=False))
    assert S.use_native_stem7(seq) == 1
    m = seq[0].cuda()
    assert type(m) is S.StemConv7x7s2 and m.weight.dtype == torch.float32
    with torch.no_grad():
        m.weight.copy_(m.weight.to(torch.bfloat16).float())  # a master weight that holds bf16 values: the truth below is exact about it
    x = torch.randn(2, 3, 20, 24, device="cuda").to(torch.bfloat16).float()
    calls = dict(S.STATS)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        y = m(x)
    assert y.dtype == torch.bfloat16 and "stem7_train" in N.last_kernel()
    y.float().sum().backward()
    assert m.weight.grad.dtype == torch.float32 and m.weight.grad.shape == m.weight.shape
    assert [S.STATS[k] - calls[k] for k in ("native_forward", "native_wgrad", "fallback")] == [1, 1, 0]
    # fp32 tensors outside autocast: nn.Conv2d.forward, and the counters say so
    calls = dict(S.STATS)
    y32 = m(x)
    assert y32.dtype == torch.float32
    assert [S.STATS[k] - calls[k] for k in ("native_forward", "native_wgrad", "fallback")] == [0, 0, 1]
    # an image that asks for its gradient gets it (from the framework's convolution backward), within one rounding of the fp64 one
    m.weight.grad = None
    xg = x.clone().requires_grad_(True)
    dy = torch.randn(2, 64, 10, 12, device="cuda").to(torch.bfloat16)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        y = m(xg)
    y.backward(dy)
    torch.cuda.synchronize()
    assert xg.grad.dtype == torch.float32 and xg.grad.shape == xg.shape
    x64 = x.double().cpu().requires_grad_(True)
    w64 = m.weight.detach().double().cpu().requires_grad_(True)
    F.conv2d(x64, w64, None, 2, 3).backward(dy.double().cpu())
    _rounding_bar(xg.grad, x64.grad, 2.0 ** -8, "dx under autocast")
    _wgrad_bar(m.weight.grad, w64.grad, "dW under autocast")


def test_forward_and_backward_capture_into_a_graph():
    """Capture forward + backward of one layer after a warm-up, replay twice: equal to the eager results (the queue count is the
    machine's default)."""
    import torch
    from ssds.modeling.layers import stemconv as S

    x, wt, dy = _case(3, 3, 40, 48, 64, "bf16")[:3]
    eager = _native(x, wt, dy)
    xs = x.cuda()
    ws = wt.cuda().requires_grad_(True)
    dys = dy.cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up on a side stream, as torch.cuda.graph asks
        for _ in range(2):
            y = S.stem_conv7x7s2(xs, ws)
            (gw_,) = torch.autograd.grad(y, (ws,), dys)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        y = S.stem_conv7x7s2(xs, ws)
        (gw_,) = torch.autograd.grad(y, (ws,), dys)
    for _ in range(2):
        y.detach().zero_()
        gw_.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(y.detach(), eager[0]) and torch.equal(gw_, eager[1])


def _rel(a, b):
    return float((a.double().cpu() - b.double()).norm() / b.double().norm().clamp(min=1e-12))


def _stem_run(stem, x, native):
    """One train-mode forward + backward of the stem under bf16 autocast on the GPU -> {name: tensor} of the output and every
    parameter gradient.  ``native``: BatchNorm and the 7x7 layer on the ssdk kernels, else nn.Conv2d (the PyTorch-ROCm floor)."""
    import copy

    import torch
    from ssds.modeling.layers import stemconv as S
    from ssds.modeling.layers.batchnorm import use_fast_batchnorm

    m = copy.deepcopy(stem).cuda().train()
    if native:
        use_fast_batchnorm(m)
        assert S.use_native_stem7(m) == 1
    with torch.autocast("cuda", dtype=torch.bfloat16):
        y = m(x.cuda())
    y.float().pow(2).mean().backward()
    torch.cuda.synchronize()
    out = {"output": y.detach().float()}
    out.update({k + ".grad": p.grad for k, p in m.named_parameters()})
    return out


def test_resnet_stem_in_train_mode():
    """conv1, bn1, relu, maxpool of nets.resnet.ResNet in train mode, bf16 autocast, with use_fast_batchnorm + use_native_stem7,
    against the fp32 CPU module: per tensor (output, every parameter gradient) rel(native) <= 2 rel(floor) + 0.02, the floor being
    the same bf16-autocast module left on nn.Conv2d (the rule of tests/test_gpu_dense3_train.py::test_one_block_in_train_mode)."""
    import copy

    import torch
    import torch.nn as nn
    from ssds.modeling.layers import stemconv as S
    from ssds.modeling.nets.resnet import BasicBlock, ResNet

    torch.manual_seed(5)
    net = ResNet(layers=[1, 1, 1, 1], bottleneck=BasicBlock, outputs=[2])
    stem = nn.Sequential(net.conv1, net.bn1, net.relu, net.maxpool)
    x = torch.randn(4, 3, 64, 64)
    ref = copy.deepcopy(stem).train()
    yr = ref(x)
    yr.pow(2).mean().backward()
    want = {"output": yr.detach()}
    want.update({k + ".grad": p.grad for k, p in ref.named_parameters()})
    calls = dict(S.STATS)
    got = _stem_run(stem, x, True)
    assert [S.STATS[k] - calls[k] for k in ("native_forward", "native_wgrad", "fallback")] == [1, 1, 0], "the native path did not run"
    floor = _stem_run(stem, x, False)
    assert set(got) == set(want) == set(floor)
    bad = []
    for k in sorted(want):
        rn, rf = _rel(got[k], want[k]), _rel(floor[k], want[k])
        print("resnet stem %-16s rel native %.5f floor %.5f" % (k, rn, rf))
        if not rn <= 2.0 * rf + 0.02:
            bad.append((k, rn, rf))
    assert not bad, bad


_SWITCH = r"""
import sys, torch
sys.path[:0] = [%(root)r, %(pkg)r]
import torch.nn as nn
from ssds.core import config
from ssds.utils import train_ddp
from ssds.modeling.layers import stemconv as S
cfg = config.cfg_from_file(%(cfg)r)
s = train_ddp.Solver(cfg, 0, torch.device("cuda", 0))
net = s.model
net.train()
x = torch.randn(2, 3, 128, 128, device="cuda")
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
sum(o.float().pow(2).mean() for o in flat if o.requires_grad).backward()
torch.cuda.synchronize()
grads = [p.grad for p in net.parameters() if p.grad is not None]
finite = all(bool(torch.isfinite(g).all()) for g in grads)
conv1 = net.backbone.conv1
print("RESULT", int(type(conv1) is S.StemConv7x7s2), int(type(conv1) is nn.Conv2d), S.STATS["swapped"], S.STATS["native_forward"],
      S.STATS["native_wgrad"], S.STATS["fallback"], int(finite), len(grads), int(conv1.weight.grad is not None))
"""


@pytest.mark.parametrize("switch", ["0", "1"])
def test_the_switch(switch):
    """SSDK_STEM7_TRAIN in a subprocess: the Solver-built fpn_resnet50_640 model takes one train-mode forward + backward at batch 2,
    128 px, with finite gradients.  =1: backbone.conv1 is a StemConv7x7s2 and ran natively once, forward and weight gradient;
    =0: plain nn.Conv2d and every counter zero."""
    env = dict(os.environ, SSDK_STEM7_TRAIN=switch)
    code = _SWITCH % dict(root=ROOT, pkg=os.path.join(ROOT, "ssds.pytorch_amd"),
                          cfg=os.path.join(ROOT, "experiments", "cfgs", "fpn_resnet50_640.yml"))
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    native, plain, swapped, nf, nw, fb, finite, ngrads, has_grad = (
        int(v) for v in [l for l in out.stdout.splitlines() if l.startswith("RESULT")][-1].split()[1:])
    assert finite == 1 and ngrads > 0 and has_grad == 1
    if switch == "0":
        assert (native, plain, swapped, nf, nw, fb) == (0, 1, 0, 0, 0, 0)
    else:
        assert (native, plain, swapped, nf, nw, fb) == (1, 0, 1, 1, 1, 0)
