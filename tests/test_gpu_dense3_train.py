"""Dense 3x3 convolutions of the TRAINING step on the GPU (csrc/ssdk_conv3train.hip behind ssds/modeling/layers/denseconv.py):
forward, input gradient and weight gradient of single layers per element against ``F.conv2d`` autograd in fp64 on the CPU on the
same 16-bit-rounded operands, bit-reproducibility, the device packer against its torch twins, inert padding, the autocast
contract, hipGraph capture, the bias epilogue, a shared weight on several maps and across a native optimizer step, a ResNet
bottleneck and an FPN tower in train mode against the PyTorch-ROCm floor, and the switch.

The bars are those of tests/test_gpu_gconv_train.py: y and dx per element within eps |want| + 4 eps rms(want) (eps = 2^-8 bf16,
2^-10 fp16), dW per element within 2e-5 max|want| + 1e-6."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Cin, Cout, stride, H, W, N, bias
CASES = [
    (64, 64, 1, 40, 40, 2, False), (128, 128, 2, 40, 40, 2, False), (256, 256, 1, 40, 40, 2, False), (256, 256, 2, 10, 10, 2, False),
    (512, 512, 1, 20, 20, 2, False), (512, 512, 2, 20, 20, 1, False),
    (256, 36, 1, 20, 20, 2, True), (256, 720, 1, 10, 10, 2, True),
    (2048, 256, 2, 20, 20, 1, False), (912, 256, 2, 28, 28, 1, False),
    (256, 256, 1, 5, 5, 3, False), (256, 256, 1, 7, 7, 2, False), (256, 256, 1, 33, 31, 2, False), (64, 128, 2, 17, 23, 2, False),
    (256, 256, 1, 112, 112, 1, False), (256, 256, 2, 5, 5, 2, False), (16, 4, 1, 3, 2, 2, True), (256, 256, 1, 1, 1, 8, False),
    (256, 256, 1, 80, 80, 4, False),
]


def _seed(cin, cout, stride, h, w, n):
    return 100000 * stride + 1000 * (cin % 997) + 10 * cout + 7 * h + 3 * w + n


def _operands(cin, cout, stride, h, w, n, bias, dtype, seed=None):
    """x, dy ~ N(0, 1), w ~ N(0, 2 / (9 Cin)), bias ~ N(0, 1); x, dy, w rounded to ``dtype`` (w kept as the fp32 master tensor
    holding rounded values)."""
    import torch

    g = torch.Generator().manual_seed(_seed(cin, cout, stride, h, w, n) if seed is None else seed)
    x = torch.randn(n, cin, h, w, generator=g).to(dtype)
    wt = (torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (9 * cin)) ** 0.5).to(dtype).float()
    ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
    dy = torch.randn(n, cout, ho, wo, generator=g).to(dtype)
    b = torch.randn(cout, generator=g) if bias else None
    return x, wt, b, dy


def _truth(x, wt, b, dy, stride):
    """F.conv2d autograd in fp64 on the CPU -> y, dx, dW."""
    import torch.nn.functional as F

    x64 = x.double().requires_grad_(True)
    w64 = wt.double().requires_grad_(True)
    y = F.conv2d(x64, w64, None if b is None else b.double(), stride, 1)
    y.backward(dy.double())
    return y.detach(), x64.grad, w64.grad


def _native(x, wt, b, dy, stride):
    import torch
    from ssds.modeling.layers import denseconv as D

    xd = x.cuda().requires_grad_(True)
    wd = wt.cuda().requires_grad_(True)
    y = D.dense_conv3x3(xd, wd, None if b is None else b.cuda(), stride)
    y.backward(dy.cuda())
    torch.cuda.synchronize()
    return y.detach(), xd.grad, wd.grad


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


@pytest.mark.parametrize("cin,cout,stride,h,w,n,bias", CASES)
@pytest.mark.parametrize("dtype_name", ["bf16", "f16"])
def test_dense_conv_train_single_layer(cin, cout, stride, h, w, n, bias, dtype_name):
    import torch
    from ssds import _native as N

    dtype = torch.bfloat16 if dtype_name == "bf16" else torch.float16
    eps = 2.0 ** -8 if dtype_name == "bf16" else 2.0 ** -10
    x, wt, b, dy = _operands(cin, cout, stride, h, w, n, bias, dtype)
    y64, dx64, dw64 = _truth(x, wt, b, dy, stride)
    y, dx, dw = _native(x, wt, b, dy, stride)
    assert "conv3_train" in N.last_kernel(), N.last_kernel()
    tag = "%d->%d s%d %dx%d n=%d %s" % (cin, cout, stride, h, w, n, dtype_name)
    assert y.dtype == dtype and y.is_contiguous() and tuple(y.shape) == tuple(y64.shape)
    assert dx.dtype == dtype and dx.is_contiguous() and tuple(dx.shape) == tuple(x.shape)
    assert dw.dtype == torch.float32 and tuple(dw.shape) == (cout, cin, 3, 3)
    _rounding_bar(y, y64, eps, "y " + tag)
    _rounding_bar(dx, dx64, eps, "dx " + tag)
    _wgrad_bar(dw, dw64, "dW " + tag)


@pytest.mark.parametrize("cin,cout,stride,h,w,n,bias", [(256, 256, 1, 80, 80, 4, False), (128, 128, 2, 40, 40, 2, False),
                                                        (256, 36, 1, 20, 20, 2, True), (912, 256, 2, 28, 28, 1, False)])
def test_forward_and_backward_are_bit_reproducible(cin, cout, stride, h, w, n, bias):
    import torch

    x, wt, b, dy = _operands(cin, cout, stride, h, w, n, bias, torch.bfloat16, seed=7)
    r1 = _native(x, wt, b, dy, stride)
    r2 = _native(x, wt, b, dy, stride)
    for u, v, what in zip(r1, r2, ("y", "dx", "dW")):
        assert torch.equal(u, v), what


@pytest.mark.parametrize("dtype_name", ["bf16", "f16"])
@pytest.mark.parametrize("cin,cout", [(64, 64), (256, 36), (912, 256), (16, 4), (256, 720)])
def test_device_packer_matches_the_torch_twins(cin, cout, dtype_name):
    """ssdk_conv3x3_train_prepare == pack_dense_frag / pack_dense_frag_dgrad of the cast weights, bit for bit."""
    import torch
    from ssds.modeling.layers import denseconv as D

    dtype = torch.bfloat16 if dtype_name == "bf16" else torch.float16
    torch.manual_seed(cin + cout)
    w32 = torch.randn(cout, cin, 3, 3) * 0.1  # NOT pre-rounded: the packer's cast is part of the comparison
    fwd, dg = D.prepare_images(w32.cuda(), dtype)
    torch.cuda.synchronize()
    want_f, want_d = D.pack_dense_frag(w32.to(dtype)), D.pack_dense_frag_dgrad(w32.to(dtype))
    assert fwd.dtype == dtype and tuple(fwd.shape) == tuple(want_f.shape) and tuple(dg.shape) == tuple(want_d.shape)
    assert torch.equal(fwd.cpu().view(torch.int16), want_f.view(torch.int16)), "forward image"
    assert torch.equal(dg.cpu().view(torch.int16), want_d.view(torch.int16)), "input-gradient image"
    only_f, none = D.prepare_images(w32.cuda(), dtype, want_dgrad=False)
    assert none is None and torch.equal(only_f, fwd)


@pytest.mark.parametrize("cin,cout,stride,bias", [(64, 36, 1, True), (64, 36, 2, True), (48, 64, 1, False), (48, 64, 2, False)])
def test_padding_is_inert(cin, cout, stride, bias):
    """x, dy, the weight images' source, the bias and (through the explicit entry points) the outputs live inside larger
    NaN-filled allocations: results are finite, bit-identical to those of clean copies, and nothing is written outside the outputs."""
    import torch
    from ssds import _native as N
    from ssds.modeling.layers import denseconv as D

    dtype = torch.bfloat16
    n, h, w = 2, 13, 11
    x, wt, b, dy = _operands(cin, cout, stride, h, w, n, bias, dtype, seed=3)

    def guarded(t, dt=None):
        dt = dt or t.dtype
        per = t.numel()
        guard = 4096 + per
        big = torch.full((guard + per + guard,), float("nan"), dtype=dt, device="cuda")
        big[guard:guard + per] = t.reshape(-1).to(dt).cuda()
        v = big[guard:guard + per].view(t.shape)
        assert v.is_contiguous()
        return v, big, guard

    def run(xd, wd, bd, dyd):
        xd = xd.detach().requires_grad_(True)
        wd = wd.detach().requires_grad_(True)
        y = D.dense_conv3x3(xd, wd, bd, stride)
        y.backward(dyd)
        torch.cuda.synchronize()
        return y.detach(), xd.grad, wd.grad

    xv, keep_x, _ = guarded(x)
    dv, keep_d, _ = guarded(dy)
    wv, keep_w, _ = guarded(wt)
    bv = None
    if b is not None:
        bv, keep_b, _ = guarded(b)
    view = run(xv, wv, bv, dv)
    clean = run(x.cuda(), wt.cuda(), None if b is None else b.cuda(), dy.cuda())
    for u, v, what in zip(view, clean, ("y", "dx", "dW")):
        assert not torch.isnan(u).any() and not torch.isnan(v).any(), what
        assert torch.equal(u, v), what
    # one image alone between NaN neighbours
    one = run(guarded(x[:1])[0], wv, bv, guarded(dy[:1])[0])
    ref1 = run(x[:1].cuda(), wt.cuda(), None if b is None else b.cuda(), dy[:1].cuda())
    for u, v, what in zip(one, ref1, ("y", "dx", "dW")):
        assert not torch.isnan(u).any() and torch.equal(u, v), what
    assert torch.equal(one[0], clean[0][:1]) and torch.equal(one[1], clean[1][:1])
    # the entry points themselves with images and outputs inside NaN-filled buffers: nothing outside the outputs is written
    ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
    fwd, dg = D.prepare_images(wt.cuda(), dtype)
    fv, keep_f, _ = guarded(fwd)
    gv, keep_g, _ = guarded(dg)
    yv, keep_y, gy_ = guarded(torch.zeros(n, cout, ho, wo, dtype=dtype))
    dxv, keep_dx, gx_ = guarded(torch.zeros(n, cin, h, w, dtype=dtype))
    dwv, keep_dw, gw_ = guarded(torch.zeros(cout, cin, 3, 3))
    need = int(N.lib.ssdk_conv3x3_train_wgrad_workspace_bytes(n, cin, cout, h, w, stride))
    ws = torch.empty(need + 16, dtype=torch.uint8, device="cuda")
    sp, code = N.stream_ptr(xv.device), N.dtype_code(xv)
    N.check(N.lib.ssdk_conv3x3_train_forward(xv.data_ptr(), fv.data_ptr(), None if bv is None else bv.data_ptr(), yv.data_ptr(), n, cin, cout,
                                             h, w, stride, code, sp), "forward")
    N.check(N.lib.ssdk_conv3x3_train_dgrad(dv.data_ptr(), gv.data_ptr(), dxv.data_ptr(), n, cin, cout, h, w, stride, code, sp), "dgrad")
    N.check(N.lib.ssdk_conv3x3_train_wgrad(xv.data_ptr(), dv.data_ptr(), dwv.data_ptr(), (ws.data_ptr() + 15) & ~15, need, n, cin, cout, h, w,
                                           stride, code, sp), "wgrad")
    torch.cuda.synchronize()
    for got, want, big, guard, what in ((yv, clean[0], keep_y, gy_, "y"), (dxv, clean[1], keep_dx, gx_, "dx"), (dwv, clean[2], keep_dw, gw_, "dW")):
        assert torch.equal(got, want), what
        per = got.numel()
        assert bool(torch.isnan(big[:guard]).all()) and bool(torch.isnan(big[guard + per:]).all()), what + ": written outside"
    y64, dx64, dw64 = _truth(x, wt, b, dy, stride)
    _rounding_bar(clean[0], y64, 2.0 ** -8, "y padding case")
    _rounding_bar(clean[1], dx64, 2.0 ** -8, "dx padding case")
    _wgrad_bar(clean[2], dw64, "dW padding case")


def test_autocast_contract():
    import torch
    import torch.nn as nn
    from ssds import _native as N
    from ssds.modeling.layers import denseconv as D

    torch.manual_seed(0)
    m = D.use_native_dense3x3(nn.Sequential(nn.Conv2d(64, 96, 3, 2, 1, bias=False)))[0].cuda()
    assert type(m) is D.DenseConv3x3 and m.weight.dtype == torch.float32
    x = torch.randn(2, 64, 20, 16, device="cuda", requires_grad=True)
    calls = dict(D.STATS)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        y = m(x)
    assert y.dtype == torch.bfloat16 and "conv3_train" in N.last_kernel()
    y.float().sum().backward()
    assert m.weight.grad.dtype == torch.float32 and m.weight.grad.shape == m.weight.shape
    assert x.grad.dtype == torch.float32 and x.grad.shape == x.shape
    assert [D.STATS[k] - calls[k] for k in ("native_forward", "native_dgrad", "native_wgrad")] == [1, 1, 1]
    # an input that needs no gradient: no input-gradient call
    calls = dict(D.STATS)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        m(x.detach()).float().sum().backward()
    assert [D.STATS[k] - calls[k] for k in ("native_forward", "native_dgrad", "native_wgrad")] == [1, 0, 1]
    # 16-bit weights are taken too, and give a 16-bit weight gradient
    m16 = D.DenseConv3x3(64, 36, 3, 1, 1, bias=True).cuda().to(torch.bfloat16)
    x16 = torch.randn(2, 64, 9, 9, device="cuda").to(torch.bfloat16).requires_grad_(True)
    y16 = m16(x16)
    assert "conv3_train" in N.last_kernel()
    y16.float().sum().backward()
    assert m16.weight.grad.dtype == torch.bfloat16 and m16.bias.grad.dtype == torch.bfloat16
    ref = torch.nn.functional.conv2d(x16.detach().float(), m16.weight.detach().float(), m16.bias.detach().float(), 1, 1)
    assert float((y16.float() - ref).abs().max()) <= 2.0 ** -7 * float(ref.abs().max())
    # fp32 tensors outside autocast and non-contiguous tensors: nn.Conv2d.forward
    calls = dict(D.STATS)
    y32 = m(x.detach())
    assert y32.dtype == torch.float32
    with torch.autocast("cuda", dtype=torch.bfloat16):
        m(x.detach().to(memory_format=torch.channels_last))
    assert dict(D.STATS) == calls


def test_forward_and_backward_capture_into_a_graph():
    """Capture forward + backward of one layer after a warm-up, replay twice: equal to the eager results (the queue count is the
    machine's default)."""
    import torch
    from ssds.modeling.layers import denseconv as D

    cin, cout, stride = 64, 36, 2
    x, wt, b, dy = _operands(cin, cout, stride, 28, 20, 2, True, torch.bfloat16, seed=11)
    eager = _native(x, wt, b, dy, stride)
    xs = x.cuda().requires_grad_(True)
    ws = wt.cuda().requires_grad_(True)
    bs = b.cuda()
    dys = dy.cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up on a side stream, as torch.cuda.graph asks
        for _ in range(2):
            y = D.dense_conv3x3(xs, ws, bs, stride)
            gx, gw_ = torch.autograd.grad(y, (xs, ws), dys)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        y = D.dense_conv3x3(xs, ws, bs, stride)
        gx, gw_ = torch.autograd.grad(y, (xs, ws), dys)
    for _ in range(2):
        y.zero_()
        gx.zero_()
        gw_.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(y.detach(), eager[0]) and torch.equal(gx, eager[1]) and torch.equal(gw_, eager[2])


@pytest.mark.parametrize("dtype_name", ["bf16", "f16"])
def test_bias_epilogue_is_one_rounding(dtype_name):
    """y(bias) == round(fp32(bias-free accumulator) + bias): with a bias-free output that is exact in 16 bit (small integers), the
    biased output equals the fp32 sum rounded once, bit for bit."""
    import torch
    from ssds.modeling.layers import denseconv as D

    dtype = torch.bfloat16 if dtype_name == "bf16" else torch.float16
    g = torch.Generator().manual_seed(5)
    x = torch.randint(-2, 3, (2, 32, 9, 12), generator=g).to(dtype)
    wt = torch.randint(-1, 2, (36, 32, 3, 3), generator=g).float()
    wt[:, 8:] = 0  # |y| <= 2 * 9 * 8 = 144: exact in bf16 and fp16
    b = torch.randn(36, generator=g)
    y0 = D.dense_conv3x3(x.cuda(), wt.cuda(), None, 1)
    y1 = D.dense_conv3x3(x.cuda(), wt.cuda(), b.cuda(), 1)
    ref = torch.nn.functional.conv2d(x.double(), wt.double(), None, 1, 1)
    assert torch.equal(y0.double().cpu(), ref), "the bias-free output is exact"
    want = (y0.float().cpu() + b.view(1, -1, 1, 1)).to(dtype)
    assert torch.equal(y1.cpu().view(torch.int16), want.view(torch.int16))


def test_shared_weight_on_three_maps_and_across_an_optimizer_step():
    """One DenseConv3x3 applied to three maps of different size in one forward (the shared towers): the accumulated weight gradient
    meets the dW bar against fp64.  Then a native SGD step (parameters updated through raw pointers): the next forward uses the
    updated weight -- no stale image survives."""
    import torch
    import torch.nn.functional as F
    from ssds.core import optimizer as O
    from ssds.modeling.layers import denseconv as D

    torch.manual_seed(3)
    dtype = torch.bfloat16
    m = D.DenseConv3x3(64, 36, 3, 1, 1, bias=True).cuda()
    with torch.no_grad():
        m.weight.copy_(m.weight.to(dtype).float())
    xs = [torch.randn(2, 64, s, s).to(dtype) for s in (20, 10, 5)]
    dys = [torch.randn(2, 36, s, s).to(dtype) for s in (20, 10, 5)]
    calls = dict(D.STATS)
    xd = [x.cuda().requires_grad_(True) for x in xs]
    ys = [m(x) for x in xd]
    torch.autograd.backward(ys, [d.cuda() for d in dys])
    torch.cuda.synchronize()
    assert [D.STATS[k] - calls[k] for k in ("native_forward", "native_dgrad", "native_wgrad")] == [3, 3, 3]
    w64 = m.weight.detach().double().cpu().requires_grad_(True)
    b64 = m.bias.detach().double().cpu().requires_grad_(True)
    x64 = [x.double().requires_grad_(True) for x in xs]
    y64 = [F.conv2d(x, w64, b64, 1, 1) for x in x64]
    torch.autograd.backward(y64, [d.double() for d in dys])
    _wgrad_bar(m.weight.grad, w64.grad, "dW accumulated over three maps")
    for got, want, x in zip(ys, y64, x64):
        _rounding_bar(got.detach(), want.detach(), 2.0 ** -8, "y shared %d" % x.shape[-1])
    for got, x in zip(xd, x64):
        _rounding_bar(got.grad, x.grad, 2.0 ** -8, "dx shared %d" % x.shape[-1])
    # a native optimizer step in between
    opt = O.SsdkSGD(list(m.parameters()), lr=0.5, momentum=0.0, weight_decay=0.0)
    w_before = m.weight.detach().clone()
    y_before = m(xd[0].detach()).detach().clone()
    opt.step()
    torch.cuda.synchronize()
    assert not torch.equal(m.weight.detach(), w_before), "the optimizer did not move the weight"
    y_after = m(xd[0].detach()).detach()
    want = F.conv2d(xs[0].double(), m.weight.detach().to(dtype).double().cpu(), m.bias.detach().double().cpu(), 1, 1)
    _rounding_bar(y_after, want, 2.0 ** -8, "y after the optimizer step")
    assert not torch.equal(y_after, y_before)


def _rel(a, b):
    return float((a.double().cpu() - b.double()).norm() / b.double().norm().clamp(min=1e-12))


def _block_run(block, x, native):
    """One train-mode forward + backward of ``block`` under bf16 autocast on the GPU -> {name: tensor} of the output and every
    parameter gradient.  ``native``: the dense 3x3 layers on the ssdk kernels, else left on nn.Conv2d (the PyTorch-ROCm floor)."""
    import copy

    import torch
    from ssds.modeling.layers import denseconv as D
    from ssds.modeling.layers.batchnorm import use_fast_batchnorm
    from ssds.modeling.layers.pointwise import use_pointwise_gemm

    m = copy.deepcopy(block).cuda().train()
    if native:
        use_fast_batchnorm(m)
        use_pointwise_gemm(m)
        D.use_native_dense3x3(m)
    xd = x.cuda().requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        y = m(xd)
    y.float().pow(2).mean().backward()
    torch.cuda.synchronize()
    out = {"output": y.detach().float(), "input.grad": xd.grad}
    out.update({k + ".grad": p.grad for k, p in m.named_parameters()})
    return out


@pytest.mark.parametrize("kind", ["resnet50_bottleneck_256_64", "fpn_shared_head_36"])
def test_one_block_in_train_mode(kind):
    """A ResNet50 Bottleneck(256, 64) and an SSDFPN SharedHead(36) in train mode, bf16 autocast, with use_fast_batchnorm +
    use_pointwise_gemm + use_native_dense3x3, against the fp32 CPU block: per tensor (output, input gradient, every parameter
    gradient) rel(native) <= 2 rel(floor) + 0.02, the floor being PyTorch-ROCm on the same bf16-autocast block with the layers left
    on nn.Conv2d (the rule of tests/test_gpu_gconv_train.py::test_one_block_in_train_mode)."""
    import copy

    import torch
    from ssds.modeling.layers import denseconv as D
    from ssds.modeling.nets.resnet import Bottleneck
    from ssds.modeling.ssds.fpn import SharedHead

    torch.manual_seed(5)
    if kind.startswith("resnet50"):
        block, cin, n3, size = Bottleneck(256, 64), 256, 1, 32
    else:
        block, cin, n3, size = SharedHead(36), 256, 5, 20
    x = torch.randn(4, cin, size, size)
    ref = copy.deepcopy(block).train()
    xr = x.clone().requires_grad_(True)
    yr = ref(xr)
    yr.pow(2).mean().backward()
    want = {"output": yr.detach(), "input.grad": xr.grad}
    want.update({k + ".grad": p.grad for k, p in ref.named_parameters()})
    calls = dict(D.STATS)
    got = _block_run(block, x, True)
    assert [D.STATS[k] - calls[k] for k in ("native_forward", "native_dgrad", "native_wgrad")] == [n3, n3, n3], "the native path did not run"
    floor = _block_run(block, x, False)
    assert set(got) == set(want) == set(floor)
    bad = []
    for k in sorted(want):
        rn, rf = _rel(got[k], want[k]), _rel(floor[k], want[k])
        print("%s %-28s rel native %.5f floor %.5f" % (kind, k, rn, rf))
        if not rn <= 2.0 * rf + 0.02:
            bad.append((k, rn, rf))
    assert not bad, bad


_SWITCH = r"""
import sys, torch
sys.path[:0] = [%(root)r, %(pkg)r]
import torch.nn as nn
from ssds.core import config
from ssds.utils import train_ddp
from ssds.modeling.layers import denseconv as D
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
dense = [m for m in net.modules() if isinstance(m, nn.Conv2d) and m.kernel_size == (3, 3) and m.groups == 1 and m.in_channels > 3]
shared = sum(4 for k, m in net.named_modules() if type(m) is D.DenseConv3x3 and (k.startswith("loc.") or k.startswith("conf.")))
print("RESULT", len(dense), sum(type(m) is D.DenseConv3x3 for m in dense), D.STATS["native_forward"], D.STATS["native_dgrad"],
      D.STATS["native_wgrad"], int(finite), len(grads), shared)
"""


@pytest.mark.parametrize("switch", ["0", "1"])
def test_the_switch(switch):
    """SSDK_DENSE3_TRAIN=0 in a subprocess: the Solver-built fpn_resnet50_640 model takes one train-mode forward + backward at batch 2,
    128 px, with finite gradients and zero native dense calls; =1: every dense 3x3 runs natively, forward and both gradients (the
    layers of the two shared towers once per level: five calls each)."""
    env = dict(os.environ, SSDK_DENSE3_TRAIN=switch)
    code = _SWITCH % dict(root=ROOT, pkg=os.path.join(ROOT, "ssds.pytorch_amd"),
                          cfg=os.path.join(ROOT, "experiments", "cfgs", "fpn_resnet50_640.yml"))
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    total, native, nf, nd, nw, finite, ngrads, shared = (int(v) for v in [l for l in out.stdout.splitlines() if l.startswith("RESULT")][-1].split()[1:])
    assert total > 0 and finite == 1 and ngrads > 0
    if switch == "0":
        assert (native, nf, nd, nw) == (0, 0, 0, 0)
    else:
        assert native == total
        assert nf == nw == total + shared and nd == total + shared  # every layer's input needs a gradient: none is image-side
