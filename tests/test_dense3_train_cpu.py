"""Dense 3x3 convolutions of the training step (csrc/ssdk_conv3train.hip, ssds/modeling/layers/denseconv.py), the parts that need
no GPU: the exported entry points and their argument checks, the layout of the two weight images, which layers
``use_native_dense3x3`` swaps, and the Solver's routing under SSDK_DENSE3_TRAIN."""
import os

import pytest

from solverhelp import run_solver_script

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW = ("ssdk_conv3x3_train_prepare", "ssdk_conv3x3_train_forward", "ssdk_conv3x3_train_dgrad",
       "ssdk_conv3x3_train_wgrad_workspace_bytes", "ssdk_conv3x3_train_wgrad")


def test_c_entry_points_are_exported_and_refuse_bad_arguments():
    from ssds import _native as N

    header = open(os.path.join(ROOT, "include", "ssdk.h")).read()
    for name in NEW:
        assert name in N.EXPORTS and (name + "(") in header and hasattr(N.lib, name), name
    assert N.lib.ssdk_version() == 245 and N.ABI_VERSION == 245
    L = N.lib
    F = 0x1000  # never dereferenced: every call below fails validation first
    BF16 = N.BF16
    err = lambda: L.ssdk_last_error().decode()  # noqa: E731

    def prepare(w=F, a=F, b=F, cin=64, cout=36, dt=BF16):
        return L.ssdk_conv3x3_train_prepare(w, a, b, cin, cout, dt, None)

    def forward(x=F, w=F, bias=None, y=F, n=2, cin=64, cout=36, h=8, wd=8, stride=1, dt=BF16):
        return L.ssdk_conv3x3_train_forward(x, w, bias, y, n, cin, cout, h, wd, stride, dt, None)

    def dgrad(dy=F, w=F, dx=F, n=2, cin=64, cout=36, h=8, wd=8, stride=1, dt=BF16):
        return L.ssdk_conv3x3_train_dgrad(dy, w, dx, n, cin, cout, h, wd, stride, dt, None)

    need = int(L.ssdk_conv3x3_train_wgrad_workspace_bytes(2, 64, 36, 8, 8, 1))
    assert need > 0 and need % (9 * 64 * 64 * 4) == 0

    def wgrad(x=F, dy=F, dw=F, ws=F, nbytes=need, n=2, cin=64, cout=36, h=8, wd=8, stride=1, dt=BF16):
        return L.ssdk_conv3x3_train_wgrad(x, dy, dw, ws, nbytes, n, cin, cout, h, wd, stride, dt, None)

    # Cin not a multiple of 16, below 16, above 4096; Cout not a multiple of 4, below 4, above 4096; fp32
    bad_shapes = [dict(cin=24), dict(cin=8), dict(cin=0), dict(cin=4112), dict(cout=6), dict(cout=0), dict(cout=4100), dict(dt=0)]
    for fn, name in ((prepare, "prepare"), (forward, "forward"), (dgrad, "dgrad"), (wgrad, "wgrad")):
        for kw in bad_shapes:
            assert fn(**kw) == -1, (name, kw)
            assert ("conv3x3_train_" + name) in err() and "gconv3x3" not in err(), (name, kw, err())
    for fn, name in ((forward, "forward"), (dgrad, "dgrad"), (wgrad, "wgrad")):
        for kw in (dict(stride=3), dict(stride=0), dict(n=0), dict(h=0), dict(wd=0), dict(n=-1)):
            assert fn(**kw) == -1 and ("conv3x3_train_" + name) in err(), (name, kw)
    for kw in (dict(w=None), dict(a=None, b=None), dict(a=F + 2), dict(b=F + 8), dict(w=F + 2)):
        assert prepare(**kw) == -1 and "conv3x3_train_prepare" in err(), kw
    for kw in (dict(x=None), dict(w=None), dict(y=None), dict(w=F + 8), dict(x=F + 1), dict(y=F + 1), dict(bias=F + 2)):
        assert forward(**kw) == -1 and "conv3x3_train_forward" in err(), kw
    for kw in (dict(dy=None), dict(w=None), dict(dx=None), dict(w=F + 8), dict(dy=F + 1), dict(dx=F + 1)):
        assert dgrad(**kw) == -1 and "conv3x3_train_dgrad" in err(), kw
    for kw in (dict(x=None), dict(dy=None), dict(dw=None), dict(ws=None), dict(nbytes=need - 1), dict(nbytes=0), dict(ws=F + 4),
               dict(dw=F + 2), dict(x=F + 1)):
        assert wgrad(**kw) == -1 and "conv3x3_train_wgrad" in err(), kw
    # the workspace query answers 0 for a shape the kernels do not take
    assert L.ssdk_conv3x3_train_wgrad_workspace_bytes(2, 24, 36, 8, 8, 1) == 0
    assert L.ssdk_conv3x3_train_wgrad_workspace_bytes(2, 64, 6, 8, 8, 1) == 0
    assert L.ssdk_conv3x3_train_wgrad_workspace_bytes(2, 64, 36, 8, 8, 3) == 0
    assert L.ssdk_conv3x3_train_wgrad_workspace_bytes(0, 64, 36, 8, 8, 1) == 0


@pytest.mark.parametrize("cin,cout", [(64, 64), (256, 36), (912, 256), (16, 4)])
def test_torch_twin_packers_are_a_permutation_with_zero_padding(cin, cout):
    import torch
    import torch.nn.functional as F
    from ssds.modeling.layers import denseconv as D

    torch.manual_seed(cin + cout)
    w = torch.randn(cout, cin, 3, 3, dtype=torch.float64)
    w[w == 0] = 1.0
    fwd, dg = D.pack_dense_frag(w), D.pack_dense_frag_dgrad(w)
    for img, rows, ch in ((fwd, cout, cin), (dg, cin, cout)):
        rb, ks, cp = D.image_shape(rows, ch)
        assert tuple(img.shape) == (rb, ks, 4, 16, 8) and rb == (rows + 15) // 16 and ks == (9 * cp + 31) // 32 and cp % 16 == 0
        # a pure permutation + zero padding: the non-zero elements are exactly the weight's, each once
        nz = img[img != 0]
        assert nz.numel() == w.numel() and torch.equal(nz.sort().values, w.reshape(-1).sort().values)
    # reading the images backwards returns the weights
    assert torch.equal(D.unpack_dense_frag(fwd, cout, cin), w)
    wd = D.unpack_dense_frag(dg, cin, cout)
    assert torch.equal(wd, w.flip(2, 3).transpose(0, 1))
    assert torch.equal(dg, D.pack_dense_frag(w.flip(2, 3).transpose(0, 1).contiguous()))
    # the image definition of include/ssdk.h, element by element on a sample
    rb, ks, cp = D.image_shape(cout, cin)
    g = torch.Generator().manual_seed(1)
    for _ in range(200):
        r, k = int(torch.randint(0, rb * 16, (1,), generator=g)), int(torch.randint(0, ks * 32, (1,), generator=g))
        tap, c = k // cp, k % cp
        want = float(w[r, c, tap // 3, tap % 3]) if (r < cout and tap < 9 and c < cin) else 0.0
        assert float(fwd[r // 16, k // 32, (k % 32) // 8, r % 16, k % 8]) == want
    # and the input-gradient image holds the weights of the stride-1 input gradient
    x = torch.randn(2, cin, 6, 5, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(x, w, None, 1, 1)
    dy = torch.randn_like(y)
    y.backward(dy)
    assert float((F.conv2d(dy, wd, None, 1, 1) - x.grad).abs().max()) <= 1e-10 * max(1.0, float(x.grad.abs().max()))


def test_use_native_dense3x3_swaps_exactly_the_supported_layers():
    import torch
    import torch.nn as nn
    from ssds.modeling.layers import denseconv as D

    torch.manual_seed(0)
    model = nn.Sequential(
        nn.Conv2d(64, 64, 3, 1, 1, bias=False),                         # dense: swapped
        nn.Conv2d(64, 36, 3, 1, 1, bias=True),                          # dense, Cout = 36, bias: swapped
        nn.Conv2d(48, 64, 3, 2, 1, bias=False),                         # dense, stride 2: swapped
        nn.Conv2d(64, 64, 3, 1, 1, groups=4, bias=False),               # grouped
        nn.Conv2d(64, 64, 3, 1, 1, groups=64, bias=False),              # depthwise
        nn.Conv2d(64, 64, 3, 1, 2, dilation=2, bias=False),             # dilated
        nn.Conv2d(64, 64, 1, 1, 0, bias=False),                         # 1x1
        nn.Conv2d(24, 64, 3, 1, 1, bias=False),                         # Cin = 24
        nn.Conv2d(64, 64, 3, 1, 1, padding_mode="reflect", bias=False),  # reflect padding
        nn.Conv2d(64, 6, 3, 1, 1, bias=False),                          # Cout = 6
    )
    want = [True, True, True] + [False] * 7
    assert [D.supported(m) for m in model] == want
    refs = {}
    for i in (0, 1, 2):
        m = model[i]
        refs[i] = nn.Conv2d(m.in_channels, m.out_channels, 3, m.stride, 1, bias=m.bias is not None)
        refs[i].load_state_dict(m.state_dict())
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    before = D.STATS["swapped"]
    assert D.use_native_dense3x3(model) is model
    assert [type(m) is D.DenseConv3x3 for m in model] == want and D.STATS["swapped"] == before + 3
    assert all(type(m) is nn.Conv2d for m in list(model)[3:])
    got = model.state_dict()
    assert list(got.keys()) == list(sd.keys()) and all(torch.equal(got[k], sd[k]) for k in sd)
    for i, r in refs.items():
        m = model[i]
        x = torch.randn(2, m.in_channels, 9, 7)
        xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
        ya, yb = m(xa), r(xb)
        g = torch.randn_like(yb)
        ya.backward(g)
        yb.backward(g)
        assert torch.equal(ya, yb) and torch.equal(xa.grad, xb.grad) and torch.equal(m.weight.grad, r.weight.grad)
        if r.bias is not None:
            assert torch.equal(m.bias.grad, r.bias.grad)


_SOLVER = r"""
from ssds.core import config
from ssds.utils import train_ddp
from ssds.modeling.layers import denseconv as D
from ssds.modeling.layers import pointwise as P
import torch.nn as nn
cfg = config.cfg_from_file(%(cfg)r)
s = train_ddp.Solver(cfg, 0, torch.device("cpu"))
# (the 3-channel image stem of RegNetX is not one of them: it has its own kernels, pointwise.StemConv3x3s2)
dense = [(k, m) for k, m in s.model.named_modules()
         if isinstance(m, nn.Conv2d) and m.kernel_size == (3, 3) and m.groups == 1 and m.in_channels > 3]
native = sum(type(m) is D.DenseConv3x3 for _, m in dense)
anywhere = sum(type(m) is D.DenseConv3x3 for m in s.model.modules())
im2col_extras = sum(type(m) is P.NativeConv3x3 and k.startswith("extras.") for k, m in dense)
im2col_other = sum(type(m) is P.NativeConv3x3 and not k.startswith("extras.") for k, m in dense)
plain = sum(type(m) is nn.Conv2d for _, m in dense)
n_extras = sum(k.startswith("extras.") for k, _ in dense)
print("RESULT", len(dense), native, anywhere, im2col_extras, im2col_other, plain, n_extras, D.STATS["swapped"])
"""


def _solver(cfg_name, switch):
    return run_solver_script(_SOLVER, cfg_name, env={"SSDK_DENSE3_TRAIN": switch})


@pytest.mark.parametrize("cfg_name", ["fpn_resnet50_640.yml", "fpn_resnext50_640.yml", "bifpn_regnetx016_896.yml"])
@pytest.mark.parametrize("switch", [None, "1", "0"])
def test_solver_routing(cfg_name, switch):
    """train_ddp.Solver routes every dense 3x3 of the FPN / BiFPN configs to DenseConv3x3 unless SSDK_DENSE3_TRAIN=0 (read when the
    Solver is built; a subprocess per value); with 0 the classes are the earlier routing's: NativeConv3x3 (im2col) under ``extras``,
    nn.Conv2d elsewhere."""
    total, native, anywhere, im2col_extras, im2col_other, plain, n_extras, swapped = _solver(cfg_name, switch)
    assert total > 0
    if switch == "0":
        assert native == 0 and anywhere == 0 and swapped == 0
        assert im2col_extras == n_extras and im2col_other == 0 and plain == total - n_extras
    else:
        assert native == total == swapped == anywhere and im2col_extras == 0 and im2col_other == 0 and plain == 0


@pytest.mark.parametrize("switch", [None, "1", "0"])
def test_solver_leaves_ssd_models_alone(switch):
    total, native, anywhere, _, _, _, _, swapped = _solver("ssd_mobilenetv2_512.yml", switch)
    assert native == 0 and anywhere == 0 and swapped == 0
