"""Grouped 3x3 convolutions of the training step (csrc/ssdk_gconvtrain.hip, ssds/modeling/layers/groupedconv.py), the parts
that need no GPU: the layout of the input-gradient weights, which layers of the registered backbones ``use_native_gconv``
swaps, the argument checks of the C entry points, and the Solver's switch."""
import os

import pytest

from solverhelp import run_solver_script

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _registered():
    from ssds.modeling import nets

    return sorted(n for n in dir(nets) if n.startswith("RegNetX") or n.startswith("ResNeXt"))


@pytest.mark.parametrize("gw,groups", [(4, 6), (8, 3), (16, 2), (24, 2), (40, 2)])
def test_pack_grouped_frag_dgrad_is_the_input_gradient_layout(gw, groups):
    """At stride 1 the input gradient of the grouped layer IS the grouped convolution of dy with the weights the
    input-gradient image holds (per group transposed, taps flipped; 4-wide groups as block-diagonal pairs): fp64, 1e-12."""
    import torch
    import torch.nn.functional as F
    from ssds.modeling.layers import groupedconv as G

    torch.manual_seed(gw)
    c = gw * groups
    w = torch.randn(c, gw, 3, 3, dtype=torch.float64)
    x = torch.randn(2, c, 9, 7, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(x, w, None, 1, 1, 1, groups)
    dy = torch.randn_like(y)
    y.backward(dy)
    img, g2, gw2 = G.pack_grouped_frag_dgrad(w.permute(0, 2, 3, 1).contiguous(), groups)  # KRSC in
    assert (g2, gw2) == ((groups // 2, 8) if gw == 4 else (groups, gw))
    assert tuple(img.shape) == (g2 * ((gw2 + 15) // 16), (9 * gw2 + 31) // 32, 4, 16, 8)
    wd = G.unpack_grouped_frag(img, g2, gw2)
    dx = F.conv2d(dy, wd, None, 1, 1, 1, g2)
    assert float((dx - x.grad).abs().max()) <= 1e-12
    # and the forward image, read back the same way, is the layer itself
    from ssds.modeling.layers.fused_conv import pack_grouped_frag

    fimg, _, _ = pack_grouped_frag(w.permute(0, 2, 3, 1).contiguous(), groups)
    assert float((F.conv2d(x.detach(), G.unpack_grouped_frag(fimg, g2, gw2), None, 1, 1, 1, g2) - y.detach()).abs().max()) <= 1e-12


@pytest.mark.parametrize("name", _registered())
def test_use_native_gconv_swaps_every_grouped_3x3_of_the_registered_backbones(name):
    import torch
    import torch.nn as nn
    from ssds.modeling import nets
    from ssds.modeling.layers import groupedconv as G

    with torch.device("meta"):
        net = getattr(nets, name)(outputs=[4] if name.startswith("RegNet") else [5])
    before = {k: type(m) for k, m in net.named_modules()}
    keys = list(net.state_dict().keys())
    swapped0 = G.STATS["swapped"]
    assert G.use_native_gconv(net) is net
    n_grouped = 0
    for k, m in net.named_modules():
        if not isinstance(m, nn.Conv2d):
            assert type(m) is before[k]
            continue
        grouped3 = m.kernel_size == (3, 3) and 1 < m.groups < m.in_channels
        if grouped3:
            n_grouped += 1
            assert type(m) is G.GroupedConv3x3, "%s.%s stayed %s" % (name, k, type(m).__name__)
        else:  # dense, depthwise, 1x1, the 7x7 stem
            assert type(m) is nn.Conv2d, (k, type(m))
    assert n_grouped > 0 and G.STATS["swapped"] == swapped0 + n_grouped
    assert list(net.state_dict().keys()) == keys


def test_swapped_module_is_nn_conv2d_on_the_cpu_and_other_layers_are_untouched():
    import torch
    import torch.nn as nn
    from ssds.modeling.layers import groupedconv as G

    torch.manual_seed(0)
    model = nn.Sequential(
        nn.Conv2d(48, 48, 3, 2, 1, groups=2, bias=False),   # 24 wide: swapped
        nn.Conv2d(48, 48, 3, 1, 1, bias=False),             # dense
        nn.Conv2d(48, 48, 3, 1, 1, groups=48, bias=False),  # depthwise
        nn.Conv2d(48, 48, 1, 1, 0, groups=2, bias=False),   # grouped 1x1
        nn.Conv2d(60, 60, 3, 1, 1, groups=5, bias=False),   # 12 wide: not supported
        nn.Conv2d(12, 12, 3, 1, 1, groups=3, bias=False),   # 4 wide, odd number of groups
        nn.Conv2d(48, 48, 3, 1, 2, dilation=2, groups=2),   # dilated
        nn.Conv2d(48, 96, 3, 1, 1, groups=2),               # Cin != Cout
        nn.Conv2d(64, 64, 3, 1, 1, groups=4, bias=True),    # 16 wide, with a bias: swapped
    )
    ref = [nn.Conv2d(48, 48, 3, 2, 1, groups=2, bias=False), nn.Conv2d(64, 64, 3, 1, 1, groups=4, bias=True)]
    ref[0].load_state_dict(model[0].state_dict())
    ref[1].load_state_dict(model[8].state_dict())
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    G.use_native_gconv(model)
    assert [type(m) is G.GroupedConv3x3 for m in model] == [True] + [False] * 7 + [True]
    assert all(type(m) is nn.Conv2d for m in list(model)[1:8])
    got = model.state_dict()
    assert list(got.keys()) == list(sd.keys()) and all(torch.equal(got[k], sd[k]) for k in sd)
    for m, r, c in ((model[0], ref[0], 48), (model[8], ref[1], 64)):
        x = torch.randn(2, c, 9, 7)
        xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
        ya, yb = m(xa), r(xb)
        g = torch.randn_like(yb)
        ya.backward(g)
        yb.backward(g)
        assert torch.equal(ya, yb) and torch.equal(xa.grad, xb.grad) and torch.equal(m.weight.grad, r.weight.grad)
        if r.bias is not None:
            assert torch.equal(m.bias.grad, r.bias.grad)


NEW = ("ssdk_gconv3x3_train_prepare", "ssdk_gconv3x3_train_forward", "ssdk_gconv3x3_train_dgrad",
       "ssdk_gconv3x3_train_wgrad_workspace_bytes", "ssdk_gconv3x3_train_wgrad")


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

    def prepare(w=F, a=F, b=F, c=48, groups=2, dt=BF16):
        return L.ssdk_gconv3x3_train_prepare(w, a, b, c, groups, dt, None)

    def forward(x=F, w=F, y=F, n=2, c=48, h=8, wd=8, groups=2, stride=1, dt=BF16):
        return L.ssdk_gconv3x3_train_forward(x, w, y, n, c, h, wd, groups, stride, dt, None)

    def dgrad(dy=F, w=F, dx=F, n=2, c=48, h=8, wd=8, groups=2, stride=1, dt=BF16):
        return L.ssdk_gconv3x3_train_dgrad(dy, w, dx, n, c, h, wd, groups, stride, dt, None)

    need = int(L.ssdk_gconv3x3_train_wgrad_workspace_bytes(2, 48, 8, 8, 2, 1))
    assert need > 0 and need % (9 * 256 * 4) == 0

    def wgrad(x=F, dy=F, dw=F, ws=F, nbytes=need, n=2, c=48, h=8, wd=8, groups=2, stride=1, dt=BF16):
        return L.ssdk_gconv3x3_train_wgrad(x, dy, dw, ws, nbytes, n, c, h, wd, groups, stride, dt, None)

    bad_shapes = [dict(c=50), dict(c=60, groups=5), dict(c=12, groups=3), dict(c=528, groups=2), dict(c=0), dict(groups=0), dict(dt=0)]
    for fn, name in ((prepare, "prepare"), (forward, "forward"), (dgrad, "dgrad"), (wgrad, "wgrad")):
        for kw in bad_shapes:  # C % groups, 12 wide, 4 wide with an odd number of groups, 264 wide, no channels / groups, fp32
            assert fn(**kw) == -1, (name, kw)
            assert ("gconv3x3_train_" + name) in err(), (name, kw, err())
    for fn, name in ((forward, "forward"), (dgrad, "dgrad"), (wgrad, "wgrad")):
        for kw in (dict(stride=3), dict(stride=0), dict(n=0), dict(h=0), dict(wd=0)):
            assert fn(**kw) == -1 and ("gconv3x3_train_" + name) in err(), (name, kw)
    for kw in (dict(w=None), dict(a=None, b=None), dict(a=F + 2)):
        assert prepare(**kw) == -1 and "gconv3x3_train_prepare" in err(), kw
    for kw in (dict(x=None), dict(w=None), dict(y=None), dict(w=F + 8)):
        assert forward(**kw) == -1 and "gconv3x3_train_forward" in err(), kw
    for kw in (dict(dy=None), dict(w=None), dict(dx=None)):
        assert dgrad(**kw) == -1 and "gconv3x3_train_dgrad" in err(), kw
    for kw in (dict(x=None), dict(dy=None), dict(dw=None), dict(ws=None), dict(nbytes=need - 1), dict(nbytes=0), dict(ws=F + 4)):
        assert wgrad(**kw) == -1 and "gconv3x3_train_wgrad" in err(), kw
    # the workspace query answers 0 for a shape the kernels do not take
    assert L.ssdk_gconv3x3_train_wgrad_workspace_bytes(2, 60, 8, 8, 5, 1) == 0
    assert L.ssdk_gconv3x3_train_wgrad_workspace_bytes(2, 48, 8, 8, 2, 3) == 0
    # merged 4-wide groups: the same tiles as the 8-wide layer of half the groups
    assert L.ssdk_gconv3x3_train_wgrad_workspace_bytes(2, 64, 8, 8, 16, 1) == L.ssdk_gconv3x3_train_wgrad_workspace_bytes(2, 64, 8, 8, 8, 1)


_SOLVER = r"""
from ssds.core import config
from ssds.utils import train_ddp
from ssds.modeling.layers import groupedconv as G
import torch.nn as nn
cfg = config.cfg_from_file(%(cfg)r)
s = train_ddp.Solver(cfg, 0, torch.device("cpu"))
grouped = [m for m in s.model.modules() if isinstance(m, nn.Conv2d) and m.kernel_size == (3, 3) and 1 < m.groups < m.in_channels]
print("RESULT", len(grouped), sum(type(m) is G.GroupedConv3x3 for m in grouped), G.STATS["swapped"])
"""


@pytest.mark.parametrize("cfg_name", ["bifpn_regnetx016_896.yml", "fpn_resnext50_640.yml"])
@pytest.mark.parametrize("switch", [None, "1", "0"])
def test_solver_switch(cfg_name, switch):
    """train_ddp.Solver routes the grouped layers of the two grouped configs natively unless SSDK_GCONV_TRAIN=0 (read when the
    Solver is built; a subprocess per value)."""
    total, native, swapped = run_solver_script(_SOLVER, cfg_name, env={"SSDK_GCONV_TRAIN": switch})
    assert total > 0
    if switch == "0":
        assert native == 0 and swapped == 0
    else:
        assert native == total == swapped
