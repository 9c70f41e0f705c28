"""The neck operations of the training step (csrc/ssdk_necktrain.hip, ssds/modeling/layers/neckfuse.py), the parts that need no GPU:
the exported entry points and their argument checks (all made before any device call), what the explicit functions do with CPU
tensors, which modules ``use_native_neck`` switches on the four FPN / BiFPN configs, that a flagged model computes bit for bit
what the unflagged one does on the CPU, and the Solver's routing under SSDK_NECK_TRAIN."""
import copy
import os

import pytest

from solverhelp import run_solver_script

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW = ("ssdk_neck_fuse_fwd", "ssdk_neck_fuse_bwd_workspace_bytes", "ssdk_neck_fuse_bwd", "ssdk_maxpool3x3s2_train_fwd",
       "ssdk_maxpool3x3s2_train_bwd")
SAME, UP2, POOL2 = 0, 1, 2


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

    def fwd(a=F, b=F, c=None, w=None, ws=1, y=F, n=2, ch=8, h=6, wd=10, mb=SAME, hb=0, wb=0, mc=SAME, hc=0, wc=0, dt=BF16):
        return L.ssdk_neck_fuse_fwd(a, b, c, w, ws, y, n, ch, h, wd, mb, hb, wb, mc, hc, wc, dt, None)

    need = int(L.ssdk_neck_fuse_bwd_workspace_bytes(2, 8, 6, 10))
    assert need > 0 and need % 12 == 0

    def bwd(gy=F, a=F, b=F, c=None, nsrc=2, w=F, ws=1, ga=F, gb=F, gc=None, gw=F, cols=4, col=1, wk=F, nbytes=need, n=2, ch=8, h=6,
            wd=10, mb=SAME, hb=0, wb=0, mc=SAME, hc=0, wc=0, dt=BF16):
        return L.ssdk_neck_fuse_bwd(gy, a, b, c, nsrc, w, ws, ga, gb, gc, gw, cols, col, wk, nbytes, n, ch, h, wd, mb, hb, wb, mc, hc,
                                    wc, dt, None)

    def pfwd(x=F, y=F, n=2, ch=4, h=7, wd=9, dt=BF16):
        return L.ssdk_maxpool3x3s2_train_fwd(x, y, n, ch, h, wd, dt, None)

    def pbwd(x=F, gy=F, gx=F, n=2, ch=4, h=7, wd=9, dt=BF16):
        return L.ssdk_maxpool3x3s2_train_bwd(x, gy, gx, n, ch, h, wd, dt, None)

    fuse_bad = [
        dict(dt=0), dict(dt=3),                                          # dtype
        dict(n=0), dict(ch=0), dict(h=0), dict(wd=0), dict(n=-1),        # N, C, H, W < 1
        dict(mb=UP2, h=7), dict(mb=UP2, wd=9),                           # an odd H or W under UP2
        dict(mb=POOL2, hb=12, wb=19), dict(mb=POOL2, hb=14, wb=20), dict(mb=POOL2, hb=11, wb=20), dict(mb=POOL2),  # POOL2 dims
        dict(mb=3), dict(mb=-1),
    ]
    for fn, name in ((fwd, "neck_fuse_fwd"), (bwd, "neck_fuse_bwd")):
        for kw in fuse_bad:
            assert fn(**kw) == -1 and name in err(), (name, kw, err())
        # the same classes on the third source
        for kw in (dict(mc=UP2, h=7), dict(mc=POOL2, hc=12, wc=19), dict(mc=5)):
            extra = dict(c=F) if fn is fwd else dict(c=F, nsrc=3)
            assert fn(**dict(kw, **extra)) == -1 and name in err(), (name, kw, err())
    for kw in (dict(a=None), dict(b=None), dict(y=None), dict(a=F + 1), dict(y=F + 1), dict(w=F + 2), dict(w=F, ws=0)):
        assert fwd(**kw) == -1 and "neck_fuse_fwd" in err(), kw
    for kw in (dict(gy=None), dict(gy=F + 1), dict(gb=F + 1), dict(gw=F + 2), dict(w=F + 2), dict(ws=0), dict(nsrc=1), dict(nsrc=4),
               dict(w=None), dict(w=None, gw=None), dict(a=None), dict(b=None), dict(nsrc=3), dict(c=F), dict(gc=F),
               dict(gw=None, ga=None, gb=F, b=None, mb=POOL2, hb=12, wb=20),
               dict(wk=None), dict(wk=F + 2), dict(nbytes=need - 1), dict(nbytes=0), dict(col=4), dict(col=-1), dict(cols=0)):
        assert bwd(**kw) == -1 and "neck_fuse_bwd" in err(), kw
    for fn, name in ((pfwd, "maxpool3x3s2_train_fwd"), (pbwd, "maxpool3x3s2_train_bwd")):
        for kw in (dict(dt=0), dict(n=0), dict(ch=0), dict(h=0), dict(wd=0), dict(ch=-3), dict(x=None), dict(x=F + 1)):
            assert fn(**kw) == -1 and name in err(), (name, kw, err())
    assert pfwd(y=None) == -1 and pbwd(gy=None) == -1 and pbwd(gx=None) == -1 and pbwd(gx=F + 1) == -1
    # the workspace query answers 0 for a shape the kernels do not take, and never more than 4096 partial triples
    assert L.ssdk_neck_fuse_bwd_workspace_bytes(0, 8, 6, 10) == 0 and L.ssdk_neck_fuse_bwd_workspace_bytes(2, 8, 6, 0) == 0
    assert L.ssdk_neck_fuse_bwd_workspace_bytes(1 << 15, 1 << 10, 8, 8) == 0  # 2^31 elements
    assert L.ssdk_neck_fuse_bwd_workspace_bytes(16, 256, 112, 112) == 4096 * 12


def test_weight_gradient_depth_constant():
    from ssds.modeling.layers import neckfuse as NF

    assert 0 < NF.WSUM_DEPTH <= 512


def test_cpu_tensors_raise_in_the_explicit_functions_and_fall_back_in_the_module():
    import torch
    import torch.nn as nn
    from ssds.modeling.layers import neckfuse as NF

    torch.manual_seed(0)
    a, b = torch.randn(1, 2, 4, 4).bfloat16(), torch.randn(1, 2, 2, 2).bfloat16()
    with pytest.raises(ValueError):
        NF.neck_fuse(a, b, mode_b=NF.UP2)
    with pytest.raises(ValueError):
        NF.neck_fuse(a.float(), b.float(), weights=torch.ones(2, 3), col=1, mode_b=NF.UP2)
    with pytest.raises(ValueError):
        NF.maxpool3x3s2(a)
    assert NF.try_fuse(a, b, mode_b=NF.UP2) is None
    calls = dict(NF.STATS)
    for dtype in (torch.float32, torch.bfloat16):
        x = torch.relu(torch.randn(2, 3, 9, 7)).to(dtype)
        m, ref = NF.TrainMaxPool3x3s2(3, 2, 1), nn.MaxPool2d(3, 2, 1)
        assert repr(m).replace("TrainMaxPool3x3s2", "MaxPool2d") == repr(ref)
        xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
        ya, yb = m(xa), ref(xb)
        g = torch.randn_like(yb)
        ya.backward(g)
        yb.backward(g)
        assert torch.equal(ya, yb) and torch.equal(xa.grad, xb.grad)
    assert NF.STATS == calls


CFGS = {"fpn_resnet50_640.yml": (0, 1, 1), "fpn_resnext50_640.yml": (0, 1, 1), "bifpn_regnetx008_896.yml": (None, 0, 0),
        "bifpn_regnetx016_896.yml": (None, 0, 0)}


@pytest.mark.parametrize("cfg_name", sorted(CFGS))
def test_use_native_neck_switches_exactly_the_neck_modules(cfg_name):
    import torch.nn as nn
    from ssds.core import config
    from ssds.modeling import model_builder
    from ssds.modeling.layers import neckfuse as NF
    from ssds.modeling.ssds.bifpn import BiFPNModule
    from ssds.modeling.ssds.fpn import SSDFPN

    cfg = config.cfg_from_file(os.path.join(ROOT, "experiments", "cfgs", cfg_name))
    model = model_builder.create_model(cfg.MODEL)
    keys = list(model.state_dict().keys())
    classes = [type(m) for m in model.modules()]
    bifpn = [m for m in model.modules() if isinstance(m, BiFPNModule)]
    pools = [k for k, m in model.named_modules() if isinstance(m, nn.MaxPool2d)]
    want_bifpn, want_fpn, want_pool = CFGS[cfg_name]
    if want_bifpn is None:
        want_bifpn = len(bifpn)
        assert want_bifpn >= 1
    assert len(bifpn) == want_bifpn and int(isinstance(model, SSDFPN)) == want_fpn and len(pools) == want_pool
    assert not any(getattr(m, "native_neck", False) for m in model.modules())
    before = dict(NF.STATS)
    assert NF.use_native_neck(model) is model
    delta = {k: NF.STATS[k] - before[k] for k in before}
    want = {k: 0 for k in before}
    want.update(bifpn_modules=want_bifpn, fpn_models=want_fpn, maxpools=want_pool)
    assert delta == want
    assert all(m.native_neck for m in bifpn) and getattr(model, "native_neck", False) == bool(want_fpn)
    flagged = [m for m in model.modules() if getattr(m, "native_neck", False)]
    assert len(flagged) == want_bifpn + want_fpn
    after = [type(m) for m in model.modules()]
    changed = [(a, b) for a, b in zip(classes, after) if a is not b]
    assert changed == [(nn.MaxPool2d, NF.TrainMaxPool3x3s2)] * want_pool
    if want_pool:
        assert pools == ["backbone.maxpool"] and type(model.backbone.maxpool) is NF.TrainMaxPool3x3s2
    assert list(model.state_dict().keys()) == keys
    NF.use_native_neck(model)  # a second call switches nothing more
    assert {k: NF.STATS[k] - before[k] for k in before} == delta


def test_use_native_neck_leaves_other_pools_alone():
    import torch.nn as nn
    from ssds.modeling.layers import neckfuse as NF
    from ssds.modeling.nets.resnet import ResNet18

    for pool in (nn.MaxPool2d(3, 2, 1, ceil_mode=True), nn.MaxPool2d(2, 2), nn.MaxPool2d(3, 2, 1, return_indices=True),
                 nn.MaxPool2d(3, 2, 1, dilation=2), nn.MaxPool2d(3, 1, 1)):
        net = ResNet18([3, 4, 5])
        net.maxpool = pool
        before = NF.STATS["maxpools"]
        NF.use_native_neck(net)
        assert type(net.maxpool) is nn.MaxPool2d and NF.STATS["maxpools"] == before
    net = ResNet18([3, 4, 5])
    NF.use_native_neck(net)
    assert type(net.maxpool) is NF.TrainMaxPool3x3s2


class _StubBackbone(object):
    """Three maps of 8 / 12 / 16 channels at 16 / 8 / 4 pixels from a 3-channel image (strided 1x1 convolutions)."""

    @staticmethod
    def build():
        import torch.nn as nn

        class Stub(nn.Module):
            def __init__(self):
                super(Stub, self).__init__()
                self.c = nn.ModuleList([nn.Conv2d(3, ch, 1, stride=s) for ch, s in ((8, 2), (12, 4), (16, 8))])

            def initialize(self):
                return None

            def forward(self, x):
                return [c(x) for c in self.c]

        return Stub()


def _small_model(kind):
    from ssds.modeling.ssds.bifpn import SSDBiFPN
    from ssds.modeling.ssds.fpn import SSDFPN

    cls = SSDBiFPN if kind == "bifpn" else SSDFPN
    layers = [[0, 1, 2, "Conv:S"], [8, 12, 16, 16]] + ([2] if kind == "bifpn" else [])
    _, extras, head = cls.add_extras(layers, [2, 2, 2, 2], 3)
    return cls(_StubBackbone.build(), extras, head, 3)


@pytest.mark.parametrize("kind", ["bifpn", "fpn"])
def test_flagged_model_equals_the_unflagged_one_on_cpu(kind):
    """fp32 on the CPU, train mode: forward outputs and every parameter gradient bit for bit."""
    import torch
    from ssds.modeling.layers import neckfuse as NF

    torch.manual_seed(3)
    ref = _small_model(kind).train()
    with torch.no_grad():
        for k, p in ref.named_parameters():
            if k.endswith(".w1") or k.endswith(".w2"):
                p.copy_(torch.rand_like(p) + 0.1)
    flagged = NF.use_native_neck(copy.deepcopy(ref))
    assert any(getattr(m, "native_neck", False) for m in flagged.modules())
    assert not any(getattr(m, "native_neck", False) for m in ref.modules())
    x = torch.randn(2, 3, 32, 32)
    calls = dict(NF.STATS)
    outs = []
    for m in (ref, flagged):
        loc, conf = m(x)
        sum((t * t).mean() for t in loc + conf).backward()
        outs.append((loc + conf, {k: p.grad for k, p in m.named_parameters()}))
    (ya, ga), (yb, gb) = outs
    assert len(ya) == len(yb) == 8 and all(torch.equal(u, v) for u, v in zip(ya, yb))
    assert list(ga) == list(gb) and all(g is not None for g in ga.values())
    assert all(torch.equal(ga[k], gb[k]) for k in ga), [k for k in ga if not torch.equal(ga[k], gb[k])]
    assert {k: NF.STATS[k] for k in calls if k.startswith(("fuse_", "pool_"))} == {k: calls[k] for k in calls if k.startswith(("fuse_", "pool_"))}


_SOLVER = r"""
import torch.nn as nn
from ssds.core import config
from ssds.utils import train_ddp
from ssds.modeling.layers import neckfuse as NF
from ssds.modeling.ssds.bifpn import BiFPNModule
from ssds.modeling.ssds.fpn import SSDFPN
cfg = config.cfg_from_file(%(cfg)r)
s = train_ddp.Solver(cfg, 0, torch.device("cpu"))
mods = list(s.model.modules())
bifpn = [m for m in mods if isinstance(m, BiFPNModule)]
pools = [m for m in mods if isinstance(m, nn.MaxPool2d)]
print("RESULT", len(bifpn), sum(m.native_neck for m in bifpn), int(isinstance(s.model, SSDFPN)), int(getattr(s.model, "native_neck", False)),
      len(pools), sum(type(m) is NF.TrainMaxPool3x3s2 for m in pools), sum(bool(getattr(m, "native_neck", False)) for m in mods),
      NF.STATS["bifpn_modules"], NF.STATS["fpn_models"], NF.STATS["maxpools"])
"""


def _solver(cfg_name, switch):
    return run_solver_script(_SOLVER, cfg_name, env={"SSDK_NECK_TRAIN": switch})


@pytest.mark.parametrize("cfg_name", ["fpn_resnet50_640.yml", "bifpn_regnetx008_896.yml"])
@pytest.mark.parametrize("switch", [None, "1", "0"])
def test_solver_routing(cfg_name, switch):
    """train_ddp.Solver enables the neck kernels on the FPN / BiFPN configs unless SSDK_NECK_TRAIN=0 (read when the Solver is built; a
    subprocess per value); with 0 nothing is flagged or swapped."""
    nbifpn, bifpn_on, is_fpn, fpn_on, npools, pools_on, flagged, s_bifpn, s_fpn, s_pool = _solver(cfg_name, switch)
    assert nbifpn + is_fpn >= 1 and npools == is_fpn
    if switch == "0":
        assert (bifpn_on, fpn_on, pools_on, flagged, s_bifpn, s_fpn, s_pool) == (0, 0, 0, 0, 0, 0, 0)
    else:
        assert bifpn_on == nbifpn == s_bifpn and fpn_on == is_fpn == s_fpn and pools_on == npools == s_pool
        assert flagged == nbifpn + is_fpn


@pytest.mark.parametrize("switch", [None, "1", "0"])
def test_solver_leaves_ssd_models_alone(switch):
    res = _solver("ssd_mobilenetv2_512.yml", switch)
    assert res == [0] * 10
