"""The YOLO-only operations of the training step (csrc/ssdk_cattrain.hip, include/ssdk_cattrain.h, ssds/modeling/layers/cattrain.py), the
parts that need no GPU: the header and its bound entry points, their argument checks (all made before any device call), what the
explicit functions do with CPU tensors, which modules ``use_native_cat`` flags, that a flagged model computes bit for bit what the
unflagged one does on the CPU, and the Solver's routing of the two shipped YOLO configs."""
import copy
import os

import pytest

from solverhelp import run_solver_script

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ssdk_cat_train_fwd", "ssdk_cat_train_bwd", "ssdk_spp_train_fwd", "ssdk_spp_train_bwd")
SAME, UP2 = 0, 1


def test_header_parses_and_every_symbol_is_bound():
    from ssds import _native as N

    with open(os.path.join(ROOT, "include", "ssdk_cattrain.h")) as f:
        h = N.parse_header(f.read())
    assert tuple(h.functions) == NEW == N.CATTRAIN_EXPORTS and not h.structs
    assert h.constants["SSDK_SPP_TRAIN_MAX_SIDE"] == N.SPP_TRAIN_MAX_SIDE >= 64
    for name in NEW:
        fn = getattr(N.lib, name)
        assert (fn.restype, list(fn.argtypes)) == (h.functions[name][0], h.functions[name][1]), name
        assert name not in N.EXPORTS
    assert len(N.EXPORTS) == 127 and N.lib.ssdk_version() == 245 and N.ABI_VERSION == 245
    assert N.FUSE_SAME == SAME and N.FUSE_UP2 == UP2


def test_bad_arguments_are_refused_before_any_launch():
    from ssds import _native as N

    L = N.lib
    F = 0x1000  # never dereferenced: every call below fails validation first
    err = lambda: L.ssdk_last_error().decode()  # noqa: E731
    side = N.SPP_TRAIN_MAX_SIDE

    def cfwd(a=F, b=F, y=F, n=2, c1=3, c2=5, h=6, w=10, mode=SAME, dt=N.BF16):
        return L.ssdk_cat_train_fwd(a, b, y, n, c1, c2, h, w, mode, dt, None)

    def cbwd(gy=F, ga=F, gb=F, n=2, c1=3, c2=5, h=6, w=10, mode=SAME, dt=N.BF16):
        return L.ssdk_cat_train_bwd(gy, ga, gb, n, c1, c2, h, w, mode, dt, None)

    def sfwd(x=F, y=F, n=2, c=4, h=7, w=9, dt=N.BF16):
        return L.ssdk_spp_train_fwd(x, y, n, c, h, w, dt, None)

    def sbwd(x=F, gy=F, gx=F, n=2, c=4, h=7, w=9, dt=N.BF16):
        return L.ssdk_spp_train_bwd(x, gy, gx, n, c, h, w, dt, None)

    cat_bad = [dict(dt=N.F32), dict(dt=7), dict(n=0), dict(c1=0), dict(c2=0), dict(h=0), dict(w=0), dict(n=-1),
               dict(mode=UP2, h=7), dict(mode=UP2, w=9), dict(mode=2), dict(mode=-1), dict(mode=5),
               dict(n=1 << 15, c1=1 << 14, c2=1 << 14, h=2, w=2)]  # 2^31 elements
    for fn, name in ((cfwd, "cat_train_fwd"), (cbwd, "cat_train_bwd")):
        for kw in cat_bad:
            assert fn(**kw) == -1 and name in err(), (name, kw, err())
    for kw in (dict(a=None), dict(b=None), dict(y=None), dict(a=F + 1), dict(b=F + 1), dict(y=F + 1)):
        assert cfwd(**kw) == -1 and "cat_train_fwd" in err(), kw
    for kw in (dict(gy=None), dict(gy=F + 1), dict(ga=F + 1), dict(gb=F + 1)):
        assert cbwd(**kw) == -1 and "cat_train_bwd" in err(), kw
    assert cbwd(ga=None, gb=None) == 0  # nothing asked for: nothing launched
    spp_bad = [dict(dt=N.F32), dict(dt=9), dict(n=0), dict(c=0), dict(h=0), dict(w=0), dict(c=-2), dict(x=None), dict(x=F + 1),
               dict(h=side + 1, w=side), dict(h=side, w=side + 1), dict(n=1 << 15, c=1 << 14, h=1, w=1)]  # 4 C channels: 2^31 elements
    for fn, name in ((sfwd, "spp_train_fwd"), (sbwd, "spp_train_bwd")):
        for kw in spp_bad:
            assert fn(**kw) == -1 and name in err(), (name, kw, err())
    assert sfwd(y=None) == -1 and sbwd(gy=None) == -1 and sbwd(gx=None) == -1 and sbwd(gx=F + 1) == -1


def test_cpu_tensors_raise_in_the_explicit_functions_and_decline_in_try():
    import torch
    from ssds.modeling.layers import cattrain as CT

    torch.manual_seed(0)
    a, b = torch.randn(1, 2, 4, 4).bfloat16(), torch.randn(1, 3, 2, 2).bfloat16()
    before = dict(CT.STATS)
    with pytest.raises(ValueError):
        CT.cat2(a, b, CT.UP2)
    with pytest.raises(ValueError):
        CT.cat2(a.float(), a.float(), CT.SAME)
    with pytest.raises(ValueError):
        CT.spp(a)
    with pytest.raises(ValueError):
        CT.spp(a.float())
    assert CT.try_cat2(a, b, CT.UP2) is None and CT.try_cat2(a, a, CT.SAME) is None and CT.try_spp(a) is None
    assert CT.STATS == before and CT.MAX_SIDE >= 64 and (CT.SAME, CT.UP2) == (SAME, UP2)


def _stub_backbone(channels=(8, 12, 16)):
    import torch.nn as nn

    class Stub(nn.Module):
        """Three maps at 1/2, 1/4, 1/8 of a 3-channel image (strided 1x1 convolutions)."""

        def __init__(self):
            super(Stub, self).__init__()
            self.c = nn.ModuleList([nn.Conv2d(3, ch, 1, stride=s) for ch, s in zip(channels, (2, 4, 8))])

        def initialize(self):
            return None

        def forward(self, x):
            return [c(x) for c in self.c]

    return Stub()


def _small_model(kind):
    from ssds.modeling.ssds.yolo import YOLOV3, YOLOV4

    cls = YOLOV3 if kind == "yolov3" else YOLOV4
    _, extras, head = cls.add_extras([[0, 1, 2, "Conv:S"], [8, 12, 16, 16]], [2, 2, 2, 2], 3)
    return cls(_stub_backbone(), extras, head, 3)


@pytest.mark.parametrize("kind", ["yolov3", "yolov4"])
def test_flagged_model_equals_the_unflagged_one_on_cpu(kind):
    """fp32 on the CPU, train mode: forward outputs, the input gradient and every parameter gradient bit for bit."""
    import torch
    from ssds.modeling.layers import cattrain as CT

    torch.manual_seed(3)
    ref = _small_model(kind).train()
    flagged = CT.use_native_cat(copy.deepcopy(ref))
    assert any(getattr(m, "native_cat", False) for m in flagged.modules())
    assert not any(getattr(m, "native_cat", False) for m in ref.modules())
    assert list(flagged.state_dict()) == list(ref.state_dict())
    x = torch.randn(2, 3, 32, 32)
    calls = {k: v for k, v in CT.STATS.items() if k.endswith("ward")}
    outs = []
    for m in (ref, flagged):
        xi = x.clone().requires_grad_(True)
        loc, conf = m(xi)
        sum((t * t).mean() for t in loc + conf).backward()
        outs.append((loc + conf, dict({k: p.grad for k, p in m.named_parameters()}, input=xi.grad)))
    (ya, ga), (yb, gb) = outs
    assert len(ya) == len(yb) == 8 and all(torch.equal(u, v) for u, v in zip(ya, yb))
    assert list(ga) == list(gb) and all(g is not None for g in ga.values())
    assert all(torch.equal(ga[k], gb[k]) for k in ga), [k for k in ga if not torch.equal(ga[k], gb[k])]
    assert {k: v for k, v in CT.STATS.items() if k.endswith("ward")} == calls


CFGS = {"yolov3_resnet18_320.yml": (1, 0, 0), "yolov4_resnet18_512.yml": (0, 1, 1), "ssd_mobilenetv2_300.yml": (0, 0, 0),
        "fpn_resnet50_640.yml": (0, 0, 0)}


@pytest.mark.parametrize("cfg_name", sorted(CFGS))
def test_use_native_cat_flags_exactly_the_yolo_modules(cfg_name):
    from ssds.core import config
    from ssds.modeling import model_builder
    from ssds.modeling.layers import cattrain as CT
    from ssds.modeling.ssds.yolo import YOLOV3, PANModule, SPPModule

    cfg = config.cfg_from_file(os.path.join(ROOT, "experiments", "cfgs", cfg_name))
    model = model_builder.create_model(cfg.MODEL)
    keys = list(model.state_dict().keys())
    classes = [type(m) for m in model.modules()]
    want = [m for m in model.modules() if isinstance(m, (YOLOV3, PANModule, SPPModule))]
    n3, npan, nspp = CFGS[cfg_name]
    assert len(want) == n3 + npan + nspp
    assert not any(getattr(m, "native_cat", False) for m in model.modules())
    before = dict(CT.STATS)
    assert CT.use_native_cat(model) is model
    delta = {k: CT.STATS[k] - before[k] for k in before}
    assert delta == dict({k: 0 for k in before}, yolov3_models=n3, pan_modules=npan, spp_modules=nspp)
    flagged = [m for m in model.modules() if getattr(m, "native_cat", False)]
    assert len(flagged) == len(want) and all(a is b for a, b in zip(flagged, want))
    assert [type(m) for m in model.modules()] == classes and list(model.state_dict().keys()) == keys
    CT.use_native_cat(model)  # a second call switches nothing more
    assert {k: CT.STATS[k] - before[k] for k in before} == delta


def test_use_native_cat_leaves_other_spp_blocks_alone():
    import torch.nn as nn
    from ssds.modeling.layers import cattrain as CT
    from ssds.modeling.ssds.yolo import SPPModule

    before = dict(CT.STATS)
    others = nn.ModuleList([SPPModule(3, "avg_pool"), SPPModule(2), SPPModule(4), SPPModule(1, "avg_pool")])
    CT.use_native_cat(others)
    assert not any(m.native_cat for m in others) and CT.STATS == before
    one = nn.Sequential(SPPModule(3))
    CT.use_native_cat(one)
    assert one[0].native_cat and CT.STATS["spp_modules"] == before["spp_modules"] + 1


_SOLVER = r"""
import torch.nn as nn
from ssds.core import config
from ssds.utils import train_ddp
from ssds.modeling.layers import cattrain as CT, denseconv as DC, neckfuse as NF
cfg = config.cfg_from_file(%(cfg)r)
s = train_ddp.Solver(cfg, 0, torch.device("cpu"))
mods = list(s.model.modules())
plain3 = sum(type(m) is nn.Conv2d and m.kernel_size == (3, 3) for m in mods)
print("RESULT", plain3, sum(bool(getattr(m, "native_cat", False)) for m in mods), CT.STATS["yolov3_models"], CT.STATS["pan_modules"],
      CT.STATS["spp_modules"], DC.STATS["swapped"], NF.STATS["maxpools"], NF.STATS["bifpn_modules"] + NF.STATS["fpn_models"])
"""


def _solver(cfg_name, **switches):
    unset = dict.fromkeys(("SSDK_CAT_TRAIN", "SSDK_DENSE3_TRAIN", "SSDK_NECK_TRAIN", "SSDK_CONV3_NATIVE"))
    return run_solver_script(_SOLVER, cfg_name, env=dict(unset, **switches))


@pytest.mark.parametrize("cfg_name", ["yolov3_resnet18_320.yml", "yolov4_resnet18_512.yml"])
@pytest.mark.parametrize("setting", ["defaults", "on", "off"])
def test_solver_routing(cfg_name, setting):
    """train_ddp.Solver on the two YOLO configs (the switches are read when the Solver is built: a subprocess per setting).  With
    SSDK_DENSE3_TRAIN on, no plain nn.Conv2d with a 3x3 kernel is left in the model; an unset SSDK_DENSE3_TRAIN means
    denseconv.YOLO_DEFAULT on these models (the step A/B of DESIGN.md 4.5h decides it: with "0" only the extras leave nn.Conv2d, for
    the im2col path).  The stem max-pool is switched under SSDK_NECK_TRAIN, and SSDK_CAT_TRAIN flags exactly the YOLO modules unless
    it is 0."""
    from ssds.modeling.layers import cattrain as CT, denseconv as DC

    n3, npan, nspp = CFGS[cfg_name]
    every, none = (n3 + npan + nspp, n3, npan, nspp), (0, 0, 0, 0)
    assert CT.DEFAULT in ("0", "1") and DC.YOLO_DEFAULT in ("0", "1")
    if setting == "defaults":
        plain3, flagged, s3, span, sspp, swapped, pools, necks = _solver(cfg_name)
        assert pools == 1 and necks == 0
        assert (flagged, s3, span, sspp) == (every if CT.DEFAULT == "1" else none)
        assert (plain3 == 0 and swapped > 0) if DC.YOLO_DEFAULT == "1" else (plain3 > 0 and swapped == 0)
    elif setting == "on":
        plain3, flagged, s3, span, sspp, swapped, pools, necks = _solver(cfg_name, SSDK_DENSE3_TRAIN="1", SSDK_CAT_TRAIN="1", SSDK_NECK_TRAIN="1")
        assert plain3 == 0 and swapped > 0 and pools == 1 and necks == 0 and (flagged, s3, span, sspp) == every
    else:
        plain3, flagged, s3, span, sspp, swapped, pools, necks = _solver(cfg_name, SSDK_DENSE3_TRAIN="0", SSDK_CAT_TRAIN="0", SSDK_NECK_TRAIN="0")
        assert plain3 > 0 and swapped == 0 and pools == 0 and necks == 0 and (flagged, s3, span, sspp) == none


@pytest.mark.parametrize("switch", [None, "1", "0"])
def test_solver_leaves_ssd_models_alone(switch):
    res = _solver("ssd_mobilenetv2_512.yml", **({} if switch is None else {"SSDK_CAT_TRAIN": switch}))
    assert res[1:5] == [0, 0, 0, 0] and res[5:] == [0, 0, 0]
