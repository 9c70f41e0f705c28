"""The ShuffleNetV2 training step (csrc/ssdk_shuffletrain.hip, include/ssdk_shuffletrain.h, ssds/modeling/layers/shuffletrain.py), the
parts that need no GPU: the header and its bound entry points, their argument checks (all made before any device call), the layout
of the padded weight images, which modules ``use_native_shuffle`` flags, swaps and marks, that a flagged model computes bit for
bit what the unflagged one does on the CPU, the Solver's routing, and the channel arithmetic of a slice."""
import copy
import os

import numpy as np
import pytest

import shufflejudge as SJ
from solverhelp import run_solver_script

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ssdk_pws_prepare", "ssdk_pws_stats_workspace_bytes", "ssdk_pws_forward", "ssdk_pws_wgrad_workspace_bytes", "ssdk_pws_wgrad",
       "ssdk_shuffle_join_fwd", "ssdk_shuffle_join_bwd")
CONFIGS = {"fpn_shufflenetv2_x1_512.yml": [("transforms.0", 116)],
           "yolov3_shufflenetv2_x2_416.yml": [("extras.0.0", 366), ("extras.1.0", 732)]}  # marked 1x1 layers outside the backbone


def test_header_parses_and_every_symbol_is_bound():
    from ssds import _native as N

    with open(os.path.join(ROOT, "include", "ssdk_shuffletrain.h")) as f:
        h = N.parse_header(f.read())
    assert tuple(h.functions) == NEW == N.SHUFFLETRAIN_EXPORTS and not h.structs and not h.constants
    assert N.SHUFFLETRAIN_HEADER_PATH.endswith("ssdk_shuffletrain.h")
    for name in NEW:
        fn = getattr(N.lib, name)
        assert (fn.restype, list(fn.argtypes)) == (h.functions[name][0], h.functions[name][1]), name
        assert name not in N.EXPORTS
    assert len(N.EXPORTS) == 127 and N.lib.ssdk_version() == 245 and N.ABI_VERSION == 245


def test_bad_arguments_are_refused_before_any_launch():
    from ssds import _native as N

    L = N.lib
    F = 0x1000  # never dereferenced: every call below fails validation first
    err = lambda: L.ssdk_last_error().decode()  # noqa: E731
    BAD, WORKSPACE = -1, -2
    assert (N._K["SSDK_E_BADARG"], N._K["SSDK_E_WORKSPACE"]) == (BAD, WORKSPACE)

    def prep(w32=F, w16=F, wt16=F, cout=58, cin=58, dt=N.BF16):
        return L.ssdk_pws_prepare(w32, w16, wt16, cout, cin, dt, None)

    for kw in (dict(w32=None), dict(w16=None), dict(wt16=None), dict(cout=0), dict(cin=0), dict(cin=-3), dict(dt=N.F32), dict(dt=9)):
        assert prep(**kw) == BAD and "pws_prepare" in err(), kw

    def fwd(x=F, xs=58 * 63, a=F, lda=64, bias=None, y=F, ys=58 * 63, sums=None, ws=None, wsb=0, b=2, k=58, m=58, hw=63, dt=N.BF16):
        return L.ssdk_pws_forward(x, xs, a, lda, bias, y, ys, sums, ws, wsb, b, k, m, hw, dt, None)

    fwd_bad = [dict(x=None), dict(a=None), dict(y=None), dict(x=F + 1), dict(y=F + 1), dict(a=F + 8), dict(k=7), dict(m=7), dict(k=0),
               dict(m=-1), dict(b=0), dict(hw=0), dict(lda=56), dict(lda=60), dict(lda=0), dict(xs=58 * 63 - 1), dict(ys=58 * 63 - 1),
               dict(xs=0), dict(dt=N.F32), dict(dt=5), dict(b=1 << 16, xs=1 << 16, ys=1 << 16),  # 2^32 elements over the strides
               dict(xs=1 << 32), dict(ys=1 << 32), dict(sums=F), dict(sums=F, ws=F + 4, wsb=1 << 30)]
    for kw in fwd_bad:
        assert fwd(**kw) == BAD and "pws_forward" in err(), (kw, err())
    need = L.ssdk_pws_stats_workspace_bytes(2, 58, 58, 63)
    assert need > 0 and L.ssdk_pws_stats_workspace_bytes(2, 7, 58, 63) == 0 and L.ssdk_pws_stats_workspace_bytes(0, 58, 58, 63) == 0
    assert fwd(sums=F, ws=F, wsb=need - 1) == WORKSPACE and "workspace" in err()

    def wg(dy=F, x=F, xs=58 * 63, dw=F, ws=F, wsb=1 << 40, b=2, cout=58, cin=58, hw=63, dt=N.BF16):
        return L.ssdk_pws_wgrad(dy, x, xs, dw, ws, wsb, b, cout, cin, hw, dt, None)

    for kw in (dict(dy=None), dict(x=None), dict(dw=None), dict(ws=None), dict(x=F + 1), dict(dy=F + 1), dict(b=0), dict(cout=0), dict(cin=0),
               dict(hw=0), dict(xs=58 * 63 - 1), dict(dt=N.F32), dict(dt=4), dict(b=1 << 16, xs=1 << 16), dict(xs=1 << 32),
               dict(b=1 << 12, cout=1 << 12, hw=1 << 8, cin=8, xs=8 << 8)):
        assert wg(**kw) == BAD and "pws_wgrad" in err(), (kw, err())
    need = L.ssdk_pws_wgrad_workspace_bytes(2, 58, 58, 63)
    assert need > 0 and L.ssdk_pws_wgrad_workspace_bytes(2, 0, 58, 63) == 0
    assert wg(wsb=need - 1) == WORKSPACE and "workspace" in err()

    def jf(left=F, ls=58 * 63, right=F, y=F, n=2, cb=58, hw=63, dt=N.BF16):
        return L.ssdk_shuffle_join_fwd(left, ls, right, y, n, cb, hw, dt, None)

    def jb(gy=F, gl=F, gls=58 * 63, gr=F, n=2, cb=58, hw=63, dt=N.BF16):
        return L.ssdk_shuffle_join_bwd(gy, gl, gls, gr, n, cb, hw, dt, None)

    for kw in (dict(left=None), dict(right=None), dict(y=None), dict(left=F + 1), dict(right=F + 1), dict(y=F + 1), dict(n=0), dict(cb=0),
               dict(hw=0), dict(ls=58 * 63 - 1), dict(dt=N.F32), dict(dt=3), dict(n=1 << 15, cb=1 << 14, hw=4, ls=1 << 16), dict(ls=1 << 32)):
        assert jf(**kw) == BAD and "shuffle_join_fwd" in err(), (kw, err())
    for kw in (dict(gy=None), dict(gr=None), dict(gy=F + 1), dict(gl=F + 1), dict(gr=F + 1), dict(n=0), dict(cb=-1), dict(hw=0),
               dict(gls=58 * 63 - 1), dict(dt=N.F32), dict(n=1 << 15, cb=1 << 14, hw=4, gls=1 << 16), dict(gls=1 << 32)):
        assert jb(**kw) == BAD and "shuffle_join_bwd" in err(), (kw, err())


@pytest.mark.parametrize("cout,cin", SJ.PREPARE_SHAPES)
def test_padded_weight_images(cout, cin):
    """The layout ssdk_pws_prepare writes, as the numpy oracle describes it (tests/test_gpu_shuffle_train.py holds the kernel
    against the same oracle): Kp / Mp columns, the matrix and its transpose in place, zeros in the padding; and the layer's buffers
    have those shapes."""
    from ssds.modeling.layers import shuffletrain as ST

    w = np.arange(1, cout * cin + 1, dtype=np.float32).reshape(cout, cin)
    w16, wt16 = SJ.prepare_oracle(w)
    kp, mp = w16.shape[1], wt16.shape[1]
    assert (kp, mp) == (ST._pad8(cin), ST._pad8(cout)) and kp % 8 == 0 and mp % 8 == 0 and 0 <= kp - cin < 8 and 0 <= mp - cout < 8
    assert {(58, 24): (24, 64), (58, 58): (64, 64), (122, 244): (248, 128)}[(cout, cin)] == (kp, mp)
    assert w16.shape == (cout, kp) and wt16.shape == (cin, mp)
    assert np.array_equal(w16[:, :cin], w) and np.array_equal(wt16[:, :cout], w.T)
    assert not w16[:, cin:].any() and not wt16[:, cout:].any()
    assert w16.ravel()[3 * kp + 5] == w[3, 5] and wt16.ravel()[5 * mp + 3] == w[3, 5]  # row-major, leading dimensions Kp / Mp


def test_wgrad_plan_restates_the_library():
    from ssds import _native as N
    from ssds.modeling.layers import shuffletrain as ST

    for b, cout, cin, hw in ((2, 58, 58, 63), (3, 122, 122, 169), (2, 116, 116, 25), (2, 24, 24, 25), (2, 58, 24, 81), (1, 232, 232, 128),
                             (32, 976, 488, 169), (32, 116, 116, 4096), (64, 24, 58, 16384)):
        tiled, splits, cps = ST.wgrad_plan(b, cout, cin, hw)
        assert (splits + (splits + 63) // 64) * cout * cin * 4 == N.lib.ssdk_pws_wgrad_workspace_bytes(b, cout, cin, hw)
        assert N.lib.ssdk_pws_wgrad_workspace_bytes(b, cout, cin, hw) == N.lib.ssdk_pw_wgrad_workspace_bytes(b, cout, cin, hw)
        assert tiled == (cout > 48 and cin > 48) and splits * cps >= b * ((hw + 127) // 128)
    assert ST.wgrad_sum_depth(1) == 32 + 4 + 36


@pytest.mark.parametrize("cfg_name", sorted(CONFIGS))
def test_use_native_shuffle_flags_swaps_and_marks(cfg_name):
    import torch.nn as nn
    from ssds.core import config
    from ssds.modeling import model_builder
    from ssds.modeling.layers import shuffletrain as ST
    from ssds.modeling.layers.dwconv import DepthwiseConv2d
    from ssds.modeling.nets.shufflenet import InvertedResidual

    cfg = config.cfg_from_file(os.path.join(ROOT, "experiments", "cfgs", cfg_name))
    model = model_builder.create_model(cfg.MODEL)
    keys = list(model.state_dict().keys())
    assert not any(getattr(m, "native_shuffle", False) or getattr(m, "_ssdk_any_width", False) for m in model.modules())
    before = dict(ST.STATS)
    assert ST.use_native_shuffle(model) is model
    delta = {k: ST.STATS[k] - before[k] for k in before}
    outside = CONFIGS[cfg_name]
    assert delta == dict({k: 0 for k in before}, units=16, depthwise=19, pointwise=35 + len(outside))
    units = [m for m in model.backbone.modules() if isinstance(m, InvertedResidual)]
    assert len(units) == 16 and all(m.native_shuffle for m in units) and not InvertedResidual.native_shuffle
    assert sum(m.stride == 1 for m in units) == 13
    assert sum(type(m) is DepthwiseConv2d for m in model.backbone.modules()) == 19
    assert not any(type(m) is nn.Conv2d and m.groups > 1 for m in model.backbone.modules())
    marked = [(n, m.in_channels) for n, m in model.named_modules() if getattr(m, "_ssdk_any_width", False)]
    assert [nm for nm in marked if not nm[0].startswith("backbone.")] == outside
    inside = [m for n, m in model.named_modules() if n.startswith("backbone.") and getattr(m, "_ssdk_any_width", False)]
    assert len(inside) == 35 and all(m.kernel_size == (1, 1) and m.groups == 1 for m in inside)
    assert list(model.state_dict().keys()) == keys
    ST.use_native_shuffle(model)  # a second call switches nothing more
    assert {k: ST.STATS[k] - before[k] for k in before} == delta


def test_use_native_shuffle_leaves_other_models_alone():
    from ssds.core import config
    from ssds.modeling import model_builder
    from ssds.modeling.layers import shuffletrain as ST

    cfg = config.cfg_from_file(os.path.join(ROOT, "experiments", "cfgs", "ssd_mobilenetv2_512.yml"))
    model = model_builder.create_model(cfg.MODEL)
    classes = [type(m) for m in model.modules()]
    before = dict(ST.STATS)
    ST.use_native_shuffle(model)
    assert ST.STATS == before and [type(m) for m in model.modules()] == classes
    assert not any(getattr(m, "_ssdk_any_width", False) for m in model.modules())


def test_flagged_backbone_equals_the_unflagged_one_on_cpu():
    """fp32 on the CPU, train mode: the flag declines -- outputs, the input gradient and every parameter gradient bit for bit, and
    no counter moves."""
    import torch
    from ssds.modeling.layers import shuffletrain as ST
    from ssds.modeling.nets.shufflenet import ShuffleNetV2

    torch.manual_seed(5)
    ref = ShuffleNetV2([2, 2, 2], [24, 116, 232, 464, 1024], outputs=[2, 3, 4]).train()
    flagged = ST.use_native_shuffle(copy.deepcopy(ref))
    assert all(m.native_shuffle for m in flagged.stage2) and not any(m.native_shuffle for m in ref.stage2)
    assert list(flagged.state_dict()) == list(ref.state_dict())
    x = torch.randn(2, 3, 64, 64)
    calls = {k: v for k, v in ST.STATS.items() if k.endswith("ward")}
    outs = []
    for m in (ref, flagged):
        xi = x.clone().requires_grad_(True)
        ys = m(xi)
        sum((t * t).mean() for t in ys).backward()
        outs.append((ys, dict({k: p.grad for k, p in m.named_parameters()}, input=xi.grad)))
    (ya, ga), (yb, gb) = outs
    assert len(ya) == len(yb) == 3 and all(torch.equal(u, v) for u, v in zip(ya, yb))
    assert list(ga) == list(gb) and all(g is not None for g in ga.values())
    assert all(torch.equal(ga[k], gb[k]) for k in ga), [k for k in ga if not torch.equal(ga[k], gb[k])]
    assert {k: v for k, v in ST.STATS.items() if k.endswith("ward")} == calls
    # the explicit functions raise on operands outside the contract, the try_ forms decline
    a = torch.randn(1, 16, 4, 4).bfloat16()
    with pytest.raises(ValueError):
        ST.join(a, a)
    with pytest.raises(ValueError):
        ST.conv_slice(a, 8, torch.randn(8, 8, 1, 1))
    assert ST.try_join(a, a) is None and ST.try_unit(flagged.stage2[1], torch.randn(1, 116, 4, 4)) is None
    assert {k: v for k, v in ST.STATS.items() if k.endswith("ward")} == calls


@pytest.mark.parametrize("shape,cb", [((2, 116, 7, 9), 58), ((3, 244, 13, 13), 122), ((2, 48, 5, 5), 24), ((1, 464, 16, 8), 232), ((2, 24, 3, 3), 7)])
def test_slice_arithmetic_matches_torch_strides(shape, cb):
    """The pointer offset and the image stride the kernels are handed are those of the view x[:, cb:]."""
    import torch
    from ssds.modeling.layers import shuffletrain as ST

    x = torch.zeros(shape, dtype=torch.bfloat16)
    view = x[:, cb:]
    off, stride = ST.slice_geometry(x.shape, cb)
    assert off == view.storage_offset() and stride == view.stride(0)
    assert view.data_ptr() == x.data_ptr() + 2 * off and view.stride(1) == shape[2] * shape[3]
    assert stride >= view.shape[1] * shape[2] * shape[3]  # what the entry points require of an image stride
    halves = x.chunk(2, 1)
    if 2 * cb == shape[1]:
        assert halves[1].data_ptr() == view.data_ptr() and halves[1].stride() == view.stride()
        assert halves[1].is_contiguous() == (shape[0] == 1)  # (one image: the half is a contiguous tensor)
        assert ST.slice_geometry(x.shape, 0) == (0, halves[0].stride(0))  # the left operand of the join


_SOLVER = r"""
import torch.nn as nn
from ssds.core import config
from ssds.utils import train_ddp
from ssds.modeling.layers import shuffletrain as ST
from ssds.modeling.layers.dwconv import DepthwiseConv2d
from ssds.modeling.layers.pointwise import PointwiseConv2d
cfg = config.cfg_from_file(%(cfg)r)
s = train_ddp.Solver(cfg, 0, torch.device("cpu"))
mods = list(s.model.modules())
bb = list(s.model.backbone.modules())
print("RESULT", sum(bool(getattr(m, "native_shuffle", False)) for m in mods), ST.STATS["units"], ST.STATS["depthwise"], ST.STATS["pointwise"],
      sum(bool(getattr(m, "_ssdk_any_width", False)) and type(m) is PointwiseConv2d for m in mods),
      sum(type(m) is DepthwiseConv2d and m._ssdk_bn_follows for m in bb), sum(type(m) is nn.Conv2d and m.groups > 1 for m in bb))
"""


def _solver(cfg_name, switch):
    return run_solver_script(_SOLVER, cfg_name, env={"SSDK_SHUFFLE_TRAIN": switch})


@pytest.mark.parametrize("switch", [None, "0", "1"])
def test_solver_routing(switch):
    """train_ddp.Solver on a ShuffleNetV2 config (the switch is read when the Solver is built: a subprocess per setting): with the
    switch on, the 16 units are flagged, the 19 depthwise layers are DepthwiseConv2d with the statistics hand-off to their
    BatchNorm, the marked 1x1 layers are PointwiseConv2d; with 0 nothing is touched.  Unset follows shuffletrain.DEFAULT."""
    from ssds.modeling.layers import shuffletrain as ST

    assert ST.DEFAULT in ("0", "1")
    on = (ST.DEFAULT if switch is None else switch) == "1"
    flagged, units, dw, pw, marked_pw, dw_bn, plain_dw = _solver("fpn_shufflenetv2_x1_512.yml", switch)
    if on:
        assert (flagged, units, dw, pw, marked_pw, dw_bn, plain_dw) == (16, 16, 19, 36, 36, 19, 0)
    else:
        assert (flagged, units, dw, pw, marked_pw, dw_bn, plain_dw) == (0, 0, 0, 0, 0, 0, 19)


@pytest.mark.parametrize("switch", [None, "0", "1"])
def test_solver_leaves_mobilenet_alone(switch):
    res = _solver("ssd_mobilenetv2_512.yml", switch)
    assert res[:5] == [0, 0, 0, 0, 0] and res[6] == 0
