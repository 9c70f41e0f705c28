"""The transposed convolution of the Shelf TRAINING step (csrc/ssdk_convttrain.hip, include/ssdk_convttrain.h,
ssds/modeling/layers/convttrain.py), the parts that need no GPU: the header and its bound entry points, their argument checks (all
made before any device call), the torch twins of the packed images walked the way the kernels walk them, which layers ``supported``
takes, that a swapped model computes bit for bit what the unswapped one does on the CPU, and the Solver's routing of the shipped
Shelf config.  The kernels themselves are checked on the GPU in tests/test_gpu_shelf_train.py."""
import copy
import os

import pytest

from solverhelp import run_solver_script

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ssdk_convt_train_prepare", "ssdk_convt_train_forward", "ssdk_convt_train_dgrad", "ssdk_convt_train_wgrad_workspace_bytes",
       "ssdk_convt_train_wgrad")


def test_header_parses_and_every_symbol_is_bound():
    import ctypes
    from ssds import _native as N

    with open(os.path.join(ROOT, "include", "ssdk_convttrain.h")) as f:
        h = N.parse_header(f.read())
    assert tuple(h.functions) == NEW == N.CONVTTRAIN_EXPORTS and not h.structs
    for name in NEW:
        fn = getattr(N.lib, name)
        assert (fn.restype, list(fn.argtypes)) == (h.functions[name][0], h.functions[name][1]), name
        assert name not in N.EXPORTS
    assert N.lib.ssdk_convt_train_wgrad_workspace_bytes.restype is ctypes.c_size_t
    assert len(N.EXPORTS) == 127 and N.lib.ssdk_version() == 245 and N.ABI_VERSION == 245


def test_bad_arguments_are_refused_before_any_launch():
    from ssds import _native as N

    L = N.lib
    F = 0x1000  # never dereferenced: every call below fails validation first
    err = lambda: L.ssdk_last_error().decode()  # noqa: E731

    def prep(w=F, f=F, d=F, cin=32, cout=16, dt=N.BF16):
        return L.ssdk_convt_train_prepare(w, f, d, cin, cout, dt, None)

    def fwd(x=F, img=F, bias=None, skip=None, y=F, n=2, cin=32, cout=16, h=5, w=4, dt=N.BF16):
        return L.ssdk_convt_train_forward(x, img, bias, skip, y, n, cin, cout, h, w, dt, None)

    def dgr(gy=F, img=F, gx=F, n=2, cin=32, cout=16, h=5, w=4, dt=N.BF16):
        return L.ssdk_convt_train_dgrad(gy, img, gx, n, cin, cout, h, w, dt, None)

    def need(n=2, cin=32, cout=16, h=5, w=4):
        return int(L.ssdk_convt_train_wgrad_workspace_bytes(n, cin, cout, h, w))

    def wgr(x=F, gy=F, gw=F, gb=F, ws=F, nbytes=None, n=2, cin=32, cout=16, h=5, w=4, dt=N.BF16):
        nbytes = need(n, cin, cout, h, w) if nbytes is None else nbytes
        return L.ssdk_convt_train_wgrad(x, gy, gw, gb, ws, nbytes, n, cin, cout, h, w, dt, None)

    shapes = [dict(cin=24), dict(cout=24), dict(cin=17), dict(cout=15), dict(cin=8), dict(cout=8), dict(cin=0), dict(cin=4112),
              dict(cout=4112), dict(dt=N.F32), dict(dt=7)]
    maps = [dict(n=0), dict(h=0), dict(w=0), dict(n=-1),
            dict(n=1 << 15, cin=4096, h=4, w=4),  # x: 2^31 elements
            dict(n=1 << 13, cout=4096, h=5, w=5),  # y: 2^13 * 2^12 * 81 elements
            dict(n=1, h=1 << 15, w=1 << 15)]
    for fn, name in ((fwd, "convt_train_forward"), (dgr, "convt_train_dgrad"), (wgr, "convt_train_wgrad")):
        for kw in shapes + maps:
            assert fn(**kw) == -1 and name in err(), (name, kw, err())
        for kw in maps + [k for k in shapes if "dt" not in k]:
            assert need(**{k: v for k, v in kw.items()}) == 0, kw
    for kw in shapes:
        assert prep(**kw) == -1 and "convt_train_prepare" in err(), kw
    for kw in (dict(w=None), dict(f=None, d=None), dict(f=F + 8), dict(d=F + 2), dict(w=F + 1)):
        assert prep(**kw) == -1 and "convt_train_prepare" in err(), kw
    for kw in (dict(x=None), dict(img=None), dict(y=None), dict(x=F + 1), dict(y=F + 1), dict(skip=F + 1), dict(bias=F + 2), dict(img=F + 8)):
        assert fwd(**kw) == -1 and "convt_train_forward" in err(), kw
    for kw in (dict(gy=None), dict(img=None), dict(gx=None), dict(gy=F + 1), dict(gx=F + 1), dict(img=F + 4)):
        assert dgr(**kw) == -1 and "convt_train_dgrad" in err(), kw
    assert need() > 0 and need() % 16 == 0
    for kw in (dict(x=None), dict(gy=None), dict(gw=None), dict(ws=None), dict(ws=F + 8), dict(x=F + 1), dict(gy=F + 1), dict(gw=F + 2),
               dict(gb=F + 2), dict(nbytes=need() - 1), dict(nbytes=0)):
        assert wgr(**kw) == -1 and "convt_train_wgrad" in err(), kw


@pytest.mark.parametrize("h,w", [(1, 1), (2, 3), (5, 4)])
def test_the_images_walked_as_the_kernels_walk_them_are_the_layer(h, w):
    """The torch twins of the packed images, evaluated in fp64 with the kernels' tap offsets (the method of
    tests/test_shelf_cpu.py::test_parity_form_is_the_transposed_convolution): the forward per output parity class over the pixels
    that have the neighbours it reads, the input gradient as the stride-2 convolution -- against F.conv_transpose2d and its
    autograd, 16 -> 16 channels."""
    import torch
    import torch.nn.functional as F
    from ssds.modeling.layers import convttrain as CT, denseconv as D

    torch.manual_seed(10 * h + w)
    cin = cout = 16
    n = 2
    wt = torch.randn(cin, cout, 3, 3, dtype=torch.float64)
    x = torch.randn(n, cin, h, w, dtype=torch.float64, requires_grad=True)
    want = F.conv_transpose2d(x, wt, None, 2, 1)
    assert tuple(want.shape) == (n, cout, 2 * h - 1, 2 * w - 1)
    gy = torch.randn_like(want)
    (gx_want,) = torch.autograd.grad(want, (x,), gy)
    fimg, dimg = CT.pack_forward_image(wt), CT.pack_dgrad_image(wt)
    assert tuple(fimg.shape) == D.image_shape(cout, cin)[:2] + (4, 16, 8) and tuple(dimg.shape) == D.image_shape(cin, cout)[:2] + (4, 16, 8)
    for py in (0, 1):
        for px in (0, 1):
            taps = CT.forward_class_taps(py, px)
            assert len(taps) == (1 + py) * (1 + px) and len({t[2] for t in taps}) == len(taps)
            # an output pixel (2a + py, 2b + px) and the input pixel (a + dy, b + dx) meet at tap ky = py + 1 - 2 dy of w, which the
            # flipped image numbers 2 - ky
            assert all(tap == 3 * (2 - (py + 1 - 2 * dy)) + (2 - (px + 1 - 2 * dx)) for dy, dx, tap in taps)
    got = CT.forward_from_image(x.detach(), fimg, cout)
    torch.testing.assert_close(got, want.detach(), rtol=0, atol=1e-12)
    torch.testing.assert_close(CT.dgrad_from_image(gy, dimg, cin), gx_want, rtol=0, atol=1e-12)


def test_supported_takes_the_config_layers_and_declines_the_rest():
    import torch.nn as nn
    from ssds.core import config
    from ssds.modeling import model_builder
    from ssds.modeling.layers import convttrain as CT

    cfg = config.cfg_from_file(os.path.join(ROOT, "experiments", "cfgs", "shelf_resnet18_513.yml"))
    model = model_builder.create_model(cfg.MODEL)
    convts = [m for m in model.modules() if isinstance(m, nn.ConvTranspose2d)]
    assert [(m.in_channels, m.out_channels) for m in convts] == [(512, 256), (256, 128)] * 2
    assert all(CT.supported(m) for m in convts)
    T = nn.ConvTranspose2d
    assert CT.supported(T(16, 16, 3, stride=2, padding=1)) and CT.supported(T(4096, 2048, 3, stride=2, padding=1, bias=False))
    for m in (T(32, 16, 3, stride=2, padding=1, output_padding=1), T(32, 16, 3, stride=1, padding=1), T(32, 16, 2, stride=2),
              T(32, 16, 3, stride=2, padding=0), T(32, 32, 3, stride=2, padding=1, groups=2), T(24, 16, 3, stride=2, padding=1),
              T(16, 24, 3, stride=2, padding=1), T(8, 16, 3, stride=2, padding=1), T(32, 16, 3, stride=2, padding=1, dilation=2),
              nn.Conv2d(32, 16, 3, stride=2, padding=1)):
        assert not CT.supported(m), m
    before = dict(CT.STATS)
    other = CT.use_native_convt(nn.Sequential(T(24, 16, 3, stride=2, padding=1), nn.Conv2d(16, 16, 3)))
    assert type(other[0]) is T and dict(CT.STATS) == before


def _stub_shelf(channels=(32, 48, 64)):
    import torch.nn as nn
    from ssds.modeling.ssds.shelf import SSDShelf

    class Stub(nn.Module):
        """Three maps at 17 / 9 / 5 pixels of a 33 x 33 image (strided 1x1 convolutions)."""

        def __init__(self):
            super(Stub, self).__init__()
            self.c = nn.ModuleList([nn.Conv2d(3, ch, 1, stride=s) for ch, s in zip(channels, (2, 4, 8))])

        def initialize(self):
            return None

        def forward(self, x):
            return [c(x) for c in self.c]

    _, extras, head = SSDShelf.add_extras([[0, 1, 2], list(channels)], [2, 2, 2], 3)
    return SSDShelf(Stub(), extras, head, 3)


def test_swapped_model_equals_the_unswapped_one_on_cpu():
    """fp32 on the CPU, train mode, Dropout2d.p = 0: forward outputs, the input gradient and every parameter gradient bit for bit;
    the same state_dict keys in the same order."""
    import torch
    import torch.nn as nn
    from ssds.modeling.layers import convttrain as CT

    torch.manual_seed(4)
    ref = _stub_shelf().train()
    for m in ref.modules():
        if isinstance(m, nn.Dropout2d):
            m.p = 0.0
    before = dict(CT.STATS)
    swapped = CT.use_native_convt(copy.deepcopy(ref))
    assert CT.STATS["swapped"] - before["swapped"] == 4
    assert sum(type(m) is CT.ShelfConvT for m in swapped.modules()) == 4 and not any(type(m) is CT.ShelfConvT for m in ref.modules())
    assert sum(type(m) is nn.ConvTranspose2d for m in ref.modules()) == 4
    assert list(swapped.state_dict()) == list(ref.state_dict())
    assert all(torch.equal(a, b) for a, b in zip(swapped.state_dict().values(), ref.state_dict().values()))
    CT.use_native_convt(swapped)  # a second call switches nothing more
    assert CT.STATS["swapped"] - before["swapped"] == 4
    x = torch.randn(2, 3, 33, 33)
    outs = []
    for m in (ref, swapped):
        xi = x.clone().requires_grad_(True)
        loc, conf = m(xi)
        sum((t * t).mean() for t in loc + conf).backward()
        outs.append((loc + conf, dict({k: p.grad for k, p in m.named_parameters()}, input=xi.grad)))
    (ya, ga), (yb, gb) = outs
    assert len(ya) == len(yb) == 6 and all(torch.equal(u, v) for u, v in zip(ya, yb))
    assert list(ga) == list(gb) and all(g is not None for g in ga.values())
    assert all(torch.equal(ga[k], gb[k]) for k in ga), [k for k in ga if not torch.equal(ga[k], gb[k])]
    assert {k: CT.STATS[k] - before[k] for k in before} == dict(swapped=4, native_forward=0, native_dgrad=0, native_wgrad=0)


def test_cpu_fp32_and_strided_operands_raise_in_the_explicit_call():
    import torch
    from ssds.modeling.layers import convttrain as CT

    torch.manual_seed(0)
    w = torch.randn(16, 16, 3, 3)
    before = dict(CT.STATS)
    for x in (torch.randn(1, 16, 3, 3).bfloat16(), torch.randn(1, 16, 3, 3)):
        with pytest.raises(ValueError):
            CT.convt3x3s2(x, w)
    assert dict(CT.STATS) == before and CT.DEFAULT in ("0", "1")


_SOLVER = r"""
import torch.nn as nn
from ssds.core import config
from ssds.utils import train_ddp
from ssds.modeling.layers import cattrain as CAT, convttrain as CT, denseconv as DC, neckfuse as NF
cfg = config.cfg_from_file(%(cfg)r)
s = train_ddp.Solver(cfg, 0, torch.device("cpu"))
mods = list(s.model.modules())
plain3 = sum(type(m) is nn.Conv2d and m.kernel_size == (3, 3) for m in mods)
print("RESULT", sum(type(m) is CT.ShelfConvT for m in mods), CT.STATS["swapped"], sum(type(m) is nn.ConvTranspose2d for m in mods), plain3,
      DC.STATS["swapped"], NF.STATS["maxpools"], sum(CAT.STATS.values()))
"""


def _solver(cfg_name, **switches):
    unset = dict.fromkeys(("SSDK_CONVT_TRAIN", "SSDK_CAT_TRAIN", "SSDK_DENSE3_TRAIN", "SSDK_NECK_TRAIN", "SSDK_CONV3_NATIVE"))
    return run_solver_script(_SOLVER, cfg_name, env=dict(unset, **switches))


@pytest.mark.parametrize("setting", ["defaults", "on", "off"])
def test_solver_routing_of_the_shelf_config(setting):
    """train_ddp.Solver on shelf_resnet18_513.yml (the switches are read when the Solver is built: a subprocess per setting).
    SSDK_CONVT_TRAIN swaps the four transposed convolutions; SSDK_DENSE3_TRAIN, which unset means denseconv.YOLO_DEFAULT on this
    model, leaves no plain 3x3 nn.Conv2d; SSDK_NECK_TRAIN switches the stem max-pool."""
    from ssds.modeling.layers import convttrain as CT, denseconv as DC

    if setting == "defaults":
        cls, swapped, plain_t, plain3, dense, pools, cat = _solver("shelf_resnet18_513.yml")
        assert (cls, swapped, plain_t) == ((4, 4, 0) if CT.DEFAULT == "1" else (0, 0, 4)) and pools == 1 and cat == 0
        assert (plain3 == 0 and dense > 0) if DC.YOLO_DEFAULT == "1" else (plain3 > 0 and dense == 0)
    elif setting == "on":
        cls, swapped, plain_t, plain3, dense, pools, cat = _solver("shelf_resnet18_513.yml", SSDK_CONVT_TRAIN="1", SSDK_DENSE3_TRAIN="1",
                                                                   SSDK_NECK_TRAIN="1")
        assert (cls, swapped, plain_t) == (4, 4, 0) and plain3 == 0 and dense > 0 and pools == 1 and cat == 0
    else:
        cls, swapped, plain_t, plain3, dense, pools, cat = _solver("shelf_resnet18_513.yml", SSDK_CONVT_TRAIN="0", SSDK_DENSE3_TRAIN="0",
                                                                   SSDK_NECK_TRAIN="0")
        assert (cls, swapped, plain_t) == (0, 0, 4) and plain3 > 0 and dense == 0 and pools == 0 and cat == 0


_UNSET = {}  # cfg name -> the routing with the new switch unset, built once


@pytest.mark.parametrize("cfg_name", ["ssd_mobilenetv2_512.yml", "fpn_resnet50_640.yml", "yolov3_resnet18_320.yml"])
@pytest.mark.parametrize("switch", [None, "1", "0"])
def test_solver_leaves_other_models_alone(cfg_name, switch):
    """SSD, FPN and YOLO models under any setting of the new switch: no layer is swapped, and what their own switches route is what
    they route without it."""
    res = _solver(cfg_name, **({} if switch is None else {"SSDK_CONVT_TRAIN": switch}))
    assert res[:3] == [0, 0, 0]
    if switch is None:
        _UNSET[cfg_name] = res
    else:
        if cfg_name not in _UNSET:
            _UNSET[cfg_name] = _solver(cfg_name)
        assert res == _UNSET[cfg_name]
