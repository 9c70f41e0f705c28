"""The DenseNet121 backbone without a GPU: ``DenseNet`` / ``DenseNet121`` (ssds/modeling/nets/densenet.py) against the outputs of the
REFERENCE's own classes on the same seeded weights (tests/golden/net_*dn121*.npz, written by tests/golden/make_golden_densenet.py), the
two shipped configs, the C-ABI of include/ssdk_denselayer.h and the planner's walk.  The kernels and the plans are checked on the GPU
in tests/test_gpu_denselayer.py."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import cases_densenet
import nethelp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFGS = {"SSDFPN": os.path.join(ROOT, "experiments", "cfgs", "fpn_densenet121_640.yml"),
        "YOLOV3": os.path.join(ROOT, "experiments", "cfgs", "yolov3_densenet121_416.yml")}
LEVELS = {"fpn_dn121": 5, "yolov3_dn121": 3}
BLOCKS = (6, 12, 24, 16)
# (input channels, output channels) of the four dense blocks of DenseNet121; block l lives on the image over 2^(l + 1)
WIDTHS = [(64, 256), (128, 512), (256, 1024), (512, 1024)]


class Fixture(dict):
    """A fixture as nethelp reads one: ``bn_flat`` (make_golden_densenet.py stores the 240 BatchNorm statistics as one vector) is
    split back into the ``bn/<key>`` entries of the other fixtures."""

    def __init__(self, name):
        npz = nethelp.load_fixture(name)
        super().__init__({k: npz[k] for k in npz.files})
        for k, v in cases_densenet.bn_state(self).items():
            self["bn/" + k] = v

    @property
    def files(self):
        return list(self)


def build(name, monkeypatch):
    """nethelp.build (schema, shapes and key order against the fixture, seeded weights, stored BatchNorm statistics)."""
    monkeypatch.setattr(nethelp, "cases", cases_densenet)
    return nethelp.build(name, fx=Fixture(name))


def build_bare(name="dn121_bare"):
    """The bare backbone of ``BACKBONE_CASES`` with nethelp.build's checks: keys, shapes and ORDER of the state_dict equal the
    reference's."""
    from ssds.modeling import nets

    fx = Fixture(name)
    seed, net, outputs, _ = cases_densenet.BACKBONE_CASES[name]
    model = getattr(nets, net)(outputs=outputs)
    ref_spec = [(str(k), tuple(int(s) for s in str(sh).split(",")) if str(sh) else ()) for k, sh in zip(fx["keys"], fx["shapes"])]
    assert [(k, tuple(v.shape)) for k, v in model.state_dict().items()] == ref_spec
    state = cases_densenet.seeded_state(ref_spec, seed)
    for k in list(state):
        if "bn/" + k in fx:
            state[k] = fx["bn/" + k]
    model.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in state.items()})
    return model.eval(), torch.from_numpy(cases_densenet.net_image(name)), fx


# ---- 1. the module ---------------------------------------------------------------------------------------------------------------
def test_reachable_by_name():
    from ssds.modeling import nets
    from ssds.modeling.nets.densenet import DenseNet, DenseNet121, _DenseBlock, _DenseLayer, _Transition

    assert getattr(nets, "DenseNet121") is DenseNet121
    net = DenseNet121(outputs=[2, 3, 4])
    assert isinstance(net, DenseNet) and net.outputs == [2, 3, 4] and net.initialize() is None
    assert [n for n, _ in net.named_children()] == ["conv1", "denseblock1", "transition1", "denseblock2", "transition2", "denseblock3",
                                                     "transition3", "denseblock4"]
    assert [n for n, _ in net.conv1.named_children()] == ["conv", "norm", "relu", "pool"]
    assert [len(getattr(net, "denseblock%d" % (i + 1))) for i in range(4)] == list(BLOCKS)
    assert all(isinstance(getattr(net, "denseblock%d" % (i + 1)), _DenseBlock) for i in range(4))
    assert all(isinstance(getattr(net, "transition%d" % (i + 1)), _Transition) for i in range(3))
    layer = net.denseblock3.denselayer24
    assert isinstance(layer, _DenseLayer) and [n for n, _ in layer.named_children()] == ["norm1", "relu1", "conv1", "norm2", "relu2", "conv2"]
    assert layer.conv1.in_channels == 256 + 23 * 32 and layer.conv1.out_channels == 128 and layer.conv2.out_channels == 32
    assert [n for n, _ in net.transition2.named_children()] == ["norm", "relu", "conv", "pool"]
    assert not hasattr(net, "norm5") and not hasattr(net, "classifier")
    assert all(m.bias is None for m in net.modules() if isinstance(m, torch.nn.Conv2d))
    bns = [m for m in net.modules() if isinstance(m, torch.nn.BatchNorm2d)]
    assert all(bool((m.weight == 1).all()) and bool((m.bias == 0).all()) for m in bns)
    # the reference's defaults
    d = DenseNet(outputs=[1])
    assert (d.growth_rate, d.block_config, d.bn_size, d.drop_rate) == (32, (6, 12, 24, 16), 4, 0) and d.conv1.conv.out_channels == 64
    # the maps of the levels in `outputs`, nothing behind the last one
    short = DenseNet(block_config=(2, 2, 2, 2), outputs=[1, 3])
    with torch.no_grad():
        maps = short.eval()(torch.zeros(1, 3, 64, 64))
    assert [tuple(m.shape) for m in maps] == [(1, 128, 16, 16), (1, 128, 4, 4)]
    with torch.no_grad():
        maps = DenseNet121(outputs=[1, 2, 3, 4]).eval()(torch.zeros(1, 3, 64, 32))
    assert [tuple(m.shape) for m in maps] == [(1, 256, 16, 8), (1, 512, 8, 4), (1, 1024, 4, 2), (1, 1024, 2, 1)]


@pytest.fixture(scope="module", params=["SSDFPN", "YOLOV3"])
def shipped(request):
    from ssds.core import config
    from ssds.modeling import model_builder

    cfg = config.cfg_from_file(CFGS[request.param])
    torch.manual_seed(0)
    return request.param, cfg, model_builder.create_model(cfg.MODEL)


def test_shipped_configs_build(shipped):
    from ssds.modeling import model_builder, ssds
    from ssds.modeling.nets.densenet import DenseNet

    head, cfg, model = shipped
    assert isinstance(model, getattr(ssds, head)) and cfg.MODEL.SSDS == head and cfg.MODEL.NETS == "DenseNet121"
    assert isinstance(model.backbone, DenseNet) and model.backbone.outputs == [2, 3, 4]
    assert cfg.MODEL.NUM_CLASSES == 80 and cfg.TRAIN.BATCH_SIZE == cfg.TEST.BATCH_SIZE == 32
    anchors = model_builder.create_anchors(cfg.MODEL, model, cfg.MODEL.IMAGE_SIZE)
    if head == "YOLOV3":
        assert list(cfg.MODEL.IMAGE_SIZE) == [416, 416] and list(anchors) == [8, 16, 32]
        assert [list(f) for f in cfg.MODEL.FEATURE_LAYER] == [[2, 3, 4], [512, 1024, 1024]]
    else:
        assert list(cfg.MODEL.IMAGE_SIZE) == [640, 640] and list(anchors) == [8, 16, 32, 64, 128]
        assert [list(f) for f in cfg.MODEL.FEATURE_LAYER] == [[2, 3, 4, "Conv:S", "Conv:S"], [512, 1024, 1024, 1024, 256]]


def test_state_dict_schema_is_the_reference_s():
    model, _, fx = build_bare()  # (asserts keys, shapes and order)
    keys = [str(k) for k in fx["keys"]]
    assert keys[:6] == ["conv1.conv.weight", "conv1.norm.weight", "conv1.norm.bias", "conv1.norm.running_mean", "conv1.norm.running_var",
                        "conv1.norm.num_batches_tracked"]
    assert keys[6] == "denseblock1.denselayer1.norm1.weight" and keys[-1] == "denseblock4.denselayer16.conv2.weight"
    assert "transition3.conv.weight" in keys and not [k for k in keys if "norm5" in k or "classifier" in k]
    assert sum(m.num_features for m in model.modules() if isinstance(m, torch.nn.BatchNorm2d)) == 40800


def test_bare_backbone_matches_reference_fp32():
    model, x, fx = build_bare()
    with torch.no_grad():
        maps = model(x)
    assert len(maps) == 2
    for i, m in enumerate(maps):
        want = torch.from_numpy(fx["out%d" % i])
        assert m.shape == want.shape and float(want.std()) > 0.1
        torch.testing.assert_close(m, want, rtol=1e-3, atol=5e-4 * float(want.abs().max()))  # (tolerances of test_darknet_cpu.py)


@pytest.mark.parametrize("name", list(cases_densenet.NET_CASES))
def test_module_matches_reference_fp32(name, monkeypatch):
    model, x, fx = build(name, monkeypatch)  # (asserts keys, shapes and order of the state_dict against the reference's)
    nt = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        with torch.no_grad():
            loc, conf = model(x)
    finally:
        torch.set_num_threads(nt)
    wl, wc = nethelp.want(fx)
    assert len(loc) == len(wl) == LEVELS[name] and len(conf) == len(wc) == LEVELS[name]
    for i, (l, a, c, b) in enumerate(zip(loc, wl, conf, wc)):
        assert l.shape == a.shape and c.shape == b.shape, (name, i)
        assert float(b.std()) > 0.01 and float(a.abs().max()) > 0.1, (name, i)  # the fixture compares something
        torch.testing.assert_close(l, a, rtol=1e-3, atol=5e-4 * float(a.abs().max()))  # (tolerances of test_darknet_cpu.py)
        torch.testing.assert_close(c, b, rtol=1e-3, atol=2e-4)


def test_train_mode_and_backward_reach_every_parameter():
    model, x, _ = build_bare()
    model.train()
    maps = model(x)
    loss = sum((m ** 2).mean() for m in maps)
    loss.backward()
    params = dict(model.named_parameters())
    assert params and all(p.requires_grad for p in params.values())
    missing = [k for k, p in params.items() if p.grad is None or not bool(torch.isfinite(p.grad).all())]
    assert not missing, missing[:8]


# ---- 2. the C-ABI ----------------------------------------------------------------------------------------------------------------
def test_abi_symbols_and_sizes(tmp_path):
    """The layer has a header of its own (include/ssdk_denselayer.h): the entry points of ssdk.h and the layout of ssdk_op stay the
    closed list of ABI 245; executor ops 11 - 13 are described by existing members of ssdk_op."""
    from ssds import _native as N

    assert N.lib.ssdk_version() == 245 and N.ABI_VERSION == 245 and len(N.EXPORTS) == 127
    header = open(os.path.join(ROOT, "include", "ssdk_denselayer.h")).read()
    main = open(os.path.join(ROOT, "include", "ssdk.h")).read()
    assert N.DENSE_EXPORTS == ("ssdk_dense_layer", "ssdk_dense_layer_desc_bytes", "ssdk_dense_layer_supported", "ssdk_dense_pool",
                               "ssdk_dense_pool_desc_bytes", "ssdk_dense_place", "ssdk_dense_place_desc_bytes")
    for name in N.DENSE_EXPORTS:
        assert (name + "(") in header and hasattr(N.lib, name) and getattr(N.lib, name).argtypes is not None, name
        assert name not in N.EXPORTS and (name + "(") not in main
    assert N.lib.ssdk_dense_layer.argtypes == [ctypes.POINTER(N.DenseLayerDesc), ctypes.c_void_p]
    assert N.lib.ssdk_dense_pool.argtypes == [ctypes.POINTER(N.DensePoolDesc), ctypes.c_void_p]
    assert N.lib.ssdk_dense_place.argtypes == [ctypes.POINTER(N.DensePlaceDesc), ctypes.c_void_p]
    assert N.lib.ssdk_dense_layer_supported.argtypes == [ctypes.c_int] * 5
    for desc, fn in ((N.DenseLayerDesc, N.lib.ssdk_dense_layer_desc_bytes), (N.DensePoolDesc, N.lib.ssdk_dense_pool_desc_bytes),
                     (N.DensePlaceDesc, N.lib.ssdk_dense_place_desc_bytes)):
        assert fn.argtypes == [] and ctypes.sizeof(desc) == fn()
    assert [f[0] for f in N.DenseLayerDesc._fields_] == ["x", "y", "w1", "a", "b", "scale1", "bias1", "w2", "w1_frag", "w2_frag",
                                                         "N", "H", "W", "Cin", "ld", "dtype"]
    assert [f[0] for f in N.DensePoolDesc._fields_] == ["x", "y", "a", "b", "N", "H", "W", "C", "ld", "dtype"]
    assert [f[0] for f in N.DensePlaceDesc._fields_] == ["x", "y", "N", "H", "W", "C", "ld", "dtype"]
    assert (N.OP_DENSE, N.OP_DENSEPOOL, N.OP_DENSEPLACE) == (11, 12, 13) and N.OP_DKRES == 10
    assert "SSDK_OP_DENSE = 11" in main and "SSDK_OP_DENSEPOOL = 12, SSDK_OP_DENSEPLACE = 13" in main
    assert [f[0] for f in N.Op._fields_] == ["kind", "lane", "conv", "mb", "fuse", "stem", "pool", "xpair", "mbse"]
    assert N.lib.ssdk_struct_size(7) == ctypes.sizeof(N.Op) and N.lib.ssdk_struct_size(8) == 0
    assert N.lib.ssdk_abi_check(N.ABI_VERSION, ctypes.sizeof(N.Op)) == 0
    assert (N.DENSE_TILE_H, N.DENSE_TILE_W, N.DENSE_CMID, N.DENSE_COUT) == (8, 16, 128, 32)
    # the sizes as a C compiler sees the headers
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include "ssdk_denselayer.h"\nint main(void) { printf("%zu %zu %zu %zu %d %d %d %d %d\\n", '
                   'sizeof(ssdk_dense_layer_desc), sizeof(ssdk_dense_pool_desc), sizeof(ssdk_dense_place_desc), sizeof(ssdk_op), '
                   '(int)SSDK_OP_DENSE, (int)SSDK_OP_DENSEPOOL, (int)SSDK_OP_DENSEPLACE, SSDK_DENSE_TILE_H, SSDK_DENSE_TILE_W); return 0; }\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert [int(v) for v in out] == [ctypes.sizeof(N.DenseLayerDesc), ctypes.sizeof(N.DensePoolDesc), ctypes.sizeof(N.DensePlaceDesc),
                                     ctypes.sizeof(N.Op), 11, 12, 13, N.DENSE_TILE_H, N.DENSE_TILE_W]


F0 = 0x100000  # never dereferenced: every call below fails validation first


def _layer(**kw):
    from ssds import _native as N

    d = N.DenseLayerDesc()
    d.N, d.H, d.W, d.Cin, d.ld, d.dtype = 2, 13, 9, 128, 192, N.BF16
    d.x, d.y = F0, F0 + 2 * 128
    d.w1, d.a, d.b, d.scale1, d.bias1, d.w2 = (F0 + 0x1000000 + 0x100000 * i for i in range(6))
    for k, v in kw.items():
        setattr(d, k, v)
    rc = N.lib.ssdk_dense_layer(ctypes.byref(d), None)
    return rc, N.lib.ssdk_last_error().decode()


def _pool(**kw):
    from ssds import _native as N

    d = N.DensePoolDesc()
    d.N, d.H, d.W, d.C, d.ld, d.dtype = 2, 13, 9, 128, 192, N.BF16
    d.x, d.y, d.a, d.b = F0, F0 + 0x1000000, F0 + 0x2000000, F0 + 0x3000000
    for k, v in kw.items():
        setattr(d, k, v)
    rc = N.lib.ssdk_dense_pool(ctypes.byref(d), None)
    return rc, N.lib.ssdk_last_error().decode()


def _place(**kw):
    from ssds import _native as N

    d = N.DensePlaceDesc()
    d.N, d.H, d.W, d.C, d.ld, d.dtype = 2, 13, 9, 128, 192, N.BF16
    d.x, d.y = F0, F0 + 0x1000000
    for k, v in kw.items():
        setattr(d, k, v)
    rc = N.lib.ssdk_dense_place(ctypes.byref(d), None)
    return rc, N.lib.ssdk_last_error().decode()


def test_bad_arguments_are_refused_before_any_launch():
    """No device is needed: each call is refused by the argument checks, with a message that names the entry point."""
    from ssds import _native as N

    for kw in (dict(Cin=0), dict(Cin=16), dict(Cin=100), dict(Cin=2080, ld=2112), dict(Cin=-32),  # Cin outside the rule
               dict(ld=128), dict(ld=152), dict(ld=164), dict(ld=0),  # ld < Cin + 32; not a multiple of 8
               dict(y=F0), dict(y=F0 + 2 * 96), dict(y=F0 + 2 * 176), dict(y=F0 + 2 * (192 + 64)), dict(y=F0 - 2 * 16),  # y on x's channels
               dict(w1_frag=F0 + 0x4000000), dict(w2_frag=F0 + 0x4000000),  # one fragment image without the other
               dict(dtype=N.F32), dict(dtype=9), dict(H=0), dict(W=0), dict(H=-3), dict(W=32769), dict(N=0),
               dict(x=None), dict(y=None), dict(w1=None), dict(w2=None), dict(a=None), dict(b=None), dict(scale1=None), dict(bias1=None),
               dict(x=F0 + 8), dict(y=F0 + 2 * 128 + 2), dict(w2=F0 + 0x1000000 + 4), dict(a=F0 + 0x1100000 + 4),
               dict(N=1 << 20, H=1 << 15, W=1 << 15)):
        rc, msg = _layer(**kw)
        assert rc == -1 and msg.startswith("dense_layer:"), (kw, rc, msg)
    assert "overlap" in _layer(y=F0)[1] and "overlap" in _layer(y=F0 + 2 * 176)[1] and "overlap" in _layer(y=F0 + 2 * (192 + 64))[1]
    assert "together" in _layer(w1_frag=F0 + 0x4000000)[1]
    assert N.lib.ssdk_dense_layer(None, None) == -1
    for kw in (dict(C=0), dict(C=12), dict(C=200), dict(ld=100), dict(ld=124), dict(H=1), dict(W=1), dict(H=0), dict(W=32769), dict(N=0),
               dict(dtype=N.F32), dict(x=None), dict(y=None), dict(a=None), dict(b=None), dict(x=F0 + 8), dict(y=F0 + 0x1000000 + 4),
               dict(a=F0 + 0x2000000 + 4), dict(y=F0 + 64), dict(x=F0 + 0x1000000 + 32)):
        rc, msg = _pool(**kw)
        assert rc == -1 and msg.startswith("dense_pool:"), (kw, rc, msg)
    assert N.lib.ssdk_dense_pool(None, None) == -1
    for kw in (dict(C=0), dict(C=12), dict(C=200), dict(ld=100), dict(ld=124), dict(H=0), dict(W=0), dict(W=32769), dict(N=0),
               dict(dtype=N.F32), dict(x=None), dict(y=None), dict(x=F0 + 8), dict(y=F0 + 0x1000000 + 4), dict(y=F0 + 64),
               dict(x=F0 + 0x1000000 + 32)):
        rc, msg = _place(**kw)
        assert rc == -1 and msg.startswith("dense_place:"), (kw, rc, msg)
    assert N.lib.ssdk_dense_place(None, None) == -1


def test_the_predicate_agrees_with_the_refusals():
    from ssds import _native as N

    sup = N.lib.ssdk_dense_layer_supported
    for cin in range(8, 2080, 8):
        ok = cin % 32 == 0 and 32 <= cin <= 2048
        for ld in (cin + 32, cin + 96):
            assert bool(sup(cin, 13, 9, ld, N.BF16)) == ok and bool(sup(cin, 13, 9, ld, N.F16)) == ok, (cin, ld)
            if not ok:
                rc, msg = _layer(Cin=cin, ld=ld, y=F0 + 2 * cin)
                assert rc == -1 and "unsupported" in msg, (cin, msg)
        for ld in (cin, cin + 24, cin + 36):  # too narrow; not a multiple of 8
            assert sup(cin, 13, 9, ld, N.BF16) == 0, (cin, ld)
            rc, msg = _layer(Cin=cin, ld=ld, y=F0 + 2 * cin)
            assert rc == -1 and "unsupported" in msg, (cin, ld, msg)
    for cin in (32, 992, 2048):
        assert sup(cin, 1, 1, cin + 32, N.F16) == 1 and sup(cin, 32768, 32768, cin + 32, N.BF16) == 1
        for h, w, dt in ((0, 4, N.BF16), (4, 0, N.BF16), (-1, 4, N.F16), (4, 32769, N.F16), (4, 4, N.F32), (4, 4, 7)):
            assert sup(cin, h, w, cin + 32, dt) == 0
            rc, msg = _layer(Cin=cin, ld=cin + 32, y=F0 + 2 * cin, H=h, W=w, dtype=dt)
            assert rc == -1 and "unsupported" in msg, (cin, h, w, dt, msg)


# ---- 3. the planner --------------------------------------------------------------------------------------------------------------
def _bare_plan(dtype=torch.bfloat16):
    from ssds.modeling.layers import fused_conv as FC
    from ssds.modeling.layers import planner

    model, x, _ = build_bare()
    model = model.to(dtype)
    plan = FC.ConvPlan(x.device, dtype, x.shape)
    outs = planner.record_backbone(plan, plan.input_value(), model)
    return model, plan.finalize(), outs


def test_planner_records_one_dense_op_per_layer_into_one_buffer_per_block(monkeypatch):
    from ssds import _native as N

    monkeypatch.delenv("SSDK_DENSELAYER", raising=False)
    _, plan, outs = _bare_plan()
    kinds = [L.get("kind") for L in plan.layers]
    assert kinds.count("dense") == 58 and kinds.count("densepool") == 3 and kinds.count("denseplace") == 4
    assert "cat" not in kinds and kinds.count(None) == 3 and kinds[:3] == ["stem7", "pool", "denseplace"]
    assert len(kinds) == 2 + 58 + 3 + 4 + 3
    assert [tuple(o[1:]) for o in outs] == [(2, 1024, 6, 4), (2, 1024, 3, 2)]
    # the order: place, the block's layers, then per transition pool -> 1x1 -> place
    want_order = []
    for bi, nl in enumerate(BLOCKS):
        want_order += ["denseplace"] + ["dense"] * nl + (["densepool", None] if bi < 3 else [])
    assert kinds[2:] == want_order
    # the buffer walk: every dense op reads [0, Cin) and writes [Cin, Cin + 32) of its block's buffer, Cin growing by 32
    at = 2
    hw = [(24, 16), (12, 8), (6, 4), (3, 2)]
    bufs = []
    for bi, nl in enumerate(BLOCKS):
        c0, ctot = WIDTHS[bi]
        place = plan.layers[at]
        buf = place["y"]
        bufs.append(buf)
        assert (place["ch"], place["ld"], place["h"], place["w"]) == (c0, ctot, hw[bi][0], hw[bi][1]) and place["x"] != buf
        for j in range(nl):
            L, op = plan.layers[at + 1 + j], plan.ops[at + 1 + j]
            cin = c0 + 32 * j
            assert L["x"] == L["y"] == buf and (L["cin"], L["ld"], L["h"], L["w"]) == (cin, ctot, hw[bi][0], hw[bi][1])
            xp = op.xpair
            assert op.kind == N.OP_DENSE and op.lane == 0 and xp.x == plan.arena.ptr(buf) and xp.y == xp.x + 2 * cin
            assert (xp.Cin, xp.Cmid, xp.Cout, xp.pad, xp.N, xp.H, xp.W) == (cin, 128, 32, ctot, 2, hw[bi][0], hw[bi][1])
            assert xp.act1 == N.ACT["relu"] and xp.act2 == N.ACT["none"] and xp.dtype == N.BF16
            assert xp.w1 and xp.w2 and xp.scale1 and xp.bias1 and xp.scale2 and xp.bias2 and bool(xp.w1_frag) == bool(xp.w2_frag)
            assert L["pack"].a.numel() == cin and L["pack"].w1.shape == (128, cin) and L["pack"].w2.shape == (32, 3, 3, 128)
        at += 1 + nl
        if bi < 3:
            pool, conv = plan.layers[at], plan.layers[at + 1]
            assert pool["x"] == buf and (pool["ch"], pool["ld"]) == (ctot, ctot) and pool["y"] != buf
            assert conv["x"] == pool["y"] and conv["pack"].k == 1 and conv["pack"].scale is None and conv["act"] == "none"
            assert (conv["pack"].cin, conv["pack"].cout, conv["h"], conv["w"]) == (ctot, ctot // 2, hw[bi + 1][0], hw[bi + 1][1])
            op = plan.ops[at]
            assert op.kind == N.OP_DENSEPOOL and (op.conv.Cin, op.conv.Cout, op.conv.k, op.conv.stride, op.conv.split) == (ctot, ctot, 2, 2, ctot)
            assert plan.ops[at + 2].kind == N.OP_DENSEPLACE and plan.ops[at + 2].conv.split == WIDTHS[bi + 1][1]
            at += 2
    assert at == len(plan.layers)
    assert [o[0] for o in outs] == bufs[2:]
    table = plan.layer_table()
    assert len(table) == len(plan.layers)
    row = table[3]
    assert row["name"] == "dense 64>128>32 k1,k3 @24x16"
    assert row["flops"] == 2.0 * 2 * 24 * 16 * (64 * 128 + 9 * 128 * 32)
    assert row["bytes"] == 2.0 * (2 * 24 * 16 * (64 + 32) + 64 * 128 + 9 * 128 * 32)


def test_no_buffer_is_released_before_its_last_reader(monkeypatch):
    """The arena hands a buffer out again once it is released.  Replaying the recording in order: whatever an op reads was last
    written by the op that was recorded as its producer, with the shape the reader expects, and the output maps are never written
    again."""
    from ssds.modeling.layers.fused_conv import _out_hw

    _, plan, outs = _bare_plan()
    holds, checked = {}, 0  # buffer -> (tag of the tensor it holds, channels valid, h, w)
    for i, L in enumerate(plan.layers):
        kind = L.get("kind")
        if kind == "dense":
            assert holds[L["x"]] == ("block", L["cin"], L["h"], L["w"], L["ld"]), (i, holds[L["x"]])
            holds[L["x"]] = ("block", L["cin"] + 32, L["h"], L["w"], L["ld"])
            checked += 1
            continue
        if kind == "denseplace":
            assert holds[L["x"]] == ("dense", L["ch"], L["h"], L["w"]) and L["y"] != L["x"], (i, holds[L["x"]])
            holds[L["y"]] = ("block", L["ch"], L["h"], L["w"], L["ld"])
            checked += 1
            continue
        if kind == "densepool":
            assert holds[L["x"]] == ("block", L["ch"], L["h"], L["w"], L["ch"]) and L["y"] != L["x"], (i, holds[L["x"]])
            holds[L["y"]] = ("dense", L["ch"], L["h"] // 2, L["w"] // 2)
            checked += 1
            continue
        if kind == "pool":
            assert holds[L["x"]] == ("dense", L["ch"], L["h"], L["w"]) and L["y"] != L["x"]
            holds[L["y"]] = ("dense", L["ch"], (L["h"] - 1) // 2 + 1, (L["w"] - 1) // 2 + 1)
            checked += 1
            continue
        pk = L["pack"]
        if isinstance(L["x"], int):
            assert holds[L["x"]] == ("dense", pk.cin, L["h"], L["w"]) and L["y"] != L["x"], (i, holds[L["x"]])
            checked += 1
        if kind == "stem7":
            holds[L["y"]] = ("dense", pk.cout, (L["h"] - 1) // 2 + 1, (L["w"] - 1) // 2 + 1)
        else:
            holds[L["y"]] = ("dense", pk.cout) + _out_hw(L["h"], L["w"], pk.k, pk.stride)
    assert checked == len(plan.layers) - 1
    assert [holds[o[0]] for o in outs] == [("block", 1024, 6, 4, 1024), ("block", 1024, 3, 2, 1024)]


def test_the_switch_sends_the_backbone_to_torch(monkeypatch):
    from ssds.modeling.layers import planner

    monkeypatch.setenv("SSDK_DENSELAYER", "0")
    with pytest.raises(planner.PlanUnsupported, match="SSDK_DENSELAYER=0"):
        _bare_plan()
    monkeypatch.setenv("SSDK_DENSELAYER", "1")
    _, plan, _ = _bare_plan()
    assert [L.get("kind") for L in plan.layers].count("dense") == 58


def test_planner_refuses_what_the_kernels_do_not_cover():
    from ssds.modeling.layers import fused_conv as FC
    from ssds.modeling.layers import planner
    from ssds.modeling.nets.densenet import DenseNet

    def record(net, train=False):
        net = net.train(train).to(torch.bfloat16)
        plan = FC.ConvPlan(torch.device("cpu"), torch.bfloat16, (1, 3, 64, 64))
        return planner.record_backbone(plan, plan.input_value(), net)

    assert len(record(DenseNet(block_config=(2, 2, 2, 2), outputs=[2]))) == 1
    with pytest.raises(planner.PlanUnsupported, match=r"denseblock1\.denselayer1.*growth = 16"):
        record(DenseNet(growth_rate=16, block_config=(2, 2), num_init_features=64, bn_size=8, outputs=[1]))
    with pytest.raises(planner.PlanUnsupported, match=r"denseblock1\.denselayer1.*bn_size \* growth = 64"):
        record(DenseNet(block_config=(2, 2), bn_size=2, outputs=[1]))
    with pytest.raises(planner.PlanUnsupported, match=r"denseblock1\.denselayer1.*drop_rate 0\.2 in training mode"):
        record(DenseNet(block_config=(2, 2), drop_rate=0.2, outputs=[1]), train=True)
    assert len(record(DenseNet(block_config=(2, 2), drop_rate=0.2, outputs=[1]))) == 1  # (eval: dropout is the identity)
    net = DenseNet(block_config=(2, 2), outputs=[2])
    net.denseblock2 = torch.nn.Identity()
    with pytest.raises(planner.PlanUnsupported, match="denseblock2: block Identity has no planner"):
        record(net)
    net = DenseNet(block_config=(2, 2), outputs=[2])
    net.denseblock1.denselayer2 = torch.nn.Identity()
    with pytest.raises(planner.PlanUnsupported, match=r"denseblock1\.denselayer2: block Identity has no planner"):
        record(net)
    net = DenseNet(block_config=(2, 2), outputs=[2])
    net.denseblock1.denselayer2.relu1 = torch.nn.ReLU6()
    with pytest.raises(planner.PlanUnsupported, match=r"denseblock1\.denselayer2.*ReLU"):
        record(net)
    net = DenseNet(block_config=(2, 2), outputs=[2])
    net.transition1.pool = torch.nn.MaxPool2d(2, 2)
    with pytest.raises(planner.PlanUnsupported, match=r"transition1.*AvgPool2d"):
        record(net)
    net = DenseNet(block_config=(2, 2), outputs=[1])
    net.conv1.conv = torch.nn.Conv2d(3, 64, 3, stride=2, padding=1, bias=False)
    with pytest.raises(planner.PlanUnsupported, match="conv1"):
        record(net)
    # a layer the predicate refuses: 2080 input channels
    with pytest.raises(planner.PlanUnsupported, match=r"denseblock1\.denselayer64.*ssdk_dense_layer_supported"):
        record(DenseNet(block_config=(64,), outputs=[1]))
    # a map without a 2x2 window in front of a transition
    net = DenseNet(block_config=(2, 2, 2, 2), outputs=[4]).eval().to(torch.bfloat16)
    plan = FC.ConvPlan(torch.device("cpu"), torch.bfloat16, (1, 3, 16, 16))
    with pytest.raises(planner.PlanUnsupported, match="transition3.*no 2x2 window"):
        planner.record_backbone(plan, plan.input_value(), net)
