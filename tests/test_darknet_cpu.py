"""The DarkNet53 backbone without a GPU: ``DarkNet`` / ``DarkNet53`` (ssds/modeling/nets/darknet.py) against the outputs of the
REFERENCE's own classes on the same seeded weights (tests/golden/net_*dk53*.npz, written by tests/golden/make_golden_darknet.py), the
two shipped configs, the C-ABI of ``ssdk_dkres`` (include/ssdk_dkres.h) and the planner's walk.  The kernel itself and the plans are
checked on the GPU in tests/test_gpu_dkres.py."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import cases_darknet
import nethelp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFGS = {"YOLOV3": os.path.join(ROOT, "experiments", "cfgs", "yolov3_darknet53_416.yml"),
        "YOLOV4": os.path.join(ROOT, "experiments", "cfgs", "yolov4_darknet53_512.yml")}
LEVELS = {"yolov3_dk53": 3, "yolov4_dk53": 4}
# the residual blocks of DarkNet53: (level, C, blocks); a level-l map is the image over 2^l
STAGES = [(1, 64, 1), (2, 128, 2), (3, 256, 8), (4, 512, 8), (5, 1024, 4)]


def build(name, monkeypatch):
    """nethelp.build (schema, shapes and key order against the fixture, seeded weights, stored BatchNorm statistics)."""
    monkeypatch.setattr(nethelp, "cases", cases_darknet)
    return nethelp.build(name)


def build_bare(name="dk53_bare"):
    """The bare backbone of ``BACKBONE_CASES`` with nethelp.build's checks: keys, shapes and ORDER of the state_dict equal the
    reference's."""
    from ssds.modeling import nets

    fx = nethelp.load_fixture(name)
    seed, net, outputs, _ = cases_darknet.BACKBONE_CASES[name]
    model = getattr(nets, net)(outputs=outputs)
    ref_spec = [(str(k), tuple(int(s) for s in str(sh).split(",")) if str(sh) else ()) for k, sh in zip(fx["keys"], fx["shapes"])]
    assert [(k, tuple(v.shape)) for k, v in model.state_dict().items()] == ref_spec
    state = cases_darknet.seeded_state(ref_spec, seed)
    for k in list(state):
        if "bn/" + k in fx:
            state[k] = fx["bn/" + k]
    model.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in state.items()})
    return model.eval(), torch.from_numpy(cases_darknet.net_image(name)), fx


# ---- 1. the module ---------------------------------------------------------------------------------------------------------------
def test_reachable_by_name():
    from ssds.modeling import nets
    from ssds.modeling.nets.darknet import DarkNet, DarkNet53, Residual

    assert getattr(nets, "DarkNet53") is DarkNet53
    net = DarkNet53(outputs=[3, 4, 5])
    assert isinstance(net, DarkNet) and net.outputs == [3, 4, 5] and net.initialize() is None
    assert [n for n, _ in net.named_children()] == ["conv1", "block1", "block2", "block3", "block4", "block5"]
    assert [sum(isinstance(m, Residual) for m in getattr(net, "block%d" % l)) for l, _, _ in STAGES] == [1, 2, 8, 8, 4]
    assert net.conv1[0].stride == (1, 1) and net.conv1[0].bias is not None and isinstance(net.conv1[2], torch.nn.ReLU6)
    assert [n for n, _ in net.block3[1].named_children()] == ["conv1x1", "conv3x3"]
    assert sum(m.num_features for m in net.modules() if isinstance(m, torch.nn.BatchNorm2d)) == 17856
    # the maps of the levels in `outputs`, nothing behind the last one
    short = DarkNet(layers=[1, 1, 1, 1, 1], outputs=[2, 4])
    with torch.no_grad():
        maps = short.eval()(torch.zeros(1, 3, 32, 32))
    assert [tuple(m.shape) for m in maps] == [(1, 128, 8, 8), (1, 512, 2, 2)]


@pytest.fixture(scope="module", params=["YOLOV3", "YOLOV4"])
def shipped(request):
    from ssds.core import config
    from ssds.modeling import model_builder

    cfg = config.cfg_from_file(CFGS[request.param])
    torch.manual_seed(0)
    return request.param, cfg, model_builder.create_model(cfg.MODEL)


def test_shipped_configs_build_with_strides_8_16_32(shipped):
    from ssds.modeling import model_builder, ssds
    from ssds.modeling.nets.darknet import DarkNet

    head, cfg, model = shipped
    assert isinstance(model, getattr(ssds, head)) and cfg.MODEL.SSDS == head and cfg.MODEL.NETS == "DarkNet53"
    assert isinstance(model.backbone, DarkNet) and model.backbone.outputs == [3, 4, 5]
    assert cfg.MODEL.NUM_CLASSES == 80 and cfg.TRAIN.BATCH_SIZE == cfg.TEST.BATCH_SIZE == 32
    anchors = model_builder.create_anchors(cfg.MODEL, model, cfg.MODEL.IMAGE_SIZE)
    if head == "YOLOV3":
        assert list(cfg.MODEL.IMAGE_SIZE) == [416, 416] and list(anchors) == [8, 16, 32]
        assert [list(f) for f in cfg.MODEL.FEATURE_LAYER] == [[3, 4, 5], [256, 512, 1024]]
    else:
        assert list(cfg.MODEL.IMAGE_SIZE) == [512, 512] and list(anchors) == [8, 16, 32, 64]


def test_bare_backbone_matches_reference_fp32():
    model, x, fx = build_bare()  # (asserts keys, shapes and order of the state_dict against the reference's)
    with torch.no_grad():
        maps = model(x)
    assert len(maps) == 2
    for i, m in enumerate(maps):
        want = torch.from_numpy(fx["out%d" % i])
        assert m.shape == want.shape and float(want.std()) > 0.1
        torch.testing.assert_close(m, want, rtol=1e-3, atol=5e-4 * float(want.abs().max()))


@pytest.mark.parametrize("name", list(cases_darknet.NET_CASES))
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
        torch.testing.assert_close(l, a, rtol=1e-3, atol=5e-4 * float(a.abs().max()))  # (tolerances of test_yolo_cpu.py)
        torch.testing.assert_close(c, b, rtol=1e-3, atol=2e-4)


def test_train_mode_returns_logits_and_backward_reaches_every_parameter(monkeypatch):
    model, x, _ = build("yolov3_dk53", monkeypatch)
    with torch.no_grad():
        _, conf_eval = model(x)
    model.train()
    for m in model.modules():  # (batch statistics would change the outputs: the comparison is on the stored ones)
        if isinstance(m, torch.nn.BatchNorm2d):
            m.eval()
    loc, conf_train = model(x)
    for a, b in zip(conf_eval, conf_train):
        torch.testing.assert_close(a, torch.sigmoid(b.detach()), rtol=1e-6, atol=1e-7)
    loss = sum((l ** 2).mean() for l in loc) + sum(c.mean() for c in conf_train)
    loss.backward()
    params = dict(model.named_parameters())
    assert params and all(p.requires_grad for p in params.values())
    missing = [k for k, p in params.items() if p.grad is None or not bool(torch.isfinite(p.grad).all())]
    assert not missing, missing[:8]
    dead = [k for k, p in params.items() if float(p.grad.abs().max()) == 0]
    assert not dead, dead[:8]


# ---- 2. the C-ABI ----------------------------------------------------------------------------------------------------------------
def test_abi_symbols_and_sizes(tmp_path):
    """The block has a header of its own (include/ssdk_dkres.h): the entry points of ssdk.h and the layout of ssdk_op stay the
    closed list of ABI 245, and executor op kind 10 is described by the op's ssdk_xpair_desc."""
    from ssds import _native as N

    assert N.lib.ssdk_version() == 245 and N.ABI_VERSION == 245 and len(N.EXPORTS) == 127
    header = open(os.path.join(ROOT, "include", "ssdk_dkres.h")).read()
    main = open(os.path.join(ROOT, "include", "ssdk.h")).read()
    assert N.DKRES_EXPORTS == ("ssdk_dkres", "ssdk_dkres_desc_bytes", "ssdk_dkres_supported")
    for name in N.DKRES_EXPORTS:
        assert (name + "(") in header and hasattr(N.lib, name) and getattr(N.lib, name).argtypes is not None, name
        assert name not in N.EXPORTS and (name + "(") not in main
    assert N.lib.ssdk_dkres.argtypes == [ctypes.POINTER(N.DkresDesc), ctypes.c_void_p]
    assert N.lib.ssdk_dkres_supported.argtypes == [ctypes.c_int] * 4 and N.lib.ssdk_dkres_desc_bytes.argtypes == []
    assert ctypes.sizeof(N.DkresDesc) == N.lib.ssdk_dkres_desc_bytes()
    assert [f[0] for f in N.DkresDesc._fields_] == ["x", "y", "w1", "scale1", "bias1", "w2", "scale2", "bias2", "w1_frag", "w2_frag",
                                                    "N", "H", "W", "C", "act1", "act2", "dtype", "pad"]
    assert N.OP_DKRES == 10 and (N.OP_CAT, N.OP_SPP) == (8, 9) and "SSDK_OP_CAT = 8, SSDK_OP_SPP = 9" in main
    assert "SSDK_OP_DKRES = 10" in main
    assert [f[0] for f in N.Op._fields_] == ["kind", "lane", "conv", "mb", "fuse", "stem", "pool", "xpair", "mbse"]
    assert N.lib.ssdk_struct_size(7) == ctypes.sizeof(N.Op) and N.lib.ssdk_struct_size(8) == 0
    assert N.lib.ssdk_abi_check(N.ABI_VERSION, ctypes.sizeof(N.Op)) == 0
    assert (N.DKRES_TILE_H, N.DKRES_TILE_W) == (8, 16)
    # the sizes as a C compiler sees the headers
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include "ssdk_dkres.h"\nint main(void) { printf("%zu %zu %d %d %d\\n", sizeof(ssdk_dkres_desc), '
                   'sizeof(ssdk_op), (int)SSDK_OP_DKRES, SSDK_DKRES_TILE_H, SSDK_DKRES_TILE_W); return 0; }\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert [int(v) for v in out] == [ctypes.sizeof(N.DkresDesc), ctypes.sizeof(N.Op), N.OP_DKRES, N.DKRES_TILE_H, N.DKRES_TILE_W]


F0 = 0x100000  # never dereferenced: every call below fails validation first
WIDTHS = (64, 128, 256)  # what ssdk_dkres_supported is documented to take (include/ssdk_dkres.h)


def _dkres(**kw):
    from ssds import _native as N

    d = N.DkresDesc()
    d.N, d.H, d.W, d.C, d.act1, d.act2, d.dtype = 2, 13, 9, 128, N.ACT["relu6"], N.ACT["relu6"], N.BF16
    d.x, d.y = F0, F0 + 0x100000
    d.w1, d.scale1, d.bias1, d.w2, d.scale2, d.bias2 = (F0 + 0x1000000 + 0x100000 * i for i in range(6))
    for k, v in kw.items():
        setattr(d, k, v)
    rc = N.lib.ssdk_dkres(ctypes.byref(d), None)
    return rc, N.lib.ssdk_last_error().decode()


def test_bad_arguments_are_refused_before_any_launch():
    """No device is needed: each call is refused by the argument checks, with a message that names the entry point."""
    from ssds import _native as N

    nbytes = 2 * 13 * 9 * 128 * 2  # bytes of x and of y in _dkres
    for kw in (dict(C=127), dict(C=65), dict(C=32), dict(C=96), dict(C=512), dict(C=1024), dict(C=0),  # odd C; C outside the set
               dict(y=F0), dict(y=F0 + nbytes - 16), dict(y=F0 - nbytes + 16), dict(x=F0 + 0x100000 + 16),  # y == x; y overlapping x
               dict(w1_frag=F0 + 0x4000000), dict(w2_frag=F0 + 0x4000000),  # one fragment image without the other
               dict(act1=N.ACT["silu"]), dict(act2=N.ACT["sigmoid"]), dict(act1=77), dict(act2=-1),  # unknown activation
               dict(dtype=N.F32), dict(dtype=9), dict(H=0), dict(W=0), dict(H=-3), dict(W=-1), dict(N=0),
               dict(x=None), dict(y=None), dict(w1=None), dict(w2=None), dict(scale1=None), dict(bias2=None),
               dict(x=F0 + 8), dict(y=F0 + 0x100000 + 2), dict(w2=F0 + 0x1000000 + 4),
               dict(N=1 << 20, H=1 << 15, W=1 << 15)):
        rc, msg = _dkres(**kw)
        assert rc == -1 and msg.startswith("dkres:"), (kw, rc, msg)
    assert "overlaps" in _dkres(y=F0)[1] and "overlaps" in _dkres(y=F0 + nbytes - 16)[1]
    assert "together" in _dkres(w1_frag=F0 + 0x4000000)[1]
    assert N.lib.ssdk_dkres(None, None) == -1
    # y directly behind x does not overlap: that call is refused by nothing above and would launch, so it is not made here


def test_the_predicate_agrees_with_the_refusals():
    from ssds import _native as N

    sup = N.lib.ssdk_dkres_supported
    for c in range(0, 1100):
        assert bool(sup(c, 13, 9, N.BF16)) == (c in WIDTHS), c
        if c not in WIDTHS:
            rc, msg = _dkres(C=c)
            assert rc == -1 and "unsupported" in msg, (c, msg)
    for c in WIDTHS:
        assert sup(c, 1, 1, N.F16) == 1 and sup(c, 32768, 32768, N.BF16) == 1
        for h, w, dt in ((0, 4, N.BF16), (4, 0, N.BF16), (-1, 4, N.F16), (4, 32769, N.F16), (4, 4, N.F32), (4, 4, 7)):
            assert sup(c, h, w, dt) == 0
            rc, msg = _dkres(C=c, H=h, W=w, dtype=dt)
            assert rc == -1 and "unsupported" in msg, (c, h, w, dt, msg)


# ---- 3. the planner --------------------------------------------------------------------------------------------------------------
def _residuals(h, w):
    """(C, H, W) of the 23 residual blocks of DarkNet53 on an h x w image."""
    out = []
    for level, c, blocks in STAGES:
        out += [(c, (h - 1) // (1 << level) + 1, (w - 1) // (1 << level) + 1)] * blocks
    return out


def _bare_plan(dtype=torch.bfloat16):
    from ssds.modeling.layers import fused_conv as FC
    from ssds.modeling.layers import planner

    model, x, _ = build_bare()
    model = model.to(dtype)
    plan = FC.ConvPlan(x.device, dtype, x.shape)
    outs = planner.record_backbone(plan, plan.input_value(), model)
    return model, plan.finalize(), outs


def test_planner_records_one_dkres_op_per_supported_residual(monkeypatch):
    from ssds import _native as N

    monkeypatch.delenv("SSDK_DKRES", raising=False)
    model, plan, outs = _bare_plan()
    res = _residuals(96, 64)
    assert len(res) == 23
    from ssds.modeling.layers import fused_conv as FC

    routed = [r for r in res if N.lib.ssdk_dkres_supported(r[0], r[1], r[2], N.BF16) and r[0] in FC.DKRES_DEFAULT_WIDTHS]
    kinds = [L.get("kind") for L in plan.layers]
    assert set(kinds) <= {None, "dkres"} and kinds.count("dkres") == len(routed)
    assert [(L["pack"].cin, L["h"], L["w"]) for L in plan.layers if L.get("kind") == "dkres"] == routed
    # stem + 5 stride-2 convs + two convs per residual that is not fused
    assert kinds.count(None) == 1 + 5 + 2 * (23 - len(routed))
    assert plan.layers[0]["pack"].kind == "stem" and plan.layers[0]["pack"].stride == 1 and plan.layers[0]["pack"].cout == 32
    assert [tuple(o[1:]) for o in outs] == [(2, 512, 6, 4), (2, 1024, 3, 2)]
    ops = [op for op in plan.ops if op.kind == N.OP_DKRES]
    assert [(op.xpair.Cin, op.xpair.H, op.xpair.W) for op in ops] == routed
    for op in ops:
        xp = op.xpair
        assert op.lane == 0 and xp.x and xp.y and xp.x != xp.y and xp.Cout == xp.Cin == 2 * xp.Cmid and xp.N == 2
        assert xp.act1 == xp.act2 == N.ACT["relu6"] and xp.dtype == N.BF16
        assert xp.w1 and xp.w2 and xp.scale1 and xp.bias1 and xp.scale2 and xp.bias2 and bool(xp.w1_frag) == bool(xp.w2_frag)
    table = plan.layer_table()
    rows = [r for r in table if r["name"].startswith("dkres ")]
    assert len(table) == len(plan.layers) and len(rows) == len(routed)
    if routed:
        c, h, w = routed[0]
        assert rows[0]["name"] == "dkres %d>%d>%d k1,k3 @%dx%d" % (c, c // 2, c, h, w)
        assert rows[0]["flops"] == 2.0 * 2 * h * w * (c * c // 2 + 9 * c * c // 2)
        assert rows[0]["bytes"] == 2.0 * (2 * h * w * 2 * c + c * c // 2 + 9 * c * c // 2)


def test_ssdk_dkres_switch(monkeypatch):
    from ssds import _native as N

    monkeypatch.setenv("SSDK_DKRES", "0")
    _, plan, _ = _bare_plan()
    kinds = [L.get("kind") for L in plan.layers]
    assert kinds.count("dkres") == 0 and kinds.count(None) == 1 + 5 + 46
    # the 46 convs in their place: 1x1 then 3x3 with the block input as residual, added behind the activation (res_mode 0)
    pairs = [L for L in plan.layers if L["pack"].kind == "dense" and L["pack"].stride == 1]
    assert len(pairs) == 46 and [L["pack"].k for L in pairs] == [1, 3] * 23
    assert all(L["res"] is None for L in pairs[0::2]) and all(L["res"] is not None and L["res_mode"] == 0 for L in pairs[1::2])
    monkeypatch.setenv("SSDK_DKRES", "1")
    _, plan, _ = _bare_plan()
    want = [r for r in _residuals(96, 64) if N.lib.ssdk_dkres_supported(r[0], r[1], r[2], N.BF16)]
    assert [L.get("kind") for L in plan.layers].count("dkres") == len(want) == 11


def test_every_op_reads_the_value_that_was_recorded_for_it(monkeypatch):
    """The arena hands a buffer out again once its last reader is recorded.  Replaying the recording in order, the last writer of
    every source buffer must have produced the shape the reading op expects, and no op writes a buffer it reads."""
    from ssds.modeling.layers.fused_conv import _out_hw

    def out_shape(L):
        if L.get("kind") == "dkres":
            return (L["pack2"].cout, L["h"], L["w"])
        return (L["pack"].cout,) + _out_hw(L["h"], L["w"], L["pack"].k, L["pack"].stride)

    for env in ("0", "1"):
        monkeypatch.setenv("SSDK_DKRES", env)
        _, plan, outs = _bare_plan()
        holds, checked = {}, 0
        for i, L in enumerate(plan.layers):
            srcs = [(L["x"], (L["pack"].cin, L["h"], L["w"]))]
            if L.get("res") is not None:
                srcs.append((L["res"], out_shape(L)))
            for buf, want in srcs:
                if isinstance(buf, int):
                    assert holds[buf] == want, (env, i, holds[buf], want)
                    assert L["y"] != buf, (env, i)
                    checked += 1
            holds[L["y"]] = out_shape(L)
        assert checked >= 28
        assert [holds[o[0]] for o in outs] == [(512, 6, 4), (1024, 3, 2)]  # the kept maps are never handed out again


def test_planner_refuses_what_the_kernels_do_not_cover():
    from ssds.modeling.layers import fused_conv as FC
    from ssds.modeling.layers import planner
    from ssds.modeling.nets.darknet import DarkNet

    def record(net):
        net = net.eval().to(torch.bfloat16)
        plan = FC.ConvPlan(torch.device("cpu"), torch.bfloat16, (1, 3, 32, 32))
        return planner.record_backbone(plan, plan.input_value(), net)

    net = DarkNet(layers=[1, 1, 1, 1, 1], outputs=[2])
    assert len(record(net)) == 1
    net.block2[1].conv3x3[2] = torch.nn.LeakyReLU(0.1)
    with pytest.raises(planner.PlanUnsupported, match=r"block2\.1\.conv3x3.*ReLU6"):
        record(net)
    net = DarkNet(layers=[1, 1, 1, 1, 1], outputs=[2])
    net.block1[1].conv3x3[0] = torch.nn.Conv2d(32, 64, 3, padding=1, groups=2)
    with pytest.raises(planner.PlanUnsupported, match=r"block1\.1\.conv3x3.*not covered"):
        record(net)
    net = DarkNet(layers=[1, 1, 1, 1, 1], outputs=[2])
    net.block2[0][0] = torch.nn.Conv2d(64, 128, 3, stride=1, padding=1)
    with pytest.raises(planner.PlanUnsupported, match=r"block2\.0.*stride 2"):
        record(net)
    net = DarkNet(layers=[1, 1, 1, 1, 1], outputs=[2])
    net.block1[1] = torch.nn.Identity()
    with pytest.raises(planner.PlanUnsupported, match="Identity has no planner"):
        record(net)
