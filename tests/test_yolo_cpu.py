"""The YOLO detectors without a GPU: ``YOLOV3`` / ``YOLOV4`` (ssds/modeling/ssds/yolo.py) against the outputs of the REFERENCE's own
classes on the same seeded weights (tests/golden/net_yolo*.npz, written by tests/golden/make_golden_yolo.py), their two configs, the
C-ABI of ``ssdk_cat2`` / ``ssdk_spp`` (include/ssdk_cat.h) and the planner's walk.  The kernels themselves and the plans are checked
on the GPU in tests/test_gpu_cat.py."""
import ctypes
import os
import subprocess

import pytest
import torch
import torch.nn.functional as F

import cases_yolo
import nethelp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFGS = {"YOLOV3": os.path.join(ROOT, "experiments", "cfgs", "yolov3_resnet18_320.yml"),
        "YOLOV4": os.path.join(ROOT, "experiments", "cfgs", "yolov4_resnet18_512.yml")}
LEVELS = {"yolov3_stub": 4, "yolov4_stub": 4, "yolov3_r18": 3, "yolov4_r18": 4}


def build(name, monkeypatch):
    """nethelp.build (schema, shapes and key order against the fixture, seeded weights, stored BatchNorm statistics) on the YOLO
    cases."""
    monkeypatch.setattr(nethelp, "cases", cases_yolo)
    return nethelp.build(name)


# ---- 1. the models ---------------------------------------------------------------------------------------------------------------
def test_reachable_by_name():
    from ssds.modeling import ssds
    from ssds.modeling.ssds.yolo import PANModule, SPPModule, YOLOV3, YOLOV4

    assert getattr(ssds, "YOLOV3") is YOLOV3 and getattr(ssds, "YOLOV4") is YOLOV4
    assert all(isinstance(c, type) for c in (PANModule, SPPModule))


@pytest.fixture(scope="module", params=["YOLOV3", "YOLOV4"])
def shipped(request):
    from ssds.core import config
    from ssds.modeling import model_builder

    cfg = config.cfg_from_file(CFGS[request.param])
    torch.manual_seed(0)
    return request.param, cfg, model_builder.create_model(cfg.MODEL)


def test_shipped_configs_build_with_strides_8_16_32(shipped):
    from ssds.modeling import model_builder, ssds
    from ssds.modeling.ssds.shelf import Head

    head, cfg, model = shipped
    assert isinstance(model, getattr(ssds, head)) and cfg.MODEL.SSDS == head and cfg.MODEL.NETS == "ResNet18"
    assert cfg.MODEL.NUM_CLASSES == 80 and cfg.TRAIN.BATCH_SIZE == cfg.TEST.BATCH_SIZE == 32
    assert all(isinstance(m, Head) for m in list(model.loc) + list(model.conf))  # bench.py reads m.weight / m.bias of model.conf
    assert all(m.weight is m[-1].weight and m.bias is m[-1].bias for m in model.conf)
    anchors = model_builder.create_anchors(cfg.MODEL, model, cfg.MODEL.IMAGE_SIZE)
    if head == "YOLOV3":
        assert list(cfg.MODEL.IMAGE_SIZE) == [320, 320] and list(anchors) == [8, 16, 32]
        assert [tuple(a.shape) for a in anchors.values()] == [(6, 4), (6, 4), (9, 4)]
        assert [c[-1].out_channels for c in model.conf] == [6 * 80, 6 * 80, 9 * 80]
        assert len(model.transforms) == 2 and len(model.extras) == 3
    else:
        assert list(cfg.MODEL.IMAGE_SIZE) == [512, 512] and list(anchors) == [8, 16, 32, 64]
        assert all(tuple(a.shape) == (9, 4) for a in anchors.values())
        assert len(model.transforms) == 3 and len(model.extras) == 1 and len(model.fpn) == 1
        assert [n for n, _ in model.fpn[0].named_children()] == [
            "top-down-2-to-1", "top-down-1", "top-down-1-to-0", "top-down-0",
            "bottom-up-0-to-1", "bottom-up-1", "bottom-up-1-to-2", "bottom-up-2"]


@pytest.mark.parametrize("name", list(cases_yolo.NET_CASES))
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
    assert isinstance(loc, tuple) and isinstance(conf, tuple)
    assert len(loc) == len(wl) == LEVELS[name] and len(conf) == len(wc) == LEVELS[name]
    for i, (l, a, c, b) in enumerate(zip(loc, wl, conf, wc)):
        assert l.shape == a.shape and c.shape == b.shape, (name, i)
        assert float(b.std()) > 0.01 and float(a.abs().max()) > 0.1, (name, i)  # the fixture compares something
        torch.testing.assert_close(l, a, rtol=1e-3, atol=5e-4 * float(a.abs().max()))  # (tolerances of test_nets_golden.py)
        torch.testing.assert_close(c, b, rtol=1e-3, atol=2e-4)


@pytest.mark.parametrize("name", list(cases_yolo.NET_CASES))
def test_train_mode_returns_logits_and_backward_reaches_every_parameter(name, monkeypatch):
    model, x, _ = build(name, monkeypatch)
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


@pytest.mark.parametrize("head", ["YOLOV3", "YOLOV4"])
def test_maps_that_are_not_exact_halves_raise_like_the_reference(head):
    from ssds.modeling import ssds

    cls = getattr(ssds, head)
    outs, extras, hd = cls.add_extras([[0, 1, 2, "Conv:S"], [32, 64, 128, 64]], [3] * 4, 4)
    feats = [torch.zeros(1, c, h, w) for c, (h, w) in zip((32, 64, 128), ((17, 13), (9, 7), (5, 4)))]
    model = cls(nethelp.StubBackbone(feats), extras, hd, 4).eval()
    with pytest.raises(RuntimeError), torch.no_grad():
        model(torch.zeros(1, 3, 8, 8))


@pytest.mark.parametrize("head", ["YOLOV3", "YOLOV4"])
def test_unknown_layer_string_is_a_value_error(head):
    from ssds.modeling import ssds

    with pytest.raises(ValueError, match="YOLO"):
        getattr(ssds, head).add_extras([[0, 1, "Conv:S", "SepConv:S"], [32, 64, 64, 64]], [3] * 4, 4)


@pytest.mark.parametrize("head", ["YOLOV3", "YOLOV4"])
def test_two_element_depth_and_stack_count(head):
    """The reference's ``add_extras`` behaviours: YOLOv3 takes ``[in, out]`` depths; YOLOv4's third element stacks PAN modules."""
    from ssds.modeling import ssds
    from ssds.modeling.ssds.yolo import PANModule

    if head == "YOLOV3":
        outs, (tr, ex), (loc, conf) = ssds.YOLOV3.add_extras([[0, 1], [[32, 24], [64, 40]]], [3, 3], 4)
        assert outs == [0, 1] and tr[0][0].in_channels == 40 and tr[0][0].out_channels == 16
        assert ex[0][0].in_channels == 48 and ex[0][3].out_channels == 24 and ex[1][0].in_channels == 64 and ex[1][3].out_channels == 40
        assert [h[-1].in_channels for h in loc] == [24, 40]
    else:
        for fl, want in (([[0, 1], [32, 64]], 1), ([[0, 1], [32, 64], 3], 3)):
            _, (tr, ex, fpn), _ = ssds.YOLOV4.add_extras(fl, [3, 3], 4)
            assert len(fpn) == want and all(isinstance(m, PANModule) and m.levels == 2 for m in fpn)


@pytest.mark.parametrize("head", ["YOLOV3", "YOLOV4"])
def test_initialize_sets_the_class_prior(head):
    from ssds.modeling import ssds

    cls = getattr(ssds, head)
    outs, extras, hd = cls.add_extras([[0, 1], [32, 64]], [3, 3], 4)
    model = cls(nethelp.StubBackbone([]), extras, hd, 4)
    for c in model.conf:
        assert torch.allclose(c[-1].bias, torch.full_like(c[-1].bias, -4.59512))  # -log((1 - pi) / pi), pi = 0.01
    heads = [m for c in model.loc for m in c.modules() if isinstance(m, torch.nn.Conv2d) and m.bias is not None]
    assert len(heads) == 2 and all(float(m.bias.detach().abs().max()) == 0 for m in heads)  # initialize_head


@pytest.mark.parametrize("shape", [(2, 8, 4, 3), (1, 16, 13, 13), (1, 8, 16, 20), (3, 8, 1, 1)])
def test_spp_module_is_the_max_pool_expression(shape):
    from ssds.modeling.ssds.yolo import SPPModule

    torch.manual_seed(sum(shape))
    x = torch.randn(shape).clamp(max=2.5) - 3.0  # negative throughout: a padding value of 0 would win
    want = torch.cat([x] + [F.max_pool2d(x, k, stride=1, padding=k // 2) for k in (5, 9, 13)], 1)
    got = SPPModule(3)(x)
    assert torch.equal(got, want) and float(got.max()) < 0
    avg = SPPModule(2, pool_type="avg_pool")(x)
    assert torch.equal(avg, torch.cat([x] + [F.avg_pool2d(x, k, stride=1, padding=k // 2) for k in (5, 9)], 1))
    assert not list(SPPModule(3).parameters())


# ---- 2. the C-ABI ----------------------------------------------------------------------------------------------------------------
def test_abi_symbols_and_sizes(tmp_path):
    """The concatenation and the SPP block have a header of their own (include/ssdk_cat.h): the entry points of ssdk.h and the
    layout of ssdk_op stay the closed list of ABI 245, and executor op kinds 8 / 9 are described by the op's ssdk_conv_desc."""
    from ssds import _native as N

    assert N.lib.ssdk_version() == 245 and N.ABI_VERSION == 245 and len(N.EXPORTS) == 127
    header = open(os.path.join(ROOT, "include", "ssdk_cat.h")).read()
    main = open(os.path.join(ROOT, "include", "ssdk.h")).read()
    assert N.CAT_EXPORTS == ("ssdk_cat2", "ssdk_cat_desc_bytes", "ssdk_spp", "ssdk_spp_desc_bytes")
    for name in N.CAT_EXPORTS:
        assert (name + "(") in header and hasattr(N.lib, name) and getattr(N.lib, name).argtypes is not None, name
        assert name not in N.EXPORTS and (name + "(") not in main
    assert N.lib.ssdk_cat2.argtypes == [ctypes.POINTER(N.CatDesc), ctypes.c_void_p]
    assert N.lib.ssdk_spp.argtypes == [ctypes.POINTER(N.SppDesc), ctypes.c_void_p]
    assert ctypes.sizeof(N.CatDesc) == N.lib.ssdk_cat_desc_bytes() and ctypes.sizeof(N.SppDesc) == N.lib.ssdk_spp_desc_bytes()
    assert [f[0] for f in N.CatDesc._fields_][:3] == ["a", "b", "y"] and [f[0] for f in N.SppDesc._fields_][:2] == ["x", "y"]
    assert (N.OP_CAT, N.OP_SPP) == (8, 9) and "SSDK_OP_CAT = 8, SSDK_OP_SPP = 9" in main
    assert [f[0] for f in N.Op._fields_] == ["kind", "lane", "conv", "mb", "fuse", "stem", "pool", "xpair", "mbse"]
    # ssdk_struct_size keeps its eight indices and ssdk_abi_check accepts the header: sizeof(ssdk_op) did not move
    assert N.lib.ssdk_struct_size(7) == ctypes.sizeof(N.Op) and N.lib.ssdk_struct_size(8) == 0
    assert N.lib.ssdk_abi_check(N.ABI_VERSION, ctypes.sizeof(N.Op)) == 0
    # the sizes as a C compiler sees the headers
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include "ssdk_cat.h"\nint main(void) { printf("%zu %zu %zu %d %d\\n", sizeof(ssdk_cat_desc), '
                   'sizeof(ssdk_spp_desc), sizeof(ssdk_op), (int)SSDK_OP_CAT, (int)SSDK_OP_SPP); return 0; }\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert [int(v) for v in out] == [ctypes.sizeof(N.CatDesc), ctypes.sizeof(N.SppDesc), ctypes.sizeof(N.Op), N.OP_CAT, N.OP_SPP]


F0 = 0x1000  # never dereferenced: every call below fails validation first


def _cat(**kw):
    from ssds import _native as N

    d = N.CatDesc()
    d.a, d.b, d.y = F0, F0, F0
    d.N, d.H, d.W, d.C1, d.C2, d.mode, d.dtype = 2, 6, 4, 16, 24, N.FUSE_UP2, N.BF16
    for k, v in kw.items():
        setattr(d, k, v)
    rc = N.lib.ssdk_cat2(ctypes.byref(d), None)
    return rc, N.lib.ssdk_last_error().decode()


def _spp(**kw):
    from ssds import _native as N

    d = N.SppDesc()
    d.x, d.y = F0, F0
    d.N, d.H, d.W, d.C, d.dtype = 2, 5, 4, 16, N.F16
    for k, v in kw.items():
        setattr(d, k, v)
    rc = N.lib.ssdk_spp(ctypes.byref(d), None)
    return rc, N.lib.ssdk_last_error().decode()


def test_bad_arguments_are_refused_before_any_launch():
    """No device is needed: each call is refused by the argument checks, with a message that names the entry point."""
    from ssds import _native as N

    for kw in (dict(C1=12), dict(H=5), dict(y=None), dict(dtype=N.F32), dict(a=F0 + 8),  # the issue's five
               dict(C2=20), dict(W=3), dict(b=None), dict(a=None), dict(b=F0 + 2), dict(y=F0 + 4), dict(N=0), dict(H=0), dict(C2=0),
               dict(mode=N.FUSE_POOL2), dict(N=1 << 16, H=1 << 10, W=1 << 10)):
        rc, msg = _cat(**kw)
        assert rc == -1 and msg.startswith("cat2:"), (kw, rc, msg)
    rc, msg = _cat(H=5, mode=N.FUSE_SAME, y=None)  # odd sizes are fine at the same size: the refusal is the NULL y
    assert rc == -1 and "null" in msg
    for kw in (dict(C=4), dict(C=12), dict(y=None), dict(x=None), dict(dtype=N.F32), dict(x=F0 + 8), dict(y=F0 + 8), dict(H=0),
               dict(W=0), dict(N=0), dict(N=1 << 16, H=1 << 10, W=1 << 10)):
        rc, msg = _spp(**kw)
        assert rc == -1 and msg.startswith("spp:"), (kw, rc, msg)
    assert N.lib.ssdk_cat2(None, None) == -1 and N.lib.ssdk_spp(None, None) == -1


# ---- 3. the planner --------------------------------------------------------------------------------------------------------------
def _stub_plan(name, monkeypatch):
    from ssds.modeling.layers import planner

    model, x, _ = build(name, monkeypatch)
    model = model.to(torch.bfloat16)
    feats = [f.to(torch.bfloat16) for f in model.backbone(x)]
    builder = planner.build_yolov3_plan if name.startswith("yolov3") else planner.build_yolov4_plan
    return model, feats, builder(model, feats)


def _check_ops(plan, cats, spps):
    from ssds import _native as N

    kinds = [L.get("kind") for L in plan.layers]
    assert kinds.count("cat") == len(cats) and kinds.count("spp") == len(spps)
    assert set(kinds) <= {None, "cat", "spp", "xpair"}
    got = [(L["c1"], L["c2"], L["h"], L["w"], L["up2"]) for L in plan.layers if L.get("kind") == "cat"]
    assert got == cats, got
    ops = [op for op in plan.ops if op.kind == N.OP_CAT]
    assert [(op.conv.Cin, op.conv.Cout - op.conv.Cin, op.conv.H, op.conv.W, bool(op.conv.res_mode & 1)) for op in ops] == cats
    patched = {(i, field) for i, field, _ in plan.patches}  # (a source that is an external input gets its address per run)
    for i, op in enumerate(plan.ops):
        if op.kind not in (N.OP_CAT, N.OP_SPP):
            continue
        c = op.conv
        assert op.lane == 0 and c.y and (c.x or (i, "conv.x") in patched) and not (c.w or c.scale or c.bias or c.y2 or c.w_frag)
        assert c.in_layout == c.out_layout == N.NHWC and c.stride == 1 and c.act == N.ACT["none"] and c.dtype == N.BF16
        if op.kind == N.OP_CAT:
            assert c.k == 1 and (c.residual or (i, "conv.residual") in patched)
        else:
            assert c.k == 5 and not c.residual and c.res_mode == 0
    sops = [op for op in plan.ops if op.kind == N.OP_SPP]
    assert [(op.conv.Cin, op.conv.Cout, op.conv.H, op.conv.W) for op in sops] == [(c, 4 * c, h, w) for c, h, w in spps]
    table = plan.layer_table()
    assert len(table) == len(plan.layers)
    rows = [r for r in table if r["name"].startswith(("cat ", "spp "))]
    assert len(rows) == len(cats) + len(spps) and all(r["flops"] == 0 and r["bytes"] > 0 for r in rows)
    return rows


def test_planner_records_two_cat_ops_for_yolov3(monkeypatch):
    model, feats, plan = _stub_plan("yolov3_stub", monkeypatch)
    # top-down: 8x6 takes 64 backbone channels + 32 upsampled from 4x3; 16x12 takes 32 + 16 from 8x6
    rows = _check_ops(plan, [(64, 32, 8, 6, True), (32, 16, 16, 12, True)], [])
    assert rows[0]["name"] == "cat 64+32 up2 @8x6"
    assert rows[0]["bytes"] == 2.0 * 2 * (8 * 6 * 64 + 4 * 3 * 32 + 8 * 6 * 96)  # both sources and the output once
    assert [(h[4], h[5], h[6]) for h in plan.heads] == [(16, 12, "loc"), (16, 12, "conf"), (8, 6, "loc"), (8, 6, "conf"),
                                                        (4, 3, "loc"), (4, 3, "conf"), (2, 2, "loc"), (2, 2, "conf")]
    # the 'Conv:S' extra reads the RAW last backbone map: an external input of the plan, 128 channels at 4x3
    extra = [L for L in plan.layers if L.get("kind") is None and L["pack"].stride == 2]
    assert len(extra) == 1 and extra[0]["pack"].cin == 128 and (extra[0]["h"], extra[0]["w"]) == (4, 3)
    assert extra[0]["x"] is plan.inputs[2]


def test_planner_records_eight_cat_ops_and_one_spp_op_for_yolov4(monkeypatch):
    model, feats, plan = _stub_plan("yolov4_stub", monkeypatch)
    stack = [(32, 32, 8, 6, True), (16, 16, 16, 12, True), (32, 32, 8, 6, False), (64, 64, 4, 3, False)]
    rows = _check_ops(plan, stack * 2, [(64, 4, 3)])  # two PAN stacks; SPP on the 4x3 map behind the 128 -> 64 transform
    assert [r["name"] for r in rows][:3] == ["spp 64 k5,9,13 @4x3", "cat 32+32 up2 @8x6", "cat 16+16 up2 @16x12"]
    assert rows[0]["bytes"] == 2.0 * 2 * 4 * 3 * 5 * 64
    assert [(h[4], h[5], h[6]) for h in plan.heads] == [(16, 12, "loc"), (16, 12, "conf"), (8, 6, "loc"), (8, 6, "conf"),
                                                        (4, 3, "loc"), (4, 3, "conf"), (2, 2, "loc"), (2, 2, "conf")]


def test_every_op_reads_the_value_that_was_recorded_for_it(monkeypatch):
    """The arena hands a buffer out again once its last reader is recorded.  Replaying the recording in order, the last writer of
    every source buffer must have produced the shape the reading op expects (the values that could be confused in these necks
    differ in channel count or map size), and no op writes a buffer it reads."""
    from ssds.modeling.layers.fused_conv import _out_hw

    def out_shape(L):
        if L.get("kind") == "cat":
            return (L["c1"] + L["c2"], L["h"], L["w"])
        if L.get("kind") == "spp":
            return (4 * L["ch"], L["h"], L["w"])
        if L.get("kind") == "xpair":
            return (L["pack2"].cout,) + _out_hw(L["h"], L["w"], 3, 2)
        return (L["pack"].cout,) + _out_hw(L["h"], L["w"], L["pack"].k, L["pack"].stride)

    def sources(L):
        if L.get("kind") == "cat":
            half = (L["h"] // 2, L["w"] // 2) if L["up2"] else (L["h"], L["w"])
            return [(L["x"], (L["c1"], L["h"], L["w"])), (L["b"], (L["c2"],) + half)]
        cin = L["ch"] if L.get("kind") == "spp" else L["pack"].cin
        return [(L["x"], (cin, L["h"], L["w"]))]

    for name in ("yolov3_stub", "yolov4_stub"):
        model, feats, plan = _stub_plan(name, monkeypatch)
        holds, checked = {}, 0
        for i, L in enumerate(plan.layers):
            for buf, want in sources(L):
                if isinstance(buf, int):
                    assert holds[buf] == want, (name, i, holds[buf], want)
                    assert L.get("y") != buf, (name, i)
                    checked += 1
            if L.get("y") is not None:
                holds[L["y"]] = out_shape(L)
        assert checked > 20


def test_planner_refuses_what_the_kernels_do_not_cover(monkeypatch):
    from ssds.modeling import ssds
    from ssds.modeling.layers import planner
    from ssds.modeling.ssds.yolo import SPPModule

    odd = [torch.zeros(1, c, h, w, dtype=torch.bfloat16) for c, (h, w) in zip((32, 64, 128), ((17, 13), (9, 7), (5, 4)))]
    model, feats, _ = _stub_plan("yolov3_stub", monkeypatch)
    with pytest.raises(planner.PlanUnsupported, match="exact halves"):
        planner.build_yolov3_plan(model, odd)
    model4, feats4, _ = _stub_plan("yolov4_stub", monkeypatch)
    with pytest.raises(planner.PlanUnsupported, match="exact halves"):
        planner.build_yolov4_plan(model4, odd)
    model4.transforms[2][1] = SPPModule(3, pool_type="avg_pool")
    with pytest.raises(planner.PlanUnsupported, match="avg_pool"):
        planner.build_yolov4_plan(model4, feats4)
    # widths the concatenation kernel does not take: 24 // 2 = 12 channels from the level below (every convolution before it is
    # covered: 64 -> 24 -> 48 on the last level, 48 -> 12 as the transform)
    outs, extras, head = ssds.YOLOV3.add_extras([[0, 1], [[24, 16], [64, 48]]], [3, 3], 4)
    narrow = ssds.YOLOV3(nethelp.StubBackbone([]), extras, head, 4).eval().to(torch.bfloat16)
    with pytest.raises(planner.PlanUnsupported, match="multiples of 8"):
        planner.build_yolov3_plan(narrow, [torch.zeros(1, 24, 8, 8, dtype=torch.bfloat16), torch.zeros(1, 64, 4, 4, dtype=torch.bfloat16)])
