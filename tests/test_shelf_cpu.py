"""The Shelf detector without a GPU: ``SSDShelf`` (ssds/modeling/ssds/shelf.py) against the outputs of the REFERENCE's own class
on the same seeded weights (tests/golden/net_shelf_*.npz, written by tests/golden/make_golden_shelf.py), its config, the
parity images of the transposed convolution (fused_conv.ConvTPack), the C-ABI of ``ssdk_convt3x3s2`` and the planner's walk.
The kernel itself and the plans are checked on the GPU in tests/test_gpu_convt.py."""
import ctypes
import os
import subprocess

import pytest
import torch
import torch.nn.functional as F

import cases_shelf
import nethelp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "experiments", "cfgs", "shelf_resnet18_513.yml")


def build(name, monkeypatch):
    """nethelp.build (schema, shapes and key order against the fixture, seeded weights, stored BatchNorm statistics) on the
    Shelf cases: their explicit stub maps live in cases_shelf."""
    monkeypatch.setattr(nethelp, "cases", cases_shelf)
    return nethelp.build(name)


# ---- 1. the model ----------------------------------------------------------------------------------------------------------------
def test_reachable_by_name():
    from ssds.modeling import ssds

    cls = getattr(ssds, "SSDShelf")
    from ssds.modeling.ssds.shelf import Head, SharedBlock, ShelfPyramid, SSDShelf

    assert cls is SSDShelf and all(isinstance(c, type) for c in (Head, SharedBlock, ShelfPyramid))


@pytest.fixture(scope="module")
def shipped():
    from ssds.core import config
    from ssds.modeling import model_builder

    cfg = config.cfg_from_file(CFG)
    torch.manual_seed(0)
    return cfg, model_builder.create_model(cfg.MODEL)


def test_shipped_config_builds(shipped):
    from ssds.modeling.ssds.shelf import SSDShelf

    cfg, model = shipped
    assert isinstance(model, SSDShelf) and cfg.MODEL.SSDS == "SSDShelf" and cfg.MODEL.NETS == "ResNet18"
    assert list(cfg.MODEL.IMAGE_SIZE) == [513, 513] and len(model.loc) == len(model.conf) == len(model.transforms) == 5
    assert [n for n, _ in model.shelf_head.named_children()] == ["decoder0", "encoder0", "decoder1"]
    assert model.loc[0][-1].out_channels == 9 * 4 and model.conf[0][-1].out_channels == 9 * 80


def test_anchor_strides_of_the_shipped_config(shipped):
    from ssds.modeling import model_builder

    cfg, model = shipped
    anchors = model_builder.create_anchors(cfg.MODEL, model, cfg.MODEL.IMAGE_SIZE)
    assert list(anchors) == [7, 15, 30, 57, 102]  # W_in // W_conf with maps 65, 33, 17, 9, 5
    assert all(tuple(a.shape) == (9, 4) for a in anchors.values())


@pytest.mark.parametrize("name", list(cases_shelf.NET_CASES))
def test_module_matches_reference_fp32(name, monkeypatch):
    model, x, fx = build(name, monkeypatch)  # (asserts keys, shapes and order of the state_dict against the reference's)
    keys = [str(k) for k in fx["keys"]]
    first = [k for k in keys if k.startswith("shelf_head.")][0]
    assert first == "shelf_head.decoder0.block0.conv1.weight" and keys[keys.index(first) - 1].startswith("transforms.")
    nt = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        with torch.no_grad():
            loc, conf = model(x)
    finally:
        torch.set_num_threads(nt)
    wl, wc = nethelp.want(fx)
    assert len(loc) == len(wl) == 4 and len(conf) == len(wc) == 4
    for i, (l, a, c, b) in enumerate(zip(loc, wl, conf, wc)):
        assert l.shape == a.shape and c.shape == b.shape, (name, i)
        assert float(b.std()) > 0.01 and float(a.abs().max()) > 0.1, (name, i)  # the fixture compares something
        torch.testing.assert_close(l, a, rtol=1e-3, atol=5e-4 * float(a.abs().max()))  # (tolerances of test_nets_golden.py)
        torch.testing.assert_close(c, b, rtol=1e-3, atol=2e-4)


def test_train_mode_returns_logits(monkeypatch):
    model, x, _ = build("shelf_stub", monkeypatch)
    with torch.no_grad():
        _, conf_eval = model(x)
        model.train()
        for m in model.modules():
            if isinstance(m, (torch.nn.BatchNorm2d, torch.nn.Dropout2d)):
                m.eval()
        _, conf_train = model(x)
    for a, b in zip(conf_eval, conf_train):
        torch.testing.assert_close(a, torch.sigmoid(b), rtol=1e-6, atol=1e-7)


def test_even_sized_maps_raise_like_the_reference():
    from ssds.modeling import ssds

    fl = [[0, 1, 2, "Conv:S"], [24, 40, 64, 48]]
    outs, extras, head = ssds.SSDShelf.add_extras(fl, [3] * 4, 4)
    feats = [torch.zeros(1, c, s, s) for c, s in zip((24, 40, 64), (16, 8, 4))]
    model = ssds.SSDShelf(nethelp.StubBackbone(feats), extras, head, 4).eval()
    with pytest.raises(RuntimeError), torch.no_grad():
        model(torch.zeros(1, 3, 8, 8))


def test_initialize_sets_the_class_prior():
    from ssds.modeling import ssds

    outs, extras, head = ssds.SSDShelf.add_extras([[0, 1], [24, 40]], [3, 3], 4)
    model = ssds.SSDShelf(nethelp.StubBackbone([]), extras, head, 4)
    for c in model.conf:
        assert torch.allclose(c[-1].bias, torch.full_like(c[-1].bias, -4.59512))  # -log((1 - pi) / pi), pi = 0.01
    heads = [m for c in model.loc for m in c.modules() if isinstance(m, torch.nn.Conv2d) and m.bias is not None]
    assert len(heads) == 2 and all(float(m.bias.detach().abs().max()) == 0 for m in heads)  # initialize_head


# ---- 2. the parity images ------------------------------------------------------------------------------------------------------
def _unpack(image, rows, k):
    """fragment-major [g][ks][4][16][8] -> the matrix [rows][k] (include/ssdk.h ssdk_weight_frag_bytes, inverted)."""
    g, ks = image.shape[0], image.shape[1]
    mat = image.permute(0, 3, 1, 2, 4).reshape(g * 16, ks * 32)
    assert float(mat[rows:].abs().max() if mat[rows:].numel() else 0) == 0 and float(mat[:, k:].abs().sum()) == 0  # zero padding
    return mat[:rows, :k]


@pytest.mark.parametrize("cin,cout", [(8, 8), (40, 24), (24, 40), (64, 16)])
def test_convtpack_images_round_trip(cin, cout):
    from ssds import _native as N
    from ssds.modeling.layers import fused_conv as FC

    torch.manual_seed(cin * 100 + cout)
    m = torch.nn.ConvTranspose2d(cin, cout, 3, stride=2, padding=1)
    pk = FC.ConvTPack(m, torch.bfloat16)
    w = m.weight.detach().to(torch.bfloat16)
    assert pk.w.numel() * 2 == N.lib.ssdk_convt_pack_bytes(cin, cout) and pk.bias.dtype == torch.float32
    g, off = (cout + 15) // 16, 0
    for cls, (py, px) in enumerate([(0, 0), (0, 1), (1, 0), (1, 1)]):
        taps = FC.convt_class_taps(py, px)
        assert len(taps) == (1 + py) * (1 + px)
        ks = (len(taps) * cin + 31) // 32
        assert g * 16 * ks * 32 * 2 == N.lib.ssdk_weight_frag_bytes(cout, ks * 32)
        image = pk.w[off:off + g * ks * 512].view(g, ks, 4, 16, 8)
        off += g * ks * 512
        mat = _unpack(image, cout, len(taps) * cin)
        for t, (dy, dx, ky, kx) in enumerate(taps):
            assert (ky, kx) == ((2 - 2 * dy) if py else 1, (2 - 2 * dx) if px else 1)
            assert torch.equal(mat[:, t * cin:(t + 1) * cin], w[:, :, ky, kx].t()), (cls, t)  # exactly the weight's slice
    assert off == pk.w.numel()
    assert not FC.ConvTPack.supported(torch.nn.ConvTranspose2d(12, 8, 3, stride=2, padding=1))
    assert not FC.ConvTPack.supported(torch.nn.ConvTranspose2d(8, 8, 3, stride=2, padding=1, output_padding=1))


@pytest.mark.parametrize("h,w", [(5, 4), (1, 3), (3, 1), (1, 1)])
def test_parity_form_is_the_transposed_convolution(h, w):
    """The images and tap offsets the kernel walks, evaluated in fp64 on the host: class (py, px) of the output is one matrix
    product over the (h - py) x (w - px) pixels that have the neighbours it reads -- every tap in range, nothing masked."""
    from ssds.modeling.layers import fused_conv as FC

    torch.manual_seed(h * 10 + w)
    cin, cout, n = 24, 8, 2
    wt = torch.randn(cin, cout, 3, 3, dtype=torch.float64)
    x = torch.randn(n, cin, h, w, dtype=torch.float64)
    want = F.conv_transpose2d(x, wt, stride=2, padding=1)
    assert tuple(want.shape) == (n, cout, 2 * h - 1, 2 * w - 1)
    got = torch.full_like(want, float("nan"))
    for image, (py, px) in zip(FC.convt_parity_images(wt), [(0, 0), (0, 1), (1, 0), (1, 1)]):
        taps = FC.convt_class_taps(py, px)
        mat = _unpack(image, cout, len(taps) * cin)
        hh, ww = h - py, w - px
        if hh == 0 or ww == 0:
            continue
        cols = torch.cat([x[:, :, dy:dy + hh, dx:dx + ww] for dy, dx, _, _ in taps], 1)  # [n, taps * cin, hh, ww]
        got[:, :, py::2, px::2] = torch.einsum("ok,nkhw->nohw", mat, cols)
    assert not torch.isnan(got).any()
    torch.testing.assert_close(got, want, rtol=0, atol=1e-12)


# ---- 3. the C-ABI ----------------------------------------------------------------------------------------------------------------
def test_abi_symbols_and_sizes(tmp_path):
    """The transposed convolution has a header of its own (include/ssdk_convt.h): the entry points of ssdk.h and the layout of
    ssdk_op stay the closed list of ABI 245, and the executor's op kind 7 is described by the op's ssdk_conv_desc."""
    from ssds import _native as N

    assert N.lib.ssdk_version() == 245 and N.ABI_VERSION == 245
    header = open(os.path.join(ROOT, "include", "ssdk_convt.h")).read()
    main = open(os.path.join(ROOT, "include", "ssdk.h")).read()
    assert N.CONVT_EXPORTS == ("ssdk_convt3x3s2", "ssdk_convt_pack_bytes", "ssdk_convt_desc_bytes")
    for name in N.CONVT_EXPORTS:
        assert (name + "(") in header and hasattr(N.lib, name) and getattr(N.lib, name).argtypes is not None, name
        assert name not in N.EXPORTS
    assert N.lib.ssdk_convt3x3s2.argtypes == [ctypes.POINTER(N.ConvTDesc), ctypes.c_void_p]
    assert ctypes.sizeof(N.ConvTDesc) == N.lib.ssdk_convt_desc_bytes()
    assert [f[0] for f in N.ConvTDesc._fields_][:5] == ["x", "w_pack", "bias", "skip", "y"]
    assert N.OP_CONVT == 7 and "SSDK_OP_CONVT = 7" in main and "convt" not in [f[0] for f in N.Op._fields_]
    # ssdk_struct_size keeps its eight indices and ssdk_abi_check accepts the header: sizeof(ssdk_op) did not move
    assert N.lib.ssdk_struct_size(7) == ctypes.sizeof(N.Op) and N.lib.ssdk_struct_size(8) == 0
    assert N.lib.ssdk_abi_check(N.ABI_VERSION, ctypes.sizeof(N.Op)) == 0
    assert N.lib.ssdk_convt_pack_bytes(12, 8) == 0 and N.lib.ssdk_convt_pack_bytes(8, 8) == 4 * 16 * 32 * 2
    # the sizes as a C compiler sees the headers
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include "ssdk_convt.h"\nint main(void) { printf("%zu %zu %d\\n", sizeof(ssdk_convt_desc), '
                   'sizeof(ssdk_op), (int)SSDK_OP_CONVT); return 0; }\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert [int(v) for v in out] == [ctypes.sizeof(N.ConvTDesc), ctypes.sizeof(N.Op), N.OP_CONVT]


def test_bad_arguments_are_refused_before_any_launch():
    from ssds import _native as N

    F0 = 0x1000  # never dereferenced: every call below fails validation first

    def call(**kw):
        d = N.ConvTDesc()
        d.x, d.w_pack, d.bias, d.skip, d.y = F0, F0, F0, F0, F0
        d.N, d.Cin, d.H, d.W, d.Cout, d.act, d.dtype = 2, 16, 5, 4, 24, 0, N.BF16
        for k, v in kw.items():
            setattr(d, k, v)
        rc = N.lib.ssdk_convt3x3s2(ctypes.byref(d), None)
        return rc, N.lib.ssdk_last_error().decode()

    for kw in (dict(Cin=12), dict(x=None), dict(y=F0 + 8), dict(Cout=20), dict(H=0), dict(W=0), dict(N=0), dict(N=65536),
               dict(dtype=N.F32), dict(w_pack=None), dict(y=None), dict(skip=F0 + 2), dict(bias=F0 + 4), dict(act=9)):
        rc, msg = call(**kw)
        assert rc == -1 and msg.startswith("convt3x3s2:"), (kw, rc, msg)
    assert N.lib.ssdk_convt3x3s2(None, None) == -1


# ---- 4. the planner ------------------------------------------------------------------------------------------------------------
def _stub_plan(monkeypatch):
    from ssds.modeling.layers import planner

    model, x, _ = build("shelf_stub", monkeypatch)
    model = model.to(torch.bfloat16)
    feats = [f.to(torch.bfloat16) for f in model.backbone(x)]
    return model, feats, planner.build_shelf_plan(model, feats)


def test_planner_records_one_convt_op_per_decoder_step(monkeypatch):
    from ssds import _native as N

    model, feats, plan = _stub_plan(monkeypatch)
    kinds = [L.get("kind") for L in plan.layers]
    convt = [L for L in plan.layers if L.get("kind") == "convt"]
    assert len(convt) == 4  # two per decoder, two decoders, three levels
    assert [(L["pack"].cin, L["pack"].cout, L["h"], L["w"]) for L in convt] == [(64, 40, 5, 4), (40, 24, 9, 7)] * 2
    assert all(L["res"] is not None for L in convt)
    assert set(kinds) <= {None, "convt", "xpair"}
    # 3 transforms; per pyramid 3 blocks x 2 launches + 2 steps; the Conv:S transform (2); 4 levels x 2 heads x 2 convs
    assert len(plan.layers) - kinds.count("xpair") == 3 + 3 * 8 + (0 if "xpair" in kinds else 2) + 16
    # the two launches of a SharedBlock read ONE weight with the two BatchNorms; the second adds the block input behind a ReLU
    first, second = plan.layers[3], plan.layers[4]
    blk = model.shelf_head.decoder0.block0
    assert torch.equal(first["pack"].w, second["pack"].w) and not torch.equal(first["pack"].bias, second["pack"].bias)
    assert first["res"] is None and second["res"] == plan.layers[3]["x"] and second["res_mode"] == 2 and blk.conv1.in_channels == 64
    ops = [op for op in plan.ops if op.kind == N.OP_CONVT]
    assert len(ops) == 4 and all(op.lane == 0 and op.conv.x and op.conv.y and op.conv.residual and op.conv.w and op.conv.bias
                                 and (op.conv.k, op.conv.stride, op.conv.groups, op.conv.res_mode) == (3, 2, 1, 0)
                                 and op.conv.in_layout == op.conv.out_layout == N.NHWC and not op.conv.scale for op in ops)
    assert [(op.conv.Cin, op.conv.Cout, op.conv.H, op.conv.W) for op in ops] == [(64, 40, 5, 4), (40, 24, 9, 7)] * 2
    rows = [r for r in plan.layer_table() if r["name"].startswith("convt ")]
    assert len(rows) == 4 and all(r["kind"] == "conv" and r["flops"] > 0 and r["bytes"] > 0 for r in rows)
    assert rows[0]["flops"] == 2.0 * 2 * 64 * 40 * (20 + 2 * 15 + 2 * 16 + 4 * 12)
    assert [(h[4], h[5], h[6]) for h in plan.heads] == [(17, 13, "loc"), (17, 13, "conf"), (9, 7, "loc"), (9, 7, "conf"),
                                                        (5, 4, "loc"), (5, 4, "conf"), (3, 2, "loc"), (3, 2, "conf")]


def test_planner_refuses_what_the_kernels_do_not_cover(monkeypatch):
    from ssds.modeling import ssds
    from ssds.modeling.layers import planner

    model, feats, _ = _stub_plan(monkeypatch)
    even = [torch.zeros(1, c, s, s, dtype=torch.bfloat16) for c, s in zip((24, 40, 64), (16, 8, 4))]
    with pytest.raises(planner.PlanUnsupported, match="2h - 1"):
        planner.build_shelf_plan(model, even)
    outs, extras, head = ssds.SSDShelf.add_extras([[0, 1], [12, 24]], [3, 3], 4)  # a width that is no multiple of 8
    narrow = ssds.SSDShelf(nethelp.StubBackbone([]), extras, head, 4).eval().to(torch.bfloat16)
    with pytest.raises(planner.PlanUnsupported):
        planner.build_shelf_plan(narrow, [torch.zeros(1, 12, 9, 9, dtype=torch.bfloat16), torch.zeros(1, 24, 5, 5, dtype=torch.bfloat16)])
