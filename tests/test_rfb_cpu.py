"""The RFB extra layers without a GPU: the parser's "RBF" / "RBF:S" strings, ``BasicRFB`` (ssds/modeling/layers/rfb_layers.py) against
the outputs of the REFERENCE's own class on the same seeded weights (tests/golden/rfb_blocks.npz, net_*rfb*.npz, rfb_state_keys.txt,
written by tests/golden/make_golden_rfb.py), the two configs, ``conv_kind``'s new 'dilated', the weight image of the dilated kernel,
the C-ABI of include/ssdk_dconv.h (predicate, refusals before any device call) and the planner's walk recorded on the CPU device.
The kernel itself and the plans are checked on the GPU in tests/test_gpu_rfb.py."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch
import torch.nn as nn

import cases_rfb
import nethelp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
CFGS = {"ssd_resnet18_rfb_512.yml": ("SSD", [512, 512], 6), "shelf_resnet18_rfb_513.yml": ("SSDShelf", [513, 513], 5)}


def build(name, monkeypatch):
    """nethelp.build (schema, shapes and key order against the fixture, seeded weights, stored BatchNorm statistics) on the RFB cases."""
    monkeypatch.setattr(nethelp, "cases", cases_rfb)
    return nethelp.build(name)


def make_block(name):
    """The block of cases_rfb.BLOCK_CASES[name] in eval mode with the seeded weights and the fixture's BatchNorm statistics
    -> (block, input, the reference's fp32 output)."""
    from ssds.modeling.layers.rfb_layers import BasicRFB

    fx = np.load(os.path.join(GOLD, "rfb_blocks.npz"))
    seed, cin, cout, stride, scale, visual, _ = cases_rfb.BLOCK_CASES[name]
    blk = BasicRFB(cin, cout, stride=stride, scale=scale, visual=visual)
    spec = [(k, tuple(v.shape)) for k, v in blk.state_dict().items()]
    state = cases_rfb.seeded_state(spec, seed)
    for k in list(state):
        if name + "/bn/" + k in fx:
            state[k] = fx[name + "/bn/" + k]
    blk.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in state.items()})
    return blk.eval(), torch.from_numpy(cases_rfb.block_input(name)), torch.from_numpy(fx[name + "/y"])


# ---- 1. parser and modules ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layer,stride", [("RBF", 1), ("RBF:S", 2)])
def test_parser_returns_one_block(layer, stride):
    from ssds.modeling.layers.layers_parser import parse_feature_layer
    from ssds.modeling.layers.rfb_layers import BasicConv, BasicRFB

    mods = parse_feature_layer(layer, 256, 128)
    assert len(mods) == 1 and type(mods[0]) is BasicRFB
    blk = mods[0]
    assert blk.scale == 1.0 and blk.out_channels == 128
    assert blk.branch0[1].conv.stride == (stride, stride) and blk.branch1[2].conv.stride == (stride, stride)
    assert blk.shortcut.conv.stride == (stride, stride) and blk.branch1[1].conv.stride == (1, 1)
    assert (blk.branch0[2].conv.dilation, blk.branch0[2].conv.padding) == ((3, 3), (3, 3))
    assert (blk.branch1[3].conv.dilation, blk.branch1[3].conv.padding) == ((5, 5), (5, 5))
    assert [m.conv.out_channels for m in blk.branch0] == [32, 64, 64] and [m.conv.out_channels for m in blk.branch1] == [32, 48, 64, 64]
    assert all(isinstance(m, BasicConv) for m in list(blk.branch0) + list(blk.branch1) + [blk.ConvLinear, blk.shortcut])
    bns = [m for m in blk.modules() if isinstance(m, nn.BatchNorm2d)]
    assert len(bns) == 9 and all(m.eps == 1e-5 and m.momentum == 0.01 for m in bns)
    assert blk.branch0[2].relu is None and blk.branch1[3].relu is None and blk.ConvLinear.relu is None and blk.shortcut.relu is None
    with pytest.raises(AssertionError):
        parse_feature_layer("RFB", 256, 128)  # the reference's spelling is "RBF"


def test_constructor_defaults_are_the_references():
    from ssds.modeling.layers.rfb_layers import BasicConv, BasicRFB

    blk = BasicRFB(128, 64)
    assert blk.scale == 0.1 and blk.branch0[2].conv.dilation == (2, 2) and blk.branch1[3].conv.dilation == (3, 3)
    bc = BasicConv(8, 16, 3, padding=1, bn=False, relu=False, bias=True)
    assert bc.bn is None and bc.relu is None and bc.conv.bias is not None and bc.out_channels == 16


def test_state_dict_is_the_references():
    from ssds.modeling.layers.rfb_layers import BasicRFB

    cin, cout, stride, scale, visual = cases_rfb.STATE_KEYS_BLOCK
    want = []
    for line in open(os.path.join(GOLD, "rfb_state_keys.txt")).read().splitlines():
        key, _, shape = line.partition(" ")
        want.append((key, tuple(int(v) for v in shape.split(",")) if shape else ()))
    blk = BasicRFB(cin, cout, stride=stride, scale=scale, visual=visual)
    assert [(k, tuple(v.shape)) for k, v in blk.state_dict().items()] == want
    assert want[0][0] == "branch0.0.conv.weight" and any(k.startswith("ConvLinear.") for k, _ in want)
    assert any(k.startswith("shortcut.") for k, _ in want)
    state = {k: torch.from_numpy(v) for k, v in cases_rfb.seeded_state(want, 5).items()}
    blk.load_state_dict(state, strict=True)  # a reference-shaped state loads strictly
    assert torch.equal(blk.branch1[3].conv.weight, state["branch1.3.conv.weight"])


@pytest.mark.parametrize("name", list(cases_rfb.BLOCK_CASES))
def test_block_matches_reference_fp32(name):
    blk, x, want = make_block(name)
    with torch.no_grad():
        y = blk(x)
    assert y.shape == want.shape and float(want.std()) > 0.1 and 0.05 < float((want == 0).float().mean()) < 0.95
    torch.testing.assert_close(y, want, rtol=1e-3, atol=5e-4 * float(want.abs().max()))


def test_the_block_fixture_has_a_scaled_block():
    assert any(c[4] != 1.0 for c in cases_rfb.BLOCK_CASES.values()) and any(c[6][1:] == (1, 1) for c in cases_rfb.BLOCK_CASES.values())


@pytest.mark.parametrize("name", list(cases_rfb.NET_CASES))
def test_module_matches_reference_fp32(name, monkeypatch):
    from ssds.modeling.layers.rfb_layers import BasicRFB

    model, x, fx = build(name, monkeypatch)  # (asserts keys, shapes and order of the state_dict against the reference's)
    fl = cases_rfb.NET_CASES[name][3]
    assert sum(isinstance(m, BasicRFB) for m in model.modules()) == sum(isinstance(s, str) and s.startswith("RBF") for s in fl[0]) > 0
    nt = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        with torch.no_grad():
            loc, conf = model(x)
    finally:
        torch.set_num_threads(nt)
    wl, wc = nethelp.want(fx)
    assert len(loc) == len(wl) == len(fl[0]) and len(conf) == len(wc)
    for i, (l, a, c, b) in enumerate(zip(loc, wl, conf, wc)):
        assert l.shape == a.shape and c.shape == b.shape, (name, i)
        assert float(b.std()) > 0.01 and float(a.abs().max()) > 0.1, (name, i)  # the fixture compares something
        torch.testing.assert_close(l, a, rtol=1e-3, atol=5e-4 * float(a.abs().max()))  # (tolerances of test_yolo_cpu.py)
        torch.testing.assert_close(c, b, rtol=1e-3, atol=2e-4)


def test_the_stub_case_ends_below_the_dilation():
    """ssd_rfb_stub: a stride-1 block, odd maps, and a last RFB level smaller than dilation 3 both ways (centre taps only)."""
    fx = nethelp.load_fixture("ssd_rfb_stub")
    sizes = [tuple(fx["loc%d" % i].shape[-2:]) for i in range(5)]
    assert sizes == [(7, 5), (7, 5), (4, 3), (2, 2), (1, 1)]
    fl = cases_rfb.NET_CASES["ssd_rfb_stub"][3]
    assert fl[0][1:] == ["RBF", "RBF:S", "RBF:S", "Conv:S"] and all(c % 128 == 0 for c in fl[1][:3])


@pytest.mark.parametrize("cfg_name", sorted(CFGS))
def test_shipped_configs_build(cfg_name):
    from ssds.core import config
    from ssds.modeling import model_builder, ssds
    from ssds.modeling.layers.rfb_layers import BasicRFB

    head, size, levels = CFGS[cfg_name]
    config.reset_cfg()
    cfg = config.cfg_from_file(os.path.join(ROOT, "experiments", "cfgs", cfg_name))
    torch.manual_seed(0)
    model = model_builder.create_model(cfg.MODEL)
    assert type(model) is getattr(ssds, head) and cfg.MODEL.NETS == "ResNet18" and list(cfg.MODEL.IMAGE_SIZE) == size
    assert len(model.loc) == len(model.conf) == levels
    blocks = [m for m in model.modules() if isinstance(m, BasicRFB)]
    assert len(blocks) == 2 and all(b.scale == 1.0 and b.shortcut.conv.stride == (2, 2) for b in blocks)
    assert all(b.shortcut.conv.in_channels % 128 == 0 for b in blocks)
    config.reset_cfg()


# ---- 2. conv_kind and the weight image -----------------------------------------------------------------------------------------------
def test_conv_kind_dilated():
    from ssds import _native as N
    from ssds.modeling.layers import fused_conv as FC

    C = nn.Conv2d
    for d in range(N.DCONV_MIN_DILATION, N.DCONV_MAX_DILATION + 1):
        for cin, cout in ((8, 8), (16, 24), (40, 24), (128, 128), (64, 136), (1024, 1024)):
            assert FC.conv_kind(C(cin, cout, 3, 1, d, dilation=d, bias=False)) == "dilated", (d, cin, cout)
    assert FC.conv_kind(C(16, 16, 3, 1, 3, dilation=3, bias=True)) == "dilated"
    none = [
        C(16, 16, 3, 2, 3, dilation=3),                          # stride 2
        C(16, 16, 3, 1, 1, dilation=3),                          # padding != dilation
        C(16, 16, 3, 1, 2, dilation=3),
        C(16, 16, 3, 1, (3, 2), dilation=(3, 2)),                # two dilations
        C(16, 16, 3, 1, 3, dilation=3, groups=2),                # grouped
        C(16, 16, 3, 1, 3, dilation=3, groups=16),               # depthwise
        C(16, 16, 3, 1, 9, dilation=9),                          # d outside the predicate
        C(16, 16, 3, 1, 16, dilation=16),
        C(12, 16, 3, 1, 3, dilation=3),                          # Cin % 8
        C(16, 12, 3, 1, 3, dilation=3),                          # Cout % 8
        C(2048, 16, 3, 1, 3, dilation=3),                        # wider than the predicate takes
        C(16, 16, 3, 1, 3, dilation=3, padding_mode="reflect"),
        C(16, 16, 1, 1, 0, dilation=3),                          # 1x1
        C(16, 16, 5, 1, 6, dilation=3),                          # 5x5
    ]
    for conv in none:
        assert FC.conv_kind(conv) is None, conv
        with pytest.raises(N.SsdkError):
            FC.ConvPack(conv, None, "none", torch.bfloat16)
    unchanged = [
        (C(16, 16, 3, 1, 1), "dense"), (C(16, 32, 1), "dense"), (C(16, 16, 3, 2, 1), "dense"), (C(3, 32, 3, 2, 1), "stem"),
        (C(16, 16, 3, 1, 1, groups=16), "dw"), (C(64, 64, 3, 1, 1, groups=4), "g16"), (C(48, 48, 3, 1, 1, groups=2), "gany"),
        (C(12, 16, 3, 1, 1), None), (C(16, 16, 3, 1, 0), None), (C(16, 16, 5, 1, 2), None), (C(16, 16, 3, 1, 1, dilation=1), "dense"),
    ]
    for conv, want in unchanged:
        assert FC.conv_kind(conv) == want, conv
    # no site that asks for 'dense' takes a dilated layer
    assert FC.conv_kind(C(16, 16, 3, 1, 2, dilation=2)) != "dense"


def _unpack(image, rows, k):
    """fragment-major [g][ks][4][16][8] -> the matrix [rows][k] (include/ssdk.h ssdk_weight_frag_bytes, inverted)."""
    g, ks = image.shape[0], image.shape[1]
    mat = image.permute(0, 3, 1, 2, 4).reshape(g * 16, ks * 32)
    assert float(mat[rows:].abs().max() if mat[rows:].numel() else 0) == 0 and float(mat[:, k:].abs().sum()) == 0  # zero padding
    return mat[:rows, :k]


@pytest.mark.parametrize("cin,cout", [(8, 8), (40, 24), (16, 40), (64, 136)])
def test_dfrag_is_the_layout_definition(cin, cout):
    from ssds import _native as N
    from ssds.modeling.layers import fused_conv as FC

    torch.manual_seed(cin * 100 + cout)
    conv = nn.Conv2d(cin, cout, 3, 1, 3, dilation=3, bias=False)
    pk = FC.ConvPack(conv, None, "none", torch.bfloat16)
    assert pk.kind == "dilated" and pk.dilation == 3 and isinstance(pk.dilation, int) and pk.frag() is None
    assert FC.ConvPack(nn.Conv2d(cin, cout, 3, 1, 1), None, "none", torch.bfloat16).dilation == 1
    img = pk.dfrag()
    ks, g = (9 * cin + 31) // 32, (cout + 15) // 16
    assert tuple(img.shape) == (g, ks, 4, 16, 8) and img.dtype == torch.bfloat16 and img.is_contiguous()
    assert img.numel() * 2 == N.lib.ssdk_weight_frag_bytes(cout, ks * 32)
    assert pk.dfrag() is img  # cached
    w = conv.weight.detach().to(torch.bfloat16)  # [co][ci][ky][kx]
    # element by element: frag[g][ks][fg][fr][j] = W[16 g + fr][32 ks + 8 fg + j], W[co][(3 ky + kx) Cin + ci] = w[co][ci][ky][kx]
    flat = img.reshape(-1)
    for co in range(g * 16):
        for k in range(ks * 32):
            got = float(flat[(((co // 16) * ks + k // 32) * 4 + (k % 32) // 8) * 128 + (co % 16) * 8 + k % 8])
            tap, ci = divmod(k, cin)
            want = float(w[co, ci, tap // 3, tap % 3]) if co < cout and tap < 9 else 0.0
            if got != want:
                raise AssertionError((co, k, got, want))
    mat = _unpack(img, cout, 9 * cin)
    assert torch.equal(mat, w.permute(0, 2, 3, 1).reshape(cout, 9 * cin))
    if (9 * cin) % 32:
        assert ks * 32 > 9 * cin  # zero columns behind 9 Cin (checked by _unpack)


# ---- 3. the C-ABI --------------------------------------------------------------------------------------------------------------------
def test_abi_symbols_and_header(tmp_path):
    from ssds import _native as N

    assert N.lib.ssdk_version() == 245 and N.ABI_VERSION == 245
    header = open(os.path.join(ROOT, "include", "ssdk_dconv.h")).read()
    main = open(os.path.join(ROOT, "include", "ssdk.h")).read()
    assert N.DCONV_EXPORTS == ("ssdk_dconv3x3", "ssdk_dconv3x3_supported") and N.DCONV_HEADER_PATH.endswith("ssdk_dconv.h")
    for name in N.DCONV_EXPORTS:
        assert (name + "(") in header and hasattr(N.lib, name) and getattr(N.lib, name).argtypes is not None, name
        assert name not in N.EXPORTS and (name + "(") not in main  # (ssdk.h only mentions it in a comment)
    # (ssdk_conv_desc is ssdk.h's struct: to the parser of this header alone it is an opaque pointer, byref(ConvDesc) passes as one)
    assert N.lib.ssdk_dconv3x3.argtypes == [ctypes.c_void_p, ctypes.c_void_p] and N.lib.ssdk_dconv3x3.restype is ctypes.c_int
    assert N.lib.ssdk_dconv3x3_supported.argtypes == [ctypes.c_int] * 6
    assert (N.CONV_DILATION_SHIFT, N.CONV_DILATION_MASK) == (8, 0xF00) and "bits 8-11" in main and "ssdk_dconv.h" in main
    assert N.lib.ssdk_struct_size(7) == ctypes.sizeof(N.Op) and N.lib.ssdk_abi_check(N.ABI_VERSION, ctypes.sizeof(N.Op)) == 0
    assert (N.DCONV_TILE_PIXELS, N.DCONV_FRAG_COUT, N.DCONV_TILE_COUT, N.DCONV_KSPLIT) == (16, 16, 64, 4)
    # the header compiles as C, with the sizes and constants ctypes sees
    src = tmp_path / "dc.c"
    src.write_text('#include <stdio.h>\n#include "ssdk_dconv.h"\nint main(void) { printf("%zu %zu %d %d %d %d\\n", sizeof(ssdk_conv_desc), '
                   'sizeof(ssdk_op), SSDK_CONV_DILATION_SHIFT, SSDK_CONV_DILATION_MASK, SSDK_DCONV_TILE_PIXELS, SSDK_DCONV_TILE_COUT); '
                   'int (*f)(const ssdk_conv_desc*, void*) = ssdk_dconv3x3; (void)f; '
                   'return ssdk_dconv3x3_supported(16, 24, 5, 4, 3, SSDK_BF16) == 1 && !ssdk_dconv3x3_supported(16, 24, 5, 4, 9, SSDK_BF16) '
                   '? 0 : 1; }\n')
    exe = tmp_path / "dc"
    lib = os.path.dirname(N.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-L", lib,
                    "-lssdk", "-Wl,-rpath," + lib], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert [int(v) for v in out] == [ctypes.sizeof(N.ConvDesc), ctypes.sizeof(N.Op), 8, 0xF00, 16, 64]


def test_predicate_is_the_rule_of_the_header():
    from ssds import _native as N

    f = N.lib.ssdk_dconv3x3_supported
    lo, hi, cmax, smax = N.DCONV_MIN_DILATION, N.DCONV_MAX_DILATION, N.DCONV_MAX_CHANNELS, N.DCONV_MAX_SIDE
    assert lo <= 2 and hi >= 8 and cmax >= 1024  # at least what the plan's callers rely on
    for cin in (0, 4, 8, 12, 16, 40, 128, 1000, cmax, cmax + 8):
        for cout in (0, 8, 20, 24, 136, cmax, cmax + 8):
            for d in (0, 1, lo, 3, 5, hi, hi + 1, 16):
                for h, w in ((1, 1), (0, 3), (3, 0), (2, 5), (13, 13), (smax, 1), (smax + 1, 1), (1, smax + 1)):
                    for dt in (N.BF16, N.F16, N.F32):
                        want = (8 <= cin <= cmax and cin % 8 == 0 and 8 <= cout <= cmax and cout % 8 == 0 and lo <= d <= hi
                                and 1 <= h <= smax and 1 <= w <= smax and dt in (N.BF16, N.F16))
                        assert f(cin, cout, h, w, d, dt) == int(want), (cin, cout, h, w, d, dt)


def test_ssdk_conv_refuses_a_bad_dilated_descriptor_before_any_device_call():
    from ssds import _native as N

    F0 = 0x1000  # never dereferenced: every call below fails validation first

    def call(fn, **kw):
        d = N.ConvDesc()
        d.x, d.w, d.w_frag, d.scale, d.bias, d.y = F0, F0, F0, F0, F0, 0x100000
        d.N, d.Cin, d.H, d.W, d.Cout, d.k, d.stride, d.groups = 2, 16, 5, 4, 24, 3, 1, 1
        d.act, d.dtype, d.in_layout, d.out_layout = N.ACT["relu"], N.BF16, N.NHWC, N.NHWC
        d.res_mode = (3 - 1) << N.CONV_DILATION_SHIFT
        for k, v in kw.items():
            setattr(d, k, v)
        rc = fn(d)
        return rc, N.lib.ssdk_last_error().decode()

    via_conv = lambda d: N.lib.ssdk_conv(ctypes.byref(d), None, 0, None)
    direct = lambda d: N.lib.ssdk_dconv3x3(ctypes.byref(d), None)
    bits = lambda dil, low=0: ((dil - 1) << N.CONV_DILATION_SHIFT) | low
    bad = (dict(stride=2), dict(k=1), dict(out_layout=N.NCHW), dict(in_layout=N.NCHW), dict(residual=F0), dict(y2=F0), dict(groups=2),
           dict(groups=16), dict(w_frag=None), dict(res_mode=bits(9)), dict(res_mode=bits(16)), dict(res_mode=bits(3, 2)),
           dict(res_mode=bits(3, 1)), dict(Cin=12), dict(Cout=20), dict(dtype=N.F32), dict(H=0), dict(N=0), dict(act=N.ACT["sigmoid"]),
           dict(x=None), dict(y=None), dict(bias=None), dict(w=None), dict(x=F0 + 8), dict(scale=F0 + 4), dict(y=F0))
    for fn in (via_conv, direct):
        for kw in bad:
            rc, msg = call(fn, **kw)
            assert rc == -1 and msg.startswith("dconv3x3:") and len(msg) > 12, (kw, rc, msg)
    assert N.lib.ssdk_dconv3x3(None, None) == -1
    # without the bits the descriptor means what it always meant: ssdk_conv's own checks answer (stride 3 is no geometry of its)
    rc, msg = call(via_conv, res_mode=0, stride=3)
    assert rc == -1 and msg.startswith("conv:")


# ---- 4. the planner, recorded on the CPU device ---------------------------------------------------------------------------------------
def _record(blocks, shape, dtype=torch.bfloat16):
    from ssds.modeling.layers import fused_conv as FC
    from ssds.modeling.layers import planner

    plan = FC.ConvPlan(torch.device("cpu"), dtype, shape)
    val = plan.input_value()
    for j, blk in enumerate(blocks):
        val = planner.record_rfb(plan, val, blk, keep_input=(j == 0))
    return plan.finalize(), val


def test_record_rfb_records_ten_ops(monkeypatch):
    from ssds import _native as N
    from ssds.modeling.layers import fused_conv as FC

    monkeypatch.delenv("SSDK_DCONV", raising=False)
    blk, x, _ = make_block("b128_s2_scale01")  # scale 0.1, dilations 2 and 3
    plan, out = _record([blk], x.shape)
    assert out[1:] == (2, 256, 3, 2)
    kinds = [L.get("kind") for L in plan.layers]
    assert kinds == [None] * 7 + ["cat", None, None] and all(L.get("lane", 0) == 0 for L in plan.layers)
    assert all(op.lane == 0 for op in plan.ops)
    assert [op.kind for op in plan.ops] == [N.OP_CONV] * 7 + [N.OP_CAT] + [N.OP_CONV] * 2
    convs = [L for L in plan.layers if L.get("kind") is None]
    geo = [(L["pack"].cin, L["pack"].cout, L["pack"].k, L["pack"].stride, L["pack"].dilation, L["h"], L["w"]) for L in convs]
    assert geo == [(128, 16, 1, 1, 1, 5, 3), (16, 32, 3, 2, 1, 5, 3), (32, 32, 3, 1, 2, 3, 2),
                   (128, 16, 1, 1, 1, 5, 3), (16, 24, 3, 1, 1, 5, 3), (24, 32, 3, 2, 1, 5, 3), (32, 32, 3, 1, 3, 3, 2),
                   (128, 256, 1, 2, 1, 5, 3), (64, 256, 1, 1, 1, 3, 2)]
    assert [L["act"] for L in convs] == ["relu", "relu", "none", "relu", "relu", "relu", "none", "none", "relu"]
    dil = [((op.conv.res_mode & N.CONV_DILATION_MASK) >> N.CONV_DILATION_SHIFT) + 1 for op in plan.ops]
    assert dil == [1, 1, 2, 1, 1, 1, 3, 1, 1, 1]
    for op, L in zip(plan.ops, plan.layers):
        if L.get("kind") is None and L["pack"].kind == "dilated":
            assert op.conv.w_frag == L["pack"].dfrag().data_ptr() and op.conv.res_mode & 3 == 0 and not op.conv.residual
            assert (op.conv.k, op.conv.stride, op.conv.groups, op.conv.H, op.conv.W) == (3, 1, 1, 3, 2)
    # ConvLinear: the shortcut as its residual, the ReLU behind the add, the block's scale in its folded BatchNorm
    last, short = plan.layers[9], plan.layers[8]
    assert plan.ops[9].conv.res_mode == 2 and last["res_mode"] == 2 and last["res"] == short["y"] and plan.ops[9].conv.residual
    assert plan.ops[9].conv.act == N.ACT["relu"] and last["x"] == plan.layers[7]["y"]
    plain = FC.ConvPack(blk.ConvLinear.conv, blk.ConvLinear.bn, "none", torch.bfloat16)
    torch.testing.assert_close(last["pack"].scale, plain.scale * 0.1, rtol=1e-6, atol=0)
    torch.testing.assert_close(last["pack"].bias, plain.bias * 0.1, rtol=1e-6, atol=0)
    assert torch.equal(last["pack"].w, plain.w) and float(plain.bias.abs().max()) > 0
    torch.testing.assert_close(short["pack"].scale, FC.ConvPack(blk.shortcut.conv, blk.shortcut.bn, "none", torch.bfloat16).scale)
    # the cat reads both branch ends, in order
    cat = plan.layers[7]
    assert (cat["x"], cat["b"], cat["c1"], cat["c2"]) == (plan.layers[2]["y"], plan.layers[6]["y"], 32, 32)
    rows = plan.layer_table()
    assert [r["name"] for r in rows if " d" in r["name"]] == ["conv 32>32 k3 s1 d2 @3x2", "conv 32>32 k3 s1 d3 @3x2"]
    assert rows[0]["name"] == "conv 128>16 k1 s1 @5x3"  # an undilated row reads as before


def test_the_parsers_block_carries_dilations_3_and_5(monkeypatch):
    from ssds import _native as N
    from ssds.modeling.layers.layers_parser import parse_feature_layer

    monkeypatch.delenv("SSDK_DCONV", raising=False)
    blk = parse_feature_layer("RBF:S", 256, 128)[0].eval()
    plan, _ = _record([blk], (2, 256, 5, 3), torch.float16)
    with_bits = [op.conv.res_mode for op in plan.ops if op.conv.res_mode & N.CONV_DILATION_MASK]
    assert with_bits == [2 << N.CONV_DILATION_SHIFT, 4 << N.CONV_DILATION_SHIFT]  # exactly two descriptors: dilations 3 and 5
    assert plan.ops[9].conv.res_mode & 3 == 2


def test_intermediates_are_released(monkeypatch):
    from ssds.modeling.layers.layers_parser import parse_feature_layer

    monkeypatch.delenv("SSDK_DCONV", raising=False)
    blocks = [parse_feature_layer("RBF", 128, 128)[0].eval() for _ in range(4)]
    counts = [len(_record(blocks[:n], (2, 128, 7, 5))[0].arena.bufs) for n in (1, 2, 3, 4)]
    assert counts[1] == counts[2] == counts[3], counts  # a chain of blocks re-uses the buffers of the block before
    assert counts[0] <= 7, counts  # never more than: x's two branch values in flight, the cat, the shortcut, the output ...


def test_unusable_in_planes_is_named(monkeypatch):
    """320 -> 40 -> 60 -> 80: a width inside the block is no multiple of 8.  MobileNetV2's last map has 320 channels."""
    from ssds.modeling import nets, ssds
    from ssds.modeling.layers import planner
    from ssds.modeling.layers.rfb_layers import BasicRFB

    monkeypatch.delenv("SSDK_DCONV", raising=False)
    blk = BasicRFB(320, 128, stride=2, scale=1.0, visual=2).eval()
    assert [blk.branch1[j].conv.out_channels for j in range(3)] == [40, 60, 80]
    with pytest.raises(planner.PlanUnsupported, match="BasicRFB with in_planes = 320"):
        _record([blk], (2, 320, 5, 3))
    outs, extras, head = ssds.SSD.add_extras([[5, 7, "RBF:S"], [96, 320, 128]], [6] * 3, 4)
    torch.manual_seed(0)
    model = ssds.SSD(nets.MobileNetV2(outputs=outs), extras, head, 4).eval()
    x = torch.rand(1, 3, 64, 64)
    plan = model.to(torch.bfloat16)._plan(x.to(torch.bfloat16))
    assert isinstance(plan, str) and "BasicRFB" in plan and "320" in plan
    with torch.no_grad():
        loc, conf = model.float()(x)  # the module path
    assert len(loc) == 3 and loc[2].shape[-2:] == (1, 1) and all(torch.isfinite(t).all() for t in loc + conf)


def test_ssdk_dconv_switch_is_read_at_recording_time(monkeypatch):
    from ssds.modeling.layers import fused_conv as FC
    from ssds.modeling.layers import planner

    model, x, fx = build("ssd_rfb_r18", monkeypatch)
    wl, _ = nethelp.want(fx)
    half = model.to(torch.bfloat16)
    monkeypatch.setenv("SSDK_DCONV", "0")
    off = half._plan(x.to(torch.bfloat16))
    assert isinstance(off, str) and "SSDK_DCONV=0" in off and "RFB extras run on PyTorch-ROCm" in off
    monkeypatch.setenv("SSDK_DCONV", "1")
    half.invalidate_plans()
    on = half._plan(x.to(torch.bfloat16))
    assert isinstance(on, FC.ConvPlan)
    packs = [L["pack"] for L in on.layers if L.get("kind") is None]
    assert [p.dilation for p in packs if p.kind == "dilated"] == [3, 5, 3, 5]
    assert sum(L.get("kind") == "cat" for L in on.layers) == 2
    # the Shelf builder goes through the same helper
    smodel, sx, _ = build("shelf_rfb_stub", monkeypatch)
    smodel = smodel.to(torch.bfloat16)
    feats = [f.to(torch.bfloat16) for f in smodel.backbone(sx)]
    splan = planner.build_shelf_plan(smodel, feats)
    assert [L["pack"].dilation for L in splan.layers if L.get("kind") is None and L["pack"].kind == "dilated"] == [3, 5]
    monkeypatch.setenv("SSDK_DCONV", "0")
    with pytest.raises(planner.PlanUnsupported, match="SSDK_DCONV=0: the RFB extras run on PyTorch-ROCm"):
        planner.build_shelf_plan(smodel, feats)
    # the model's forward takes the module path and still equals the fixture (a fresh fp32 model: ``half`` is ``model``, rounded)
    model, x, _ = build("ssd_rfb_r18", monkeypatch)
    with torch.no_grad():
        loc, _ = model(x)
    torch.testing.assert_close(loc[3], wl[3], rtol=1e-3, atol=5e-4 * float(wl[3].abs().max()))


def test_the_ssd_extras_record_on_external_maps(monkeypatch):
    """build_ssd_plan(model, None, features=...): the stub case's extras and heads as a plan of their own (what the GPU test runs)."""
    from ssds.modeling.layers import planner

    monkeypatch.delenv("SSDK_DCONV", raising=False)
    model, x, _ = build("ssd_rfb_stub", monkeypatch)
    model = model.to(torch.bfloat16)
    feats = [f.to(torch.bfloat16) for f in model.backbone(x)]
    plan = planner.build_ssd_plan(model, None, features=feats)
    dil = [(L["pack"].dilation, L["h"], L["w"]) for L in plan.layers if L.get("kind") is None and L["pack"].kind == "dilated"]
    assert dil == [(3, 7, 5), (5, 7, 5), (3, 4, 3), (5, 4, 3), (3, 2, 2), (5, 2, 2)]
    assert len(plan.heads) == 5 and len(plan.inputs) == 1
