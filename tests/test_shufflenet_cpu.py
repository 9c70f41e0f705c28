"""The ShuffleNetV2 backbones without a GPU: ``ShuffleNetV2_x1`` / ``_x2`` (ssds/modeling/nets/shufflenet.py) against the outputs of the
REFERENCE's own classes on the same seeded weights (tests/golden/net_*sfv2*.npz, written by tests/golden/make_golden_shufflenet.py),
the two shipped configs, the C-ABI of include/ssdk_shuffle.h, the packs and the planner's walk.  The kernels and the plans are checked
on the GPU in tests/test_gpu_shuffle.py."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import cases_shufflenet
import nethelp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFGS = {"SSDFPN": os.path.join(ROOT, "experiments", "cfgs", "fpn_shufflenetv2_x1_512.yml"),
        "YOLOV3": os.path.join(ROOT, "experiments", "cfgs", "yolov3_shufflenetv2_x2_416.yml")}
LEVELS = {"fpn_sfv2x1": 5, "yolov3_sfv2x2": 3}
REPEATS = (4, 8, 4)
WIDTHS = {"ShuffleNetV2_x1": (24, 116, 232, 464), "ShuffleNetV2_x2": (24, 244, 488, 976)}


class Fixture(dict):
    """A fixture as nethelp reads one: ``bn_flat`` (make_golden_shufflenet.py stores the BatchNorm statistics as one vector) is split
    back into the ``bn/<key>`` entries of the other fixtures."""

    def __init__(self, name):
        npz = nethelp.load_fixture(name)
        super().__init__({k: npz[k] for k in npz.files})
        for k, v in cases_shufflenet.bn_state(self).items():
            self["bn/" + k] = v

    @property
    def files(self):
        return list(self)


def build(name, monkeypatch):
    """nethelp.build (schema, shapes and key order against the fixture, seeded weights, stored BatchNorm statistics)."""
    monkeypatch.setattr(nethelp, "cases", cases_shufflenet)
    return nethelp.build(name, fx=Fixture(name))


def build_bare(name="sfv2x1_bare"):
    """The bare backbone of ``BACKBONE_CASES`` with nethelp.build's checks: keys, shapes and ORDER of the state_dict equal the
    reference's (less its classifier tail, which the fixture's schema leaves out)."""
    from ssds.modeling import nets

    fx = Fixture(name)
    seed, net, outputs, _ = cases_shufflenet.BACKBONE_CASES[name]
    model = getattr(nets, net)(outputs=outputs)
    ref_spec = [(str(k), tuple(int(s) for s in str(sh).split(",")) if str(sh) else ()) for k, sh in zip(fx["keys"], fx["shapes"])]
    assert [(k, tuple(v.shape)) for k, v in model.state_dict().items()] == ref_spec
    state = cases_shufflenet.seeded_state(ref_spec, seed)
    for k in list(state):
        if "bn/" + k in fx:
            state[k] = fx["bn/" + k]
    model.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in state.items()})
    return model.eval(), torch.from_numpy(cases_shufflenet.net_image(name)), fx


# ---- 1. the module ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(WIDTHS))
def test_reachable_by_name(name):
    from ssds.modeling import nets
    from ssds.modeling.nets import shufflenet

    assert getattr(nets, name) is getattr(shufflenet, name)
    net = getattr(nets, name)(outputs=[2, 3, 4])
    assert isinstance(net, shufflenet.ShuffleNetV2) and net.outputs == [2, 3, 4] and net.initialize() is None
    assert [n for n, _ in net.named_children()] == ["conv1", "maxpool", "stage2", "stage3", "stage4"]
    assert not hasattr(net, "conv5") and not hasattr(net, "fc")
    w = WIDTHS[name]
    assert [len(getattr(net, "stage%d" % s)) for s in (2, 3, 4)] == list(REPEATS)
    for si, s in enumerate((2, 3, 4)):
        stage = getattr(net, "stage%d" % s)
        assert [u.stride for u in stage] == [2] + [1] * (REPEATS[si] - 1)
        assert len(stage[0].branch1) == 5 and len(stage[0].branch2) == 8 and len(stage[1].branch1) == 0 and len(stage[1].branch2) == 8
        assert stage[0].branch2[0].in_channels == w[si] and stage[0].branch2[5].out_channels == w[si + 1] // 2
        assert stage[1].branch2[0].in_channels == w[si + 1] // 2
    assert all(m.bias is None for m in net.modules() if isinstance(m, torch.nn.Conv2d))
    with torch.no_grad():
        maps = net.eval()(torch.zeros(1, 3, 64, 32))
    assert [tuple(m.shape) for m in maps] == [(1, w[1], 8, 4), (1, w[2], 4, 2), (1, w[3], 2, 1)]
    with torch.no_grad():  # the forward stops at max(outputs)
        maps = getattr(nets, name)(outputs=[2]).eval()(torch.zeros(1, 3, 64, 32))
    assert [tuple(m.shape) for m in maps] == [(1, w[1], 8, 4)]


def test_channel_shuffle_interleaves_the_halves():
    from ssds.modeling.nets.shufflenet import InvertedResidual, channel_shuffle

    x = torch.arange(2 * 10 * 3 * 2, dtype=torch.float32).view(2, 10, 3, 2)
    y = channel_shuffle(x, 2)
    assert torch.equal(y[:, 0::2], x[:, :5]) and torch.equal(y[:, 1::2], x[:, 5:])
    unit = InvertedResidual(16, 16, 1).eval()
    with torch.no_grad():
        out = unit(x[:, :, :, :].repeat(1, 2, 1, 1)[:, :16])
        src = x.repeat(1, 2, 1, 1)[:, :16]
        assert torch.equal(out[:, 0::2], src[:, :8]) and torch.equal(out[:, 1::2], unit.branch2(src[:, 8:]))
    down = InvertedResidual(16, 24, 2).eval()
    with torch.no_grad():
        out = down(src)
        assert torch.equal(out[:, 0::2], down.branch1(src)) and torch.equal(out[:, 1::2], down.branch2(src))


@pytest.fixture(scope="module", params=["SSDFPN", "YOLOV3"])
def shipped(request):
    from ssds.core import config
    from ssds.modeling import model_builder

    cfg = config.cfg_from_file(CFGS[request.param])
    torch.manual_seed(0)
    return request.param, cfg, model_builder.create_model(cfg.MODEL)


def test_shipped_configs_build(shipped):
    from ssds.modeling import model_builder, ssds
    from ssds.modeling.nets.shufflenet import ShuffleNetV2

    head, cfg, model = shipped
    assert isinstance(model, getattr(ssds, head)) and cfg.MODEL.SSDS == head
    assert isinstance(model.backbone, ShuffleNetV2) and model.backbone.outputs == [2, 3, 4]
    assert cfg.MODEL.NUM_CLASSES == 80 and cfg.TRAIN.BATCH_SIZE == cfg.TEST.BATCH_SIZE == 32
    anchors = model_builder.create_anchors(cfg.MODEL, model, cfg.MODEL.IMAGE_SIZE)
    if head == "YOLOV3":
        assert cfg.MODEL.NETS == "ShuffleNetV2_x2" and list(cfg.MODEL.IMAGE_SIZE) == [416, 416] and list(anchors) == [8, 16, 32]
        assert [list(f) for f in cfg.MODEL.FEATURE_LAYER] == [[2, 3, 4], [244, 488, 976]]
    else:
        assert cfg.MODEL.NETS == "ShuffleNetV2_x1" and list(cfg.MODEL.IMAGE_SIZE) == [512, 512] and list(anchors) == [8, 16, 32, 64, 128]
        assert [list(f) for f in cfg.MODEL.FEATURE_LAYER] == [[2, 3, 4, "Conv:S", "Conv:S"], [116, 232, 464, 464, 256]]


def test_state_dict_schema_is_the_reference_s():
    model, _, fx = build_bare()  # (asserts keys, shapes and order)
    keys = [str(k) for k in fx["keys"]]
    assert keys[:6] == ["conv1.0.weight", "conv1.1.weight", "conv1.1.bias", "conv1.1.running_mean", "conv1.1.running_var",
                        "conv1.1.num_batches_tracked"]
    assert keys[6] == "stage2.0.branch1.0.weight" and keys[-1] == "stage4.3.branch2.6.num_batches_tracked"
    assert "stage3.7.branch2.5.weight" in keys and not [k for k in keys if k.startswith("conv5.") or k.startswith("fc.")]
    for name in cases_shufflenet.NET_CASES:
        keys = [str(k) for k in Fixture(name)["keys"]]
        assert "backbone.stage4.3.branch2.5.weight" in keys and not [k for k in keys if "conv5." in k or ".fc." in k]


def test_bare_backbone_matches_reference_fp32():
    model, x, fx = build_bare()
    with torch.no_grad():
        maps = model(x)
    assert len(maps) == 2
    for i, m in enumerate(maps):
        want = torch.from_numpy(fx["out%d" % i])
        assert m.shape == want.shape and float(want.std()) > 0.1
        torch.testing.assert_close(m, want, rtol=1e-3, atol=5e-4 * float(want.abs().max()))  # (tolerances of test_densenet_cpu.py)


@pytest.mark.parametrize("name", list(cases_shufflenet.NET_CASES))
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
        torch.testing.assert_close(l, a, rtol=1e-3, atol=5e-4 * float(a.abs().max()))  # (tolerances of test_densenet_cpu.py)
        torch.testing.assert_close(c, b, rtol=1e-3, atol=2e-4)


def test_fixtures_are_no_larger_than_the_largest_committed_before():
    golden = os.path.join(ROOT, "tests", "golden")
    ours = ["net_%s.npz" % n for n in list(cases_shufflenet.NET_CASES) + list(cases_shufflenet.BACKBONE_CASES)]
    others = [f for f in os.listdir(golden) if f.endswith(".npz") and f not in ours]
    assert max(os.path.getsize(os.path.join(golden, f)) for f in ours) <= max(os.path.getsize(os.path.join(golden, f)) for f in others)


def test_a_reference_checkpoint_with_the_classifier_tail_resumes(tmp_path):
    """A checkpoint written from the reference's model carries ``conv5.*`` / ``fc.*`` (torchvision's classifier tail) and, out of
    DataParallel, a ``module.`` prefix: every key of this module is loaded, the tail is skipped."""
    from ssds.core import checkpoint
    from ssds.modeling import nets

    src, _, _ = build_bare()
    state = {"module." + k: v.clone() for k, v in src.state_dict().items()}
    state["module.conv5.0.weight"] = torch.randn(1024, 464, 1, 1)
    state["module.conv5.1.weight"] = torch.ones(1024)
    state["module.fc.weight"], state["module.fc.bias"] = torch.randn(1000, 1024), torch.zeros(1000)
    path = str(tmp_path / "ref.pth")
    torch.save({"state_dict": state}, path)
    dst = nets.ShuffleNetV2_x1(outputs=[3, 4])
    assert checkpoint.resume_checkpoint(dst, path, "") is dst
    for (k, a), (_, b) in zip(src.state_dict().items(), dst.state_dict().items()):
        assert torch.equal(a, b), k


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
    """The unit has a header of its own (include/ssdk_shuffle.h): the entry points of ssdk.h and the layout of ssdk_op stay the closed
    list of ABI 245; executor ops 14 and 15 are described by existing members of ssdk_op."""
    from ssds import _native as N

    assert N.lib.ssdk_version() == 245 and N.ABI_VERSION == 245 and len(N.EXPORTS) == 127
    header = open(os.path.join(ROOT, "include", "ssdk_shuffle.h")).read()
    main = open(os.path.join(ROOT, "include", "ssdk.h")).read()
    assert N.SHUFFLE_EXPORTS == ("ssdk_shuffle_unit", "ssdk_shuffle_unit_desc_bytes", "ssdk_shuffle_unit_supported", "ssdk_shuffle_down",
                                 "ssdk_shuffle_down_desc_bytes", "ssdk_shuffle_down_supported")
    for name in N.SHUFFLE_EXPORTS:
        assert (name + "(") in header and hasattr(N.lib, name) and getattr(N.lib, name).argtypes is not None, name
        assert name not in N.EXPORTS and (name + "(") not in main
    assert N.lib.ssdk_shuffle_unit.argtypes == [ctypes.POINTER(N.ShuffleUnitDesc), ctypes.c_void_p]
    assert N.lib.ssdk_shuffle_down.argtypes == [ctypes.POINTER(N.ShuffleDownDesc), ctypes.c_void_p]
    assert N.lib.ssdk_shuffle_unit_supported.argtypes == [ctypes.c_int] * 4
    assert N.lib.ssdk_shuffle_down_supported.argtypes == [ctypes.c_int] * 5
    for desc, fn in ((N.ShuffleUnitDesc, N.lib.ssdk_shuffle_unit_desc_bytes), (N.ShuffleDownDesc, N.lib.ssdk_shuffle_down_desc_bytes)):
        assert fn.argtypes == [] and ctypes.sizeof(desc) == fn()
    assert [f[0] for f in N.ShuffleUnitDesc._fields_] == ["x", "y", "w1", "scale1", "bias1", "wd", "scale2", "bias2", "w3", "scale3",
                                                          "bias3", "N", "H", "W", "Cb", "dtype"]
    assert [f[0] for f in N.ShuffleDownDesc._fields_] == ["x", "y", "b1_wd", "b1_scale1", "b1_bias1", "b1_w2", "b1_scale2", "b1_bias2",
                                                          "w1", "scale1", "bias1", "wd", "scale2", "bias2", "w3", "scale3", "bias3",
                                                          "N", "H", "W", "Cin", "ld_in", "Cb", "dtype"]
    assert (N.OP_SHUFFLE, N.OP_SHUFFLEDOWN) == (14, 15) and N.OP_DENSEPLACE == 13
    assert "SSDK_OP_SHUFFLE = 14, SSDK_OP_SHUFFLEDOWN = 15" in main
    assert [f[0] for f in N.Op._fields_] == ["kind", "lane", "conv", "mb", "fuse", "stem", "pool", "xpair", "mbse"]
    assert N.lib.ssdk_struct_size(7) == ctypes.sizeof(N.Op) and N.lib.ssdk_struct_size(8) == 0
    assert N.lib.ssdk_abi_check(N.ABI_VERSION, ctypes.sizeof(N.Op)) == 0
    assert (N.SHUFFLE_TILE_H, N.SHUFFLE_TILE_W, N.SHUFFLE_CHUNK) == (4, 16, 64)
    # the sizes as a C compiler sees the headers
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include "ssdk_shuffle.h"\nint main(void) { printf("%zu %zu %zu %d %d %d %d %d\\n", '
                   'sizeof(ssdk_shuffle_unit_desc), sizeof(ssdk_shuffle_down_desc), sizeof(ssdk_op), (int)SSDK_OP_SHUFFLE, '
                   '(int)SSDK_OP_SHUFFLEDOWN, SSDK_SHUFFLE_TILE_H, SSDK_SHUFFLE_TILE_W, SSDK_SHUFFLE_CHUNK); return 0; }\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert [int(v) for v in out] == [ctypes.sizeof(N.ShuffleUnitDesc), ctypes.sizeof(N.ShuffleDownDesc), ctypes.sizeof(N.Op), 14, 15,
                                     N.SHUFFLE_TILE_H, N.SHUFFLE_TILE_W, N.SHUFFLE_CHUNK]


def test_the_main_header_is_the_parent_s_but_for_the_two_op_kinds():
    """ssdk.h's entry-point list, sizeof(ssdk_op) and the version are what they were: the only code change is two enumerators."""
    from ssds import _native as N

    assert ctypes.sizeof(N.Op) == N.lib.ssdk_struct_size(7) and N.ABI_VERSION == 245
    assert not [n for n in N.EXPORTS if "shuffle" in n]
    main = open(os.path.join(ROOT, "include", "ssdk.h")).read()
    assert main.count("SSDK_OP_SHUFFLE = 14") == 1 and main.count("SSDK_OP_SHUFFLEDOWN = 15") == 1


F0 = 0x100000  # never dereferenced: every call below fails validation first


def _unit_call(**kw):
    from ssds import _native as N

    d = N.ShuffleUnitDesc()
    d.N, d.H, d.W, d.Cb, d.dtype = 2, 13, 9, 58, N.BF16
    d.x, d.y = F0, F0 + 0x1000000
    for i, name in enumerate(("w1", "scale1", "bias1", "wd", "scale2", "bias2", "w3", "scale3", "bias3")):
        setattr(d, name, F0 + 0x2000000 + 0x100000 * i)
    for k, v in kw.items():
        setattr(d, k, v)
    rc = N.lib.ssdk_shuffle_unit(ctypes.byref(d), None)
    return rc, N.lib.ssdk_last_error().decode()


def _down_call(**kw):
    from ssds import _native as N

    d = N.ShuffleDownDesc()
    d.N, d.H, d.W, d.Cin, d.Cb, d.dtype = 2, 13, 9, 24, 58, N.BF16
    d.x, d.y = F0, F0 + 0x1000000
    for i, name in enumerate(("b1_wd", "b1_scale1", "b1_bias1", "b1_w2", "b1_scale2", "b1_bias2", "w1", "scale1", "bias1", "wd", "scale2",
                              "bias2", "w3", "scale3", "bias3")):
        setattr(d, name, F0 + 0x2000000 + 0x100000 * i)
    for k, v in kw.items():
        setattr(d, k, v)
    rc = N.lib.ssdk_shuffle_down(ctypes.byref(d), None)
    return rc, N.lib.ssdk_last_error().decode()


def test_bad_arguments_are_refused_before_any_launch():
    """No device is needed: each call is refused by the argument checks, with a message that names the entry point."""
    from ssds import _native as N

    for kw in (dict(Cb=0), dict(Cb=6), dict(Cb=57), dict(Cb=514), dict(Cb=-58), dict(dtype=N.F32), dict(dtype=9), dict(H=0), dict(W=0),
               dict(H=-3), dict(W=32769), dict(N=0), dict(x=None), dict(y=None), dict(w1=None), dict(wd=None), dict(w3=None),
               dict(scale1=None), dict(bias2=None), dict(scale3=None), dict(x=F0 + 8), dict(y=F0 + 0x1000000 + 2),
               dict(w3=F0 + 0x2600000 + 4), dict(y=F0), dict(y=F0 + 64), dict(N=1 << 20, H=1 << 15, W=1 << 15)):
        rc, msg = _unit_call(**kw)
        assert rc == -1 and msg.startswith("shuffle_unit:"), (kw, rc, msg)
    assert "overlaps" in _unit_call(y=F0 + 64)[1] and "unsupported" in _unit_call(Cb=57)[1]
    assert N.lib.ssdk_shuffle_unit(None, None) == -1
    for kw in (dict(Cin=0), dict(Cin=6), dict(Cin=25), dict(Cin=1026), dict(Cb=57), dict(Cb=514), dict(dtype=N.F32), dict(H=0), dict(W=0),
               dict(W=32769), dict(N=0), dict(ld_in=16), dict(ld_in=28), dict(x=None), dict(y=None), dict(b1_wd=None), dict(b1_w2=None),
               dict(w1=None), dict(bias3=None), dict(x=F0 + 8), dict(b1_scale1=F0 + 0x2100000 + 4), dict(y=F0), dict(y=F0 + 64),
               dict(N=1 << 20, H=1 << 15, W=1 << 15)):
        rc, msg = _down_call(**kw)
        assert rc == -1 and msg.startswith("shuffle_down:"), (kw, rc, msg)
    assert "ld_in" in _down_call(ld_in=28)[1] and "overlaps" in _down_call(y=F0 + 64)[1]
    assert N.lib.ssdk_shuffle_down(None, None) == -1


def test_the_predicates_take_every_unit_of_both_networks_and_refuse_the_rest():
    from ssds import _native as N

    unit, down = N.lib.ssdk_shuffle_unit_supported, N.lib.ssdk_shuffle_down_supported
    for name, w in WIDTHS.items():
        for size in (320, 416, 512):
            for si in range(3):
                m_in, m_out = size // (4 << si), size // (8 << si)  # the stage's input and output maps
                for dt in (N.BF16, N.F16):
                    assert down(w[si], w[si + 1] // 2, m_in, m_in, dt) == 1, (name, size, si)
                    assert unit(w[si + 1] // 2, m_out, m_out, dt) == 1, (name, size, si)
    for cb in range(0, 520):
        ok = cb % 2 == 0 and 8 <= cb <= 512
        assert bool(unit(cb, 13, 9, N.BF16)) == ok and bool(down(24, cb, 13, 9, N.F16)) == ok, cb
        if not ok:
            assert "unsupported" in _unit_call(Cb=cb)[1] and "unsupported" in _down_call(Cb=cb)[1]
    for cin in range(0, 1030):
        ok = cin % 2 == 0 and 8 <= cin <= 1024
        assert bool(down(cin, 58, 13, 9, N.BF16)) == ok, cin
    for h, w, dt in ((0, 4, N.BF16), (4, 0, N.BF16), (-1, 4, N.F16), (4, 32769, N.F16), (4, 4, N.F32), (4, 4, 7)):
        assert unit(58, h, w, dt) == 0 and down(24, 58, h, w, dt) == 0
    assert unit(58, 1, 1, N.F16) == 1 and unit(512, 32768, 32768, N.BF16) == 1 and down(1024, 512, 1, 1, N.BF16) == 1
    assert unit(57, 4, 4, N.BF16) == 0 and unit(514, 4, 4, N.BF16) == 0


# ---- 3. the packs ----------------------------------------------------------------------------------------------------------------
def _unfrag(img):
    """The inverse of fused_conv._frag_image: [rows / 16][K / 32][4][16][8] -> [rows][K]."""
    g, ks = img.shape[0], img.shape[1]
    return img.permute(0, 3, 1, 2, 4).reshape(g * 16, ks * 32)


def _seeded_unit(inp, oup, stride, seed):
    from ssds.modeling.nets.shufflenet import InvertedResidual

    torch.manual_seed(seed)
    unit = InvertedResidual(inp, oup, stride).eval()
    with torch.no_grad():
        for m in unit.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.weight.uniform_(-1.5, 1.5)
                m.bias.normal_(0, 0.1)
                m.running_mean.normal_(0, 0.1)
                m.running_var.uniform_(0.5, 1.0)
    return unit


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("cb", (58, 122, 232, 488))
def test_unit_pack_images_are_the_folded_weights_zero_padded(cb, dtype):
    from ssds.modeling.layers import fused_conv as FC

    unit = _seeded_unit(2 * cb, 2 * cb, 1, cb)
    pk = FC.ShuffleUnitPack(unit, dtype)
    p = pk.p
    assert p == (cb + 63) // 64 * 64 and pk.cb == cb and pk.stride == 1
    b2 = unit.branch2
    for img, mat, conv in ((pk.w1_img, pk.w1, b2[0]), (pk.w3_img, pk.w3, b2[5])):
        back = _unfrag(img)
        assert back.shape == (p, p) and img.dtype == dtype and torch.equal(back, mat)
        assert torch.equal(back[:cb, :cb], conv.weight.detach().view(cb, cb).to(dtype))
        assert not bool(back[cb:].any()) and not bool(back[:, cb:].any())
    assert pk.wd.shape == (9, p) and not bool(pk.wd[:, cb:].any())
    assert torch.equal(pk.wd[:, :cb], b2[3].weight.detach().view(cb, 9).t().to(dtype))  # tap = 3 ky + kx
    for (s, b), bn in (((pk.scale1, pk.bias1), b2[1]), ((pk.scale2, pk.bias2), b2[4]), ((pk.scale3, pk.bias3), b2[6])):
        a, c = FC.fold_norm(bn)
        assert s.dtype == torch.float32 and s.shape == (p,) and torch.equal(s[:cb], a) and torch.equal(b[:cb], c)
        assert not bool(s[cb:].any()) and not bool(b[cb:].any())
    assert pk.scale2.data_ptr() == pk.affine2.data_ptr() and pk.bias2.data_ptr() == pk.affine2.data_ptr() + 4 * p
    assert bool((pk.scale1[:cb] < 0).any())  # (BatchNorm weights of mixed sign survive the folding)


@pytest.mark.parametrize("chans", ((24, 58), (116, 116), (244, 244), (488, 488), (976, 488)))
def test_down_pack_images_are_the_folded_weights_zero_padded(chans):
    from ssds.modeling.layers import fused_conv as FC

    cin, cb = chans
    dtype = torch.bfloat16
    unit = _seeded_unit(cin, 2 * cb, 2, cin + cb)
    pk = FC.ShuffleDownPack(unit, dtype)
    p, kp = pk.p, pk.kp
    assert kp == (cin + 31) // 32 * 32 and (pk.cin, pk.cb, pk.stride) == (cin, cb, 2)
    b1, b2 = unit.branch1, unit.branch2
    for img, mat, conv, k, kpad in ((pk.w1_img, pk.w1, b2[0], cin, kp), (pk.w3_img, pk.w3, b2[5], cb, p), (pk.b1_w2_img, pk.b1_w2, b1[2], cin, kp)):
        back = _unfrag(img)
        assert back.shape == (p, kpad) and torch.equal(back, mat)
        assert torch.equal(back[:cb, :k], conv.weight.detach().view(cb, k).to(dtype))
        assert not bool(back[cb:].any()) and not bool(back[:, k:].any())
    assert pk.b1_wd.shape == (9, kp) and not bool(pk.b1_wd[:, cin:].any())
    assert torch.equal(pk.b1_wd[:, :cin], b1[0].weight.detach().view(cin, 9).t().to(dtype))
    a, c = FC.fold_norm(b1[1])
    assert torch.equal(pk.b1_scale1[:cin], a) and torch.equal(pk.b1_bias1[:cin], c) and not bool(pk.b1_scale1[cin:].any())
    a, c = FC.fold_norm(b1[3])
    assert torch.equal(pk.b1_scale2[:cb], a) and torch.equal(pk.b1_bias2[:cb], c) and not bool(pk.b1_bias2[cb:].any())


def test_the_packs_say_why_a_unit_is_not_theirs():
    from ssds.modeling.layers import fused_conv as FC
    from ssds import _native as N

    unit, down = _seeded_unit(116, 116, 1, 1), _seeded_unit(24, 116, 2, 2)
    assert FC.ShuffleUnitPack.unsupported(unit) is None and FC.ShuffleDownPack.unsupported(down) is None
    assert "stride-1" in FC.ShuffleUnitPack.unsupported(down) and "stride-2" in FC.ShuffleDownPack.unsupported(unit)
    unit.branch2[2] = torch.nn.ReLU6()
    assert "ReLU6" in FC.ShuffleUnitPack.unsupported(unit)
    with pytest.raises(N.SsdkError, match="ReLU6"):
        FC.ShuffleUnitPack(unit, torch.bfloat16)
    down.branch1[0] = torch.nn.Conv2d(24, 24, 3, 2, 1, groups=24, bias=True)
    assert "branch1.0" in FC.ShuffleDownPack.unsupported(down)
    assert "Identity" in FC.ShuffleUnitPack.unsupported(torch.nn.Identity())
    wide = _seeded_unit(1028, 1028, 1, 3)
    assert "ssdk_shuffle_unit_supported" in FC.ShuffleUnitPack.unsupported(wide)


# ---- 4. the planner --------------------------------------------------------------------------------------------------------------
def _record(net, shape=(2, 3, 96, 64), dtype=torch.bfloat16):
    from ssds.modeling.layers import fused_conv as FC
    from ssds.modeling.layers import planner

    net = net.eval().to(dtype)
    plan = FC.ConvPlan(torch.device("cpu"), dtype, shape)
    outs = planner.record_backbone(plan, plan.input_value(), net)
    return plan.finalize(), outs


@pytest.mark.parametrize("name", sorted(WIDTHS))
def test_planner_records_one_op_per_unit_and_no_concatenation(name, monkeypatch):
    from ssds import _native as N
    from ssds.modeling import nets
    from ssds.modeling.layers import fused_conv as FC

    monkeypatch.setenv("SSDK_SHUFFLEUNIT", "1")
    w = WIDTHS[name]
    plan, outs = _record(getattr(nets, name)(outputs=[2, 3, 4]))
    kinds = [L.get("kind") for L in plan.layers]
    assert kinds.count("shuffle") == 13 and kinds.count("shuffledown") == 3 and "cat" not in kinds
    assert kinds == [None, "pool"] + sum((["shuffledown"] + ["shuffle"] * (r - 1) for r in REPEATS), [])
    pad8 = lambda c: (c + 7) // 8 * 8
    assert [tuple(o[1:]) for o in outs] == [(2, pad8(w[1]), 12, 8), (2, pad8(w[2]), 6, 4), (2, pad8(w[3]), 3, 2)]
    assert [FC.value_segs(o) for o in outs] == [((w[i], pad8(w[i])),) for i in (1, 2, 3)]
    assert isinstance(outs[0], FC.PaddedValue) and outs[0].real_channels == w[1] and not isinstance(outs[1], FC.PaddedValue)
    # conv1: 24 channels as 32 per pixel, zero rows and biases in the padding; the pool keeps them
    stem = plan.layers[0]["pack"]
    assert (stem.kind, stem.cout, stem.cout_real) == ("stem", 32, 24) and not bool(stem.w[24:].any()) and not bool(stem.bias[24:].any())
    assert plan.layers[1]["ch"] == 32
    # the ops: branch2 in `mb`, branch1 in `xpair`, ld_in in xpair.pad
    at, hw = 2, [(24, 16), (12, 8), (6, 4), (3, 2)]
    for si, reps in enumerate(REPEATS):
        cb = w[si + 1] // 2
        for j in range(reps):
            L, op = plan.layers[at], plan.ops[at]
            pk, m = L["pack"], op.mb
            h, wd = hw[si] if j == 0 else hw[si + 1]
            assert (L["h"], L["w"], pk.cb) == (h, wd, cb) and op.lane == 0 and L["x"] != L["y"]
            assert op.kind == (N.OP_SHUFFLEDOWN if j == 0 else N.OP_SHUFFLE)
            assert (m.N, m.H, m.W, m.Chid, m.Cout, m.stride, m.dtype) == (2, h, wd, cb, 2 * cb, 2 if j == 0 else 1, N.BF16)
            assert m.Cin == (w[si] if j == 0 else 2 * cb) and not m.residual and not m.stem and not m.w_image
            assert m.x == plan.arena.ptr(L["x"]) and m.y == plan.arena.ptr(L["y"])
            assert m.w_expand == pk.w1_img.data_ptr() and m.w_dw == pk.wd.data_ptr() and m.bias_dw == pk.affine2.data_ptr()
            assert m.w_project == pk.w3_img.data_ptr() and m.scale_project == pk.scale3.data_ptr()
            if j == 0:
                b = op.xpair
                assert (b.Cin, b.Cmid, b.Cout, b.pad) == (w[si], w[si], cb, 32 if si == 0 else pad8(w[si]))
                assert b.w1 == pk.b1_wd.data_ptr() and b.w2_frag == pk.b1_w2_img.data_ptr() and not b.w2
                assert b.act1 == N.ACT["none"] and b.act2 == N.ACT["relu"]
            at += 1
    assert at == len(plan.layers)
    table = plan.layer_table()
    assert len(table) == len(plan.layers) and table[2]["name"] == "shuffledown 24>%d k1,dw3s2,k1 @24x16" % w[1]
    assert table[3]["name"] == "shuffle %d k1,dw3,k1 @12x8" % w[1]
    assert table[3]["flops"] == 2.0 * 2 * 12 * 8 * (2 * (w[1] // 2) ** 2 + 9 * (w[1] // 2))


def test_no_buffer_is_released_before_its_last_reader():
    """Replaying the recording in order: whatever an op reads was last written by its producer, and the output maps are never written
    again."""
    from ssds.modeling import nets

    plan, outs = _record(nets.ShuffleNetV2_x1(outputs=[2, 3, 4]))
    holds = {}
    for i, L in enumerate(plan.layers):
        if isinstance(L["x"], int):
            assert holds[L["x"]] == i - 1 and L["y"] != L["x"], (i, holds.get(L["x"]))
        holds[L["y"]] = i
    last = {2: 5, 3: 13, 4: 17}
    assert [holds[o[0]] for o in outs] == [last[s] for s in (2, 3, 4)]


def test_the_switch_sends_the_backbone_to_torch(monkeypatch):
    from ssds.modeling import nets
    from ssds.modeling.layers import fused_conv as FC
    from ssds.modeling.layers import planner

    monkeypatch.setenv("SSDK_SHUFFLEUNIT", "0")
    assert not FC.shuffleunit_enabled()
    with pytest.raises(planner.PlanUnsupported, match="SSDK_SHUFFLEUNIT=0"):
        _record(nets.ShuffleNetV2_x1(outputs=[2, 3, 4]))
    monkeypatch.setenv("SSDK_SHUFFLEUNIT", "1")
    plan, _ = _record(nets.ShuffleNetV2_x1(outputs=[2, 3, 4]))
    assert [L.get("kind") for L in plan.layers].count("shuffle") == 13
    monkeypatch.delenv("SSDK_SHUFFLEUNIT")
    assert FC.shuffleunit_enabled() == (FC.SHUFFLEUNIT_DEFAULT != "0")
    row = [l for l in open(os.path.join(ROOT, "docs", "SWITCHES.md")) if l.startswith("| `SSDK_SHUFFLEUNIT`")]
    assert len(row) == 1 and row[0].split("|")[2].strip() == FC.SHUFFLEUNIT_DEFAULT and "tests/test_gpu_shuffle.py::" in row[0]


def test_planner_refuses_what_the_kernels_do_not_cover():
    from ssds.modeling import nets
    from ssds.modeling.layers import fused_conv as FC
    from ssds.modeling.layers import planner

    net = nets.ShuffleNetV2_x1(outputs=[2, 3])
    assert len(_record(net)[1]) == 2
    net.stage3[2] = torch.nn.Identity()
    with pytest.raises(planner.PlanUnsupported, match=r"stage3\.2: block Identity has no planner"):
        _record(net)
    net = nets.ShuffleNetV2_x1(outputs=[2])
    net.stage2[1].branch2[2] = torch.nn.ReLU6()
    with pytest.raises(planner.PlanUnsupported, match=r"stage2\.1: branch2.*ReLU6"):
        _record(net)
    net = nets.ShuffleNetV2_x1(outputs=[2])
    net.stage2[0].branch1[4] = torch.nn.SiLU()
    with pytest.raises(planner.PlanUnsupported, match=r"stage2\.0: branch1.*SiLU"):
        _record(net)
    net = nets.ShuffleNetV2_x1(outputs=[2])
    net.maxpool = torch.nn.MaxPool2d(2, 2)
    with pytest.raises(planner.PlanUnsupported, match="maxpool"):
        _record(net)
    net = nets.ShuffleNetV2_x1(outputs=[2])
    net.conv1[0] = torch.nn.Conv2d(3, 24, 5, 2, 2, bias=False)
    with pytest.raises(planner.PlanUnsupported, match="conv1"):
        _record(net)
    net = nets.ShuffleNetV2_x1(outputs=[2])
    net.stage2 = torch.nn.Identity()
    with pytest.raises(planner.PlanUnsupported, match="stage2: a Sequential of units expected, got Identity"):
        _record(net)
    # nothing leaks out of a recording: outside one a 116-channel convolution is 'not covered', as it was
    assert FC.conv_kind(torch.nn.Conv2d(116, 256, 1)) is None and FC.conv_kind(torch.nn.Conv2d(3, 24, 3, 2, 1)) is None
    with pytest.raises(FC.N.SsdkError, match="outside"):
        FC.allow_padded_maps()


def test_a_consumer_of_the_116_channel_map_pads_its_input_columns(monkeypatch):
    """FPN on ShuffleNetV2 x1: the lateral 1x1 of level 2 reads the 120-channel value with 120 weight columns, the last four zero;
    YOLOv3 on x2: the convolution behind the concatenation of two 244-in-248 maps has its zero columns where the padding is."""
    from ssds.modeling.layers import fused_conv as FC

    monkeypatch.setenv("SSDK_SHUFFLEUNIT", "1")
    model, x, _ = build("fpn_sfv2x1", monkeypatch)
    model = model.to(torch.bfloat16)
    plan = model._build_neck_plan(None, image=x.to(torch.bfloat16))
    kinds = [L.get("kind") for L in plan.layers]
    assert kinds.count("shuffle") == 13 and kinds.count("shuffledown") == 3 and "cat" not in kinds
    lateral = [L["pack"] for L in plan.layers if L.get("kind") is None and L["pack"].k == 1 and L["pack"].cin == 120]
    assert len(lateral) == 1
    pk = lateral[0]
    conv = model.transforms[0]
    assert pk.in_segs == ((116, 120),) and pk.w.shape == (256, 1, 1, 120) and not bool(pk.w[..., 116:].any())
    assert torch.equal(pk.w[:, 0, 0, :116], conv.weight.detach()[:, :, 0, 0].to(torch.bfloat16))
    assert FC.conv_kind(conv) is None  # (outside the recording nothing changed)
    model, x, _ = build("yolov3_sfv2x2", monkeypatch)
    model = model.to(torch.bfloat16)
    plan = model._build_neck_plan(None, image=x.to(torch.bfloat16))
    cats = [i for i, L in enumerate(plan.layers) if L.get("kind") == "cat"]
    assert len(cats) == 2
    behind = plan.layers[cats[1] + 1]["pack"]  # level 2: 244 (in 248) backbone channels || the upsampled branch
    assert behind.in_segs[0] == (244, 248) and behind.cin == sum(q for _, q in behind.in_segs)
    assert not bool(behind.w[..., 244:248].any()) and bool(behind.w[..., :244].any()) and bool(behind.w[..., 248:].any())


@pytest.mark.parametrize("head", ["SSD", "SSDFPN", "SSDBiFPN", "SSDShelf", "YOLOV3", "YOLOV4"])
def test_every_shipped_head_records_on_this_backbone_or_says_why_not(head, monkeypatch):
    """Each detector on ShuffleNetV2 x1 either records with the backbone inside the plan or raises a PlanUnsupported that names what
    is not covered -- never an assertion or a wrong plan."""
    from ssds.modeling import nets
    from ssds.modeling import ssds as heads
    from ssds.modeling.layers import planner

    monkeypatch.setenv("SSDK_SHUFFLEUNIT", "1")
    cls = getattr(heads, head)
    size = {"SSDShelf": (2, 3, 97, 65)}.get(head, (2, 3, 128, 64))
    if head == "SSD":
        fl = [[2, 3, 4, "Conv:S", "Conv:S"], [116, 232, 464, 512, 256]]
    elif head == "YOLOV3":
        fl = [[2, 3, 4], [116, 232, 464]]
    elif head == "YOLOV4":
        fl = [[2, 3, 4, "Conv:S"], [116, 232, 464, 256]]
    elif head == "SSDShelf":
        fl = [[2, 3, 4, "Conv:S", "Conv:S"], [116, 232, 464, 256, 256]]
    else:
        fl = [[2, 3, 4, "Conv:S", "Conv:S"], [116, 232, 464, 464, 256]]
    torch.manual_seed(0)
    outputs, extras, hd = cls.add_extras(feature_layer=fl, mbox=[6] * len(fl[0]), num_classes=3)
    model = cls(backbone=nets.ShuffleNetV2_x1(outputs=outputs), extras=extras, head=hd, num_classes=3).eval().to(torch.bfloat16)
    x = torch.zeros(size, dtype=torch.bfloat16)
    try:
        plan = planner.build_ssd_plan(model, x) if head == "SSD" else model._build_neck_plan(None, image=x)
    except planner.PlanUnsupported as e:
        assert str(e), head
        print(head, "refused:", e)
        return
    kinds = [L.get("kind") for L in plan.layers]
    assert kinds.count("shuffle") == 13 and kinds.count("shuffledown") == 3
    print(head, "records", len(kinds), "ops")
