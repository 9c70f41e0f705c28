"""Guard-band tests of the inference path: kernels touch only the buffers they are handed (include/ssdk.h: "the caller owns every
buffer ... kernels fully write their outputs").  The procedure is tests/guardband.py; tests/test_guardband_cpu.py shows it failing.

Part A  every single-launch inference kernel behind ssdk_conv / ssdk_mbconv / ssdk_xpair / ssdk_fuse / ssdk_conv_stem7 /
        ssdk_maxpool3x3s2 / ssdk_mbse: one table (GUARD_CASES) whose rows name the kernel ``N.last_kernel()`` must report.
        Per row and 16-bit dtype: a clean run on ordinary allocations; a guarded run (every input, every tensor of every pack and
        every output between NaN guards: same bits as the clean run, no NaN, every guard and every input interior unchanged); a
        run with image 1 of the batch entirely NaN (every other image keeps the bits of the clean run); and in one dtype per row
        the guarded output against the fp32 reference by the bar of tests/test_gpu_conv.py.
Part B  the plan executor: every recorded detector plan on an arena filled with 0xFF, then 0x00, and on NaN head tensors.
Part C  decode / NMS: +Inf guards around the scores, NaN around the deltas, guarded outputs / mid tensors / workspace, and a
        grown workspace filled with 0xFF, 0x00 and another call's leftovers.

Every criterion is bit equality or "no NaN"; only the comparison with the reference in Part A carries that file's tolerance.
What the method cannot see: a read whose value a select then discards (it changes no result), and an access further from a
tensor than its guard (4096 elements plus one image on each side)."""
import contextlib
from collections import OrderedDict

import numpy as np
import pytest

import cases
import cases_effnet
import cases_shelf
import cases_yolo
import guardband as G
import nethelp

pytestmark = pytest.mark.gpu

POISON = 1  # the image of the batch that is NaN in the third run: interior (every row has >= 3 images), and in the rows of the
            # batch-folding kernels one that shares a workgroup with its neighbours


# ---- Part A: the table ----------------------------------------------------------------------------------------------------------
GEMM, WAVE, G256, GEMMP, PWFLOW = "conv_gemm_kernel", "conv_wave_kernel", "conv_gemm256_kernel", "conv_gemmp_kernel", "pwflow_kernel"
HALO, SHORT, SMALLMAP, FIRST, DW = "conv3x3_halo_kernel", "conv3x3_short_kernel", "conv_smallmap_kernel", "conv_first_kernel", "dwconv3x3_kernel"
G16, G16T, GANY = "gconv3x3_g16_kernel", "gconv3x3_g16_tile_kernel", "gconv3x3_any_kernel"
MBSE = "mbse_dw_kernel+mbse_gate_kernel+mbse_proj_kernel"


def conv(kernel, cin, cout, k, stride, h, w, n, act, **kw):
    return dict(entry="conv", kernel=kernel, cin=cin, cout=cout, k=k, stride=stride, h=h, w=w, n=n, act=act, **kw)


def mb(kernel, cin, cout, stride, h, w, n, variant, **kw):
    return dict(entry="mbconv", kernel=kernel, cin=cin, cout=cout, stride=stride, h=h, w=w, n=n, variant=variant, **kw)


GUARD_CASES = [
    # conv_gemm_kernel (more than 256 output pixels each: fewer go to conv_wave_kernel)
    conv(GEMM, 24, 144, 1, 1, 9, 7, 5, "relu6"),                    # K below one k-step
    conv(GEMM, 32, 16, 1, 1, 33, 31, 3, "none"),                    # N = 16 tile
    conv(GEMM, 128, 40, 3, 2, 7, 9, 16, "sigmoid"),                 # odd map, Cout not a multiple of 16
    conv(GEMM, 512, 256, 1, 1, 12, 12, 3, "relu", splitk=True),     # 8 tiles x 16 k-steps: split-K through the caller's scratch
    conv(WAVE, 64, 64, 1, 1, 2, 2, 8, "none", res="half"),
    conv(G256, 1064, 200, 1, 1, 45, 50, 16, "silu"),                # ragged everything
    conv(GEMMP, 1024, 256, 1, 1, 64, 64, 16, "none", res="half"),
    conv(PWFLOW, 64, 256, 1, 1, 64, 64, 8, "relu"),
    # conv3x3_halo_kernel
    conv(HALO, 40, 128, 3, 1, 32, 32, 24, "relu"),                  # Cin < 64: one partial slab, masked lanes
    conv(HALO, 64, 720, 3, 1, 19, 19, 16, "relu", nchw=True),       # odd map: ragged patches, scalar NCHW stores
    conv(HALO, 384, 504, 3, 1, 8, 8, 96, "none"),                   # four whole maps per tile
    conv(HALO, 256, 256, 3, 1, 16, 16, 48, "none", res="same"),
    # a 10x10 FPN tower level: too few GEMM tiles, so a split-K is planned, and the halo kernel takes the layer WITH that split
    # -- its slabs are laid out per halo tile, larger than the GEMM's (docs/HISTORY.md round 4: they once ran past the scratch)
    conv(HALO, 256, 256, 3, 1, 10, 10, 32, "relu", splitk=True),
    conv(HALO, 96, 504, 3, 1, 32, 32, 8, "none", nchw=True, split=24, act2="sigmoid", heads=True),   # loc | conf: y and y2
    # conv3x3_short_kernel
    conv(SHORT, 32, 132, 3, 1, 64, 64, 8, "none"),
    conv(SHORT, 128, 256, 3, 1, 40, 40, 20, "relu"),
    # conv_smallmap_kernel on the fragment image and on the KRSC tensor
    conv(SMALLMAP, 512, 504, 3, 1, 8, 8, 5, "sigmoid", nchw=True),
    conv(SMALLMAP, 512, 504, 3, 1, 8, 8, 5, "sigmoid", nchw=True, wfrag=False),
    conv(SMALLMAP, 256, 504, 3, 1, 4, 4, 66, "none"),
    conv(SMALLMAP, 256, 504, 3, 1, 4, 4, 66, "none", wfrag=False),
    conv(SMALLMAP, 128, 504, 3, 1, 3, 5, 9, "none"),
    conv(SMALLMAP, 128, 504, 3, 1, 3, 5, 9, "none", wfrag=False),
    conv(SMALLMAP, 128, 100, 3, 2, 4, 4, 70, "silu"),
    # (the stride-2 instance exists for the fragment image only: on the KRSC tensor the layer is conv_gemm_kernel's)
    conv(GEMM, 128, 100, 3, 2, 4, 4, 70, "silu", wfrag=False),
    conv(FIRST, 3, 32, 3, 2, 33, 30, 3, "relu6", layout="nchw"),
    conv(FIRST, 3, 32, 3, 2, 33, 30, 3, "relu6", layout="nhwc"),
    conv(DW, 96, 96, 3, 2, 17, 15, 3, "relu6", groups=96),
    conv(DW, 8, 8, 3, 2, 6, 6, 3, "relu6", groups=8),
    conv(DW, 960, 960, 3, 1, 5, 3, 3, "relu6", groups=960),
    conv(G16, 288, 288, 3, 1, 9, 7, 3, "relu", groups=18),          # 7 wide: narrower than the tile kernel's 8 output columns
    conv(G16T, 208, 208, 3, 2, 40, 24, 3, "relu", groups=13),
    conv(GANY, 168, 168, 3, 1, 33, 31, 3, "relu", groups=7),        # tests/test_gpu_gconv_any.py LAYERS (24, 7, 1, 33, 31, 3)
    conv(GANY, 128, 128, 3, 2, 33, 31, 3, "relu", groups=32),       # LAYERS (4, 32, 2, 33, 31, 3): pairs of groups merged
    dict(entry="stem7", kernel="stem7_kernel", h=75, w=53, n=3, layout="nchw"),
    dict(entry="stem7", kernel="stem7_kernel", h=75, w=53, n=3, layout="nhwc"),
    dict(entry="maxpool", kernel="maxpool3x3s2_kernel", c=64, h=75, w=53, n=3),
    dict(entry="fuse", kernel="fuse_kernel", form="bottom_up", n=3),
    dict(entry="fuse", kernel="fuse_kernel", form="top_down", n=3),
    dict(entry="xpair", kernel="xpair_kernel", cin=512, cmid=128, cout=256, h=8, w=8, n=5),
    dict(entry="xpair", kernel="xpair_kernel", cin=256, cmid=128, cout=256, h=3, w=5, n=7),   # 15 pixels, a ragged last image group
    dict(entry="xpair", kernel="xpair_kernel", cin=256, cmid=64, cout=128, h=2, w=2, n=7, wfrag=False),
    dict(entry="xpair", kernel="xpair_kernel", cin=128, cmid=64, cout=128, h=1, w=1, n=4),
    mb("mbflow_kernel", 24, 24, 1, 33, 30, 3, 1),                   # residual
    mb("mbflow_kernel", 16, 24, 2, 61, 45, 3, 1),
    mb("mbflow_kernel(stem)", 3, 16, 1, 37, 45, 3, 1, stem="nchw"),  # odd height: the bottom segment on the 2-byte gather
    mb("mbflow_kernel(stem)", 3, 16, 1, 37, 45, 3, 1, stem="nhwc"),
    mb("mbsplit_kernel", 32, 32, 1, 31, 47, 3, 2),                  # residual
    mb("mbsplit_kernel", 24, 32, 2, 70, 45, 3, 2),
    mb("mbk_kernel", 160, 160, 1, 5, 16, 3, 3),                     # 16 wide, residual, an odd number of rows
    mb("mbk_kernel", 96, 96, 1, 3, 32, 3, 3),                       # 32 wide, residual
    mb("mbk_kernel", 96, 160, 2, 10, 32, 3, 3),                     # 32 -> 16 columns
    mb("mbk_kernel", 32, 32, 1, 5, 64, 3, 3),                       # 64 wide, residual
    mb("mbk_kernel", 32, 64, 2, 6, 64, 3, 3),
    mb("mbconv_kernel", 64, 64, 1, 8, 8, 3, -1),                    # residual
    mb("mbconv_kernel", 96, 160, 2, 13, 13, 3, -1),
    mb("mbconv_kernel(16x16)", 24, 24, 1, 90, 83, 8, -1),  # 6 x 6 x 8 = 288 tiles of 16 x 16, ragged right / bottom
    mb("mbconv_kernel(stem)", 3, 16, 1, 37, 45, 3, -1, stem="nchw"),
    dict(entry="mbse", kernel=MBSE, cin=40, cout=40, expand=6, k=5, stride=1, h=19, w=17, n=3),   # residual, two tiles
    dict(entry="mbse", kernel=MBSE, cin=24, cout=40, expand=6, k=3, stride=2, h=9, w=5, n=3),
]

# what the table must reach, no more and no less (the mbconv_kernel rows report their instance)
KERNELS = {GEMM, WAVE, G256, GEMMP, PWFLOW, HALO, SHORT, SMALLMAP, FIRST, DW, G16, G16T, GANY, "stem7_kernel", "maxpool3x3s2_kernel",
           "fuse_kernel", "xpair_kernel", "mbflow_kernel", "mbflow_kernel(stem)", "mbsplit_kernel", "mbk_kernel", "mbconv_kernel",
           "mbconv_kernel(16x16)", "mbconv_kernel(stem)", "mbse_dw_kernel", "mbse_gate_kernel", "mbse_proj_kernel"}
REACHED = {}  # row index -> set of dtypes whose dispatch assertion held


def _case_id(i):
    c = GUARD_CASES[i]
    bits = [c["entry"]] + [str(c[k]) for k in ("cin", "cmid", "cout", "k", "stride", "h", "w", "n", "form") if k in c]
    bits += [k for k in ("nchw", "heads", "splitk") if c.get(k)] + [str(c[k]) for k in ("res", "layout", "stem") if c.get(k)]
    if c.get("wfrag") is False:
        bits.append("krsc")
    if "variant" in c:
        bits.append("v%d" % c["variant"])
    return "%02d-%s" % (i, "-".join(bits))


@contextlib.contextmanager
def _wfrag(on):
    from ssds.modeling.layers import fused_conv as FC

    old = FC.USE_WFRAG
    FC.USE_WFRAG = bool(on)
    try:
        yield
    finally:
        FC.USE_WFRAG = old


def _randomize(mods, dtype, gain=1.0):
    import torch

    for m in mods:
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.normal_(0, 0.2)
            m.running_var.uniform_(0.5, 1.5)
            m.weight.data.uniform_(0.5, 1.5)
            m.bias.data.normal_(0, 0.2)
        if isinstance(m, torch.nn.Conv2d):
            m.weight.data = (m.weight.data * gain).to(dtype).float()


def _cl(t):
    import torch

    return t.cuda().contiguous(memory_format=torch.channels_last)


class Ops(object):
    """One row in one dtype: ``inputs`` (name -> device tensor as the kernel takes it), ``packs()`` (fresh packs, equal from call
    to call), ``outs`` [(name, shape, dtype, memory format)], ``call(inputs, packs, outs | None)`` -> {name: tensor} and
    ``judge(got)``: the guarded outputs against the reference."""
    width = None    # the map width an MbPack's image is built for
    ws_args = None  # ssdk_conv rows: the arguments of ssdk_conv_workspace_bytes


def _build_conv(c, dtype):
    import torch
    import torch.nn as nn
    import torch.nn.functional as F
    from ssds.modeling.layers import fused_conv as FC
    from test_gpu_conv import _check, _ref

    cin, cout, k, stride, h, w, n, act = (c[key] for key in ("cin", "cout", "k", "stride", "h", "w", "n", "act"))
    groups, res, nchw, split, act2 = c.get("groups", 1), c.get("res"), c.get("nchw", False), c.get("split"), c.get("act2")
    torch.manual_seed(cin * 131 + cout + k + h)
    if c.get("heads"):
        loc, conf = nn.Conv2d(cin, split, 3, padding=1), nn.Conv2d(cin, cout - split, 3, padding=1)
        for m in (loc, conf):
            m.weight.data = (m.weight.data * 3).to(dtype).float()
            m.bias.data.normal_(0, 0.5)
        loc, conf, bn = loc.cuda(), conf.cuda(), None
        make = lambda: FC.pack_heads(loc, conf, dtype)  # noqa: E731
    else:
        cv = nn.Conv2d(cin, cout, k, stride, k // 2, groups=groups, bias=False)
        bn = nn.BatchNorm2d(cout)
        _randomize([cv, bn], dtype)
        cv, bn = cv.cuda(), bn.cuda()
        make = lambda: FC.ConvPack(cv, bn, act, dtype)  # noqa: E731
    x = (torch.rand if cin <= 4 else torch.randn)(n, cin, h, w).to(dtype)
    ho, wo = (h + 2 * (k // 2) - k) // stride + 1, (w + 2 * (k // 2) - k) // stride + 1
    o = Ops()
    o.inputs = OrderedDict(x=x.cuda() if c.get("layout") == "nchw" else _cl(x))
    r = None
    if res:
        r = torch.randn((n, cout, ho // 2, wo // 2) if res == "half" else (n, cout, ho, wo)).to(dtype)
        o.inputs["residual"] = _cl(r)
    o.packs = lambda: [make()]
    fmt = torch.contiguous_format if nchw else torch.channels_last
    o.outs = [("y", (n, split if split else cout, ho, wo), dtype, fmt)] + ([("y2", (n, cout - split, ho, wo), dtype, fmt)] if split else [])
    o.ws_args = (n, cin, h, w, cout, k, stride)
    kw = dict(nchw_out=nchw, split=split, act2=act2, res_mode={None: 0, "same": 0, "half": 1}[res])
    if c.get("heads"):
        kw["act"] = "none"

    def call(inp, packs, outs):
        with _wfrag(c.get("wfrag", True)):
            got = FC.conv_native(inp["x"], packs[0], residual=inp.get("residual"), y=outs and outs["y"],
                                 y2=outs and outs.get("y2"), **kw)
        return OrderedDict(zip(("y", "y2"), got)) if split else OrderedDict(y=got)

    def judge(got):
        what = _case_id(GUARD_CASES.index(c))
        if c.get("heads"):
            _check(got["y"], _ref(x, loc, None, "none"), dtype, what + " loc")
            _check(got["y2"], _ref(x, conf, None, act2), dtype, what + " conf")
        elif res == "half":
            want = _ref(x, cv, bn, act).to(dtype).float() + F.interpolate(r.float(), scale_factor=2, mode="nearest")
            _check(got["y"], want, dtype, what, floor=1.0)
        elif res == "same":
            _check(got["y"], _ref(x, cv, bn, act, r), dtype, what, floor=1.0)
        else:
            _check(got["y"], _ref(x, cv, bn, act), dtype, what)

    o.call, o.judge = call, judge
    with _wfrag(c.get("wfrag", True)):  # (a pack built with the switch off carries no fragment image: checked where it matters)
        probe = make()
        has_frag = probe.kind == "dense" and probe.frag() is not None
    assert has_frag == (c.get("wfrag", True) and groups == 1 and cin % 32 == 0 and cin > 4)
    return o


def _block_want(mods_chain, x, dtype, residual):
    """A MobileNetV2 block in fp32 with the intermediate tensors rounded to the model dtype (tests/test_gpu_conv.py)."""
    import torch

    with torch.no_grad():
        y = x.float()
        for i, m in enumerate(mods_chain):
            y = m(y)
            if i < len(mods_chain) - 1:
                y = y.to(dtype).float()
        if residual:
            y = y.to(dtype).float() + x.float()
    return y


def _build_mbconv(c, dtype):
    import torch
    from ssds.modeling.layers import fused_conv as FC
    from ssds.modeling.layers.planner import groups_of
    from ssds.modeling.nets.mobilenet import ConvBNReLU6, InvertedResidual
    from test_gpu_conv import _check

    cin, cout, stride, h, w, n = (c[key] for key in ("cin", "cout", "stride", "h", "w", "n"))
    torch.manual_seed(cin * 7 + cout + stride + h)
    o = Ops()
    if c.get("stem"):
        stem, blk = ConvBNReLU6(3, 32, stride=2).eval(), InvertedResidual(32, cout, 1, 1).eval()
        _randomize(list(stem.modules()) + list(blk.modules()), dtype, 2.0)
        x = torch.rand(n, 3, h, w).to(dtype)
        mods = list(blk.conv.children())
        want = _block_want([stem, mods[0], torch.nn.Sequential(mods[1], mods[2])], x, dtype, False)
        stem, blk = stem.cuda(), blk.cuda()
        sg, bg = groups_of(stem), groups_of(blk.conv)
        assert FC.MbPack.stem_supported(sg, bg)
        o.packs = lambda: [FC.MbPack(bg, False, dtype, stem_group=sg[0])]
        o.inputs = OrderedDict(x=x.cuda() if c["stem"] == "nchw" else _cl(x))
        hs, ws_ = (h + 2 - 3) // 2 + 1, (w + 2 - 3) // 2 + 1
        ho, wo = hs, ws_
    else:
        blk = InvertedResidual(cin, cout, stride, 6).eval()
        _randomize(blk.modules(), dtype, 2.0)
        x = torch.randn(n, cin, h, w).to(dtype)
        mods = list(blk.conv.children())
        want = _block_want([mods[0], mods[1], torch.nn.Sequential(mods[2], mods[3])], x, dtype, blk.use_res_connect)
        assert blk.use_res_connect == (stride == 1 and cin == cout)
        blk = blk.cuda()
        groups = groups_of(blk.conv)
        assert FC.MbPack.supported(groups, blk.use_res_connect)
        o.packs = lambda: [FC.MbPack(groups, blk.use_res_connect, dtype)]
        o.inputs = OrderedDict(x=_cl(x))
        ho, wo = (h + 2 - 3) // stride + 1, (w + 2 - 3) // stride + 1
        o.width = w
    o.outs = [("y", (n, cout, ho, wo), dtype, torch.channels_last)]
    o.call = lambda inp, packs, outs: OrderedDict(y=FC.mbconv_native(inp["x"], packs[0], variant=c["variant"], y=outs and outs["y"]))
    o.judge = lambda got: _check(got["y"], want, dtype, _case_id(GUARD_CASES.index(c)), floor=1.0)
    return o


def _build_xpair(c, dtype):
    import torch
    from ssds.modeling.layers import fused_conv as FC
    from ssds.modeling.layers.basic_layers import ConvBNReLU
    from ssds.modeling.layers.planner import groups_of
    from test_gpu_conv import _check

    cin, cmid, cout, h, w, n = (c[key] for key in ("cin", "cmid", "cout", "h", "w", "n"))
    torch.manual_seed(cin + cmid + h)
    layer = torch.nn.Sequential(ConvBNReLU(cin, cmid, 1), ConvBNReLU(cmid, cout, 3, stride=2)).eval()
    _randomize(layer.modules(), dtype, 2.0)
    x = torch.randn(n, cin, h, w).to(dtype)
    with torch.no_grad():
        want = layer[1](layer[0](x.float()).to(dtype).float())
    layer = layer.cuda()
    (c1, b1, a1), (c2, b2, a2) = groups_of(layer)
    o = Ops()
    o.inputs = OrderedDict(x=_cl(x))

    def packs():
        with _wfrag(c.get("wfrag", True)):
            p1, p2 = FC.ConvPack(c1, b1, a1, dtype), FC.ConvPack(c2, b2, a2, dtype)
            assert FC.xpair_supported(p1, p2, h, w) and (p1.frag() is not None) == c.get("wfrag", True)
        return [p1, p2]

    def call(inp, pk, outs):
        with _wfrag(c.get("wfrag", True)):
            return OrderedDict(y=FC.xpair_native(inp["x"], pk[0], pk[1], y=outs and outs["y"]))

    o.packs, o.call = packs, call
    o.outs = [("y", tuple(want.shape), dtype, torch.channels_last)]
    o.judge = lambda got: _check(got["y"], want, dtype, _case_id(GUARD_CASES.index(c)))
    return o


def _build_fuse(c, dtype):
    import torch
    import torch.nn.functional as F
    from ssds import _native as N
    from ssds.modeling.layers import fused_conv as FC
    from test_gpu_conv import _check

    n = c["n"]
    torch.manual_seed(3)
    a = torch.randn(n, 64, 14, 10).to(dtype)
    o = Ops()
    o.packs = lambda: []
    if c["form"] == "top_down":
        up = torch.randn(n, 64, 7, 5).to(dtype)
        o.inputs = OrderedDict(a=_cl(a), b=_cl(up))
        want = 0.25 * a.float() + 0.75 * F.interpolate(up.float(), scale_factor=2, mode="nearest")
        o.call = lambda inp, pk, outs: OrderedDict(y=FC.fuse_native(inp["a"], inp["b"], None, (0.25, 0.75, 0.0), N.FUSE_UP2,
                                                                    y=outs and outs["y"]))
    else:
        big = torch.randn(n, 64, 29, 21).to(dtype)  # odd: max_pool2d floors to 14 x 10
        skip = torch.randn(n, 64, 14, 10).to(dtype)
        o.inputs = OrderedDict(a=_cl(a), b=_cl(big), c=_cl(skip))
        want = 0.5 * a.float() + 0.3 * F.max_pool2d(big.float(), 2) + 0.2 * skip.float()
        o.call = lambda inp, pk, outs: OrderedDict(y=FC.fuse_native(inp["a"], inp["b"], inp["c"], (0.5, 0.3, 0.2), N.FUSE_POOL2,
                                                                    N.FUSE_SAME, y=outs and outs["y"]))
    o.outs = [("y", (n, 64, 14, 10), dtype, torch.channels_last)]
    o.judge = lambda got: _check(got["y"], want, dtype, "fuse " + c["form"])
    return o


def _build_stem7(c, dtype):
    import torch
    import torch.nn as nn
    from ssds.modeling.layers import fused_conv as FC
    from test_gpu_conv import _check, _ref

    n, h, w = c["n"], c["h"], c["w"]
    torch.manual_seed(h + w)
    cv, bn = nn.Conv2d(3, 64, 7, 2, 3, bias=False), nn.BatchNorm2d(64)
    _randomize([cv, bn], dtype)
    x = torch.randn(n, 3, h, w).to(dtype)
    want = _ref(x, cv, bn, "relu")
    cv, bn = cv.cuda(), bn.cuda()
    assert FC.StemPack.supported(cv, bn)
    o = Ops()
    o.inputs = OrderedDict(x=x.cuda() if c["layout"] == "nchw" else _cl(x))
    o.packs = lambda: [FC.StemPack(cv, bn, "relu", dtype)]
    o.outs = [("y", tuple(want.shape), dtype, torch.channels_last)]
    o.call = lambda inp, pk, outs: OrderedDict(y=FC.stem7_native(inp["x"], pk[0], y=outs and outs["y"]))
    o.judge = lambda got: _check(got["y"], want, dtype, "stem 7x7 " + c["layout"])
    return o


def _build_maxpool(c, dtype):
    import torch
    import torch.nn.functional as F
    from ssds.modeling.layers import fused_conv as FC

    n, ch, h, w = c["n"], c["c"], c["h"], c["w"]
    torch.manual_seed(h)
    x = torch.randn(n, ch, h, w).to(dtype)
    want = F.max_pool2d(x.float(), 3, 2, 1)
    o = Ops()
    o.inputs = OrderedDict(x=_cl(x))
    o.packs = lambda: []
    o.outs = [("y", tuple(want.shape), dtype, torch.channels_last)]
    o.call = lambda inp, pk, outs: OrderedDict(y=FC.maxpool_native(inp["x"], y=outs and outs["y"]))

    def judge(got):
        assert torch.equal(got["y"].float().cpu(), want), "maxpool must be exact"

    o.judge = judge
    return o


def _build_mbse(c, dtype):
    import torch
    import mbseaudit
    from ssds.modeling.layers import fused_conv as FC

    n, h, w = c["n"], c["h"], c["w"]
    blk = mbseaudit.make_block(c["cin"], c["cout"], c["expand"], c["k"], c["stride"], seed=41 + c["k"]).cuda()
    pk0 = FC.MbSePack(blk, dtype)
    g = torch.Generator().manual_seed(8 + c["k"])
    x = _cl(torch.randn(n, pk0.cin, h, w, generator=g).to(dtype))
    ho, wo = FC._out_hw(h, w, pk0.k, pk0.stride)
    o = Ops()
    o.inputs = OrderedDict(x=x)
    if pk0.residual:
        o.inputs["residual"] = _cl(torch.randn(n, pk0.cout, ho, wo, generator=g).to(dtype))
    assert pk0.residual == (c["stride"] == 1 and c["cin"] == c["cout"])
    tiles = FC.mbse_pool_tiles(h, w, pk0.k, pk0.stride)
    o.packs = lambda: [FC.MbSePack(blk, dtype)]
    o.outs = [("t", (n, pk0.cin, ho, wo), dtype, torch.channels_last), ("pool_partial", (n, tiles, pk0.cin), torch.float32, torch.contiguous_format),
              ("gate", (n, pk0.cin), torch.float32, torch.contiguous_format), ("y", (n, pk0.cout, ho, wo), dtype, torch.channels_last)]
    o.call = lambda inp, pk, outs: OrderedDict(FC.mbse_native(inp["x"], pk[0], residual=inp.get("residual"), **(outs or {})))

    def judge(got):
        lines = []
        bad = mbseaudit.judge(pk0, x, o.inputs.get("residual"), dict(got), dtype, stages=7, lines=lines)
        print("; ".join(lines))
        assert not bad, bad

    o.judge = judge
    return o


BUILDERS = dict(conv=_build_conv, mbconv=_build_mbconv, xpair=_build_xpair, fuse=_build_fuse, stem7=_build_stem7,
                maxpool=_build_maxpool, mbse=_build_mbse)


def _run(o, inputs, packs, outs=None):
    import torch
    from ssds import _native as N

    got = o.call(inputs, packs, outs)
    torch.cuda.synchronize()
    return got, N.last_kernel()


@pytest.mark.parametrize("dtype_name", ["bf16", "f16"])
@pytest.mark.parametrize("i", range(len(GUARD_CASES)), ids=_case_id)
def test_kernel_touches_only_its_buffers(i, dtype_name, monkeypatch):
    import torch
    from ssds import _native as N

    c = GUARD_CASES[i]
    dtype = torch.bfloat16 if dtype_name == "bf16" else torch.float16
    o = BUILDERS[c["entry"]](c, dtype)
    assert c["n"] >= 3, "image %d must be interior" % POISON
    # ssdk_conv rows whose geometry has a split-K plan (whichever kernel then takes the layer) get their scratch guarded too
    need = int(N.lib.ssdk_conv_workspace_bytes(*(o.ws_args + (N._DTYPES[dtype],)))) if o.ws_args else 0
    assert need or not c.get("splitk"), "the split-K row must come with a workspace"

    # 1. clean run: ordinary allocations
    clean, kernel = _run(o, o.inputs, o.packs())
    assert kernel == c["kernel"], "dispatched to %s" % kernel
    REACHED.setdefault(i, set()).add(dtype_name)
    for name, t in clean.items():
        assert not G.has_nan(t), "clean run: NaN in " + name

    # 2. guarded run: every input, every pack tensor, every output (and the split-K scratch) between guards
    gs = G.GuardSet("cuda")
    ginputs = OrderedDict((name, gs.inp(name, t)) for name, t in o.inputs.items())
    gpacks = o.packs()
    with _wfrag(c.get("wfrag", True)):
        for pi, pk in enumerate(gpacks):
            for name, storage, view in G.guard_pack(pk, width=o.width):
                gs.adopt("pack%d.%s" % (pi, name), storage, view)
    gouts = OrderedDict((name, gs.out(name, shape, dt, fmt)) for name, shape, dt, fmt in o.outs)
    scratch = {}
    if need:
        # conv_native takes the scratch from N.scratch and passes its length on: hand it a guarded, zero-filled one of exactly
        # ssdk_conv_workspace_bytes (not the 256 bytes of alignment slack conv_native asks for on top: the view is aligned, and a
        # slab layout that overran the library's own figure by a few bytes would hide in them)

        def guarded_scratch(device, user, nbytes):
            assert user == "splitk" and nbytes == need + 256 and not scratch
            scratch["ws"] = gs.zeros("splitk scratch", need)
            assert scratch["ws"].data_ptr() % 256 == 0 and scratch["ws"].numel() == need
            gs.arm()
            return scratch["ws"]

        monkeypatch.setattr(N, "scratch", guarded_scratch)
    else:
        gs.arm()
    got, kernel = _run(o, ginputs, gpacks, gouts)
    monkeypatch.undo()
    assert kernel == c["kernel"], "guarded run dispatched to %s" % kernel
    assert list(got) == list(clean)
    for name, t in got.items():
        assert t.data_ptr() == gouts[name].data_ptr(), name + " is not the buffer handed in"
        assert not G.has_nan(t), "guarded run: NaN in %s -- an element never written, or a guard value that reached arithmetic" % name
        assert G.same_bits(t, clean[name]), "guarded run: %s differs from the clean run" % name
    assert gs.problems() == []
    if need:
        assert scratch and int(scratch["ws"][:4096].count_nonzero()) == 0, "the split-K tickets were not left at zero"
        if c.get("splitk"):  # (the slabs behind the 4 KiB of tickets hold partial sums: the split path is the one that ran)
            assert int(scratch["ws"][4096:].count_nonzero()) > 0, "the row did not run split-K"

    # 3. one poisoned image: the same dispatch, image POISON of x (and of the residual / skip inputs) entirely NaN
    pinputs = OrderedDict((name, t.clone()) for name, t in o.inputs.items())
    for t in pinputs.values():
        t[POISON] = float("nan")
    pois, kernel = _run(o, pinputs, o.packs())
    assert kernel == c["kernel"], "poisoned run dispatched to %s" % kernel
    keep = [j for j in range(c["n"]) if j != POISON]
    for name, t in pois.items():
        assert G.same_bits(t[keep], clean[name][keep]), "%s: image %d leaked into another image" % (name, POISON)

    # 4. the table stays on layers the reference covers (one dtype per row: the reference is the slow part)
    if dtype_name == ("bf16", "f16")[i % 2]:
        o.judge(got)


def test_every_kernel_of_the_list_was_reached():
    """The union of the kernel names the rows reach equals KERNELS, every row in both dtypes.  Rows whose test ran before this
    one in the same process have left their dispatch in REACHED; any other (the test selected alone, another order, another
    process) is dispatched here once more, so the test stands on its own."""
    import torch

    names = set()
    for i, c in enumerate(GUARD_CASES):
        for dtype_name, dtype in (("bf16", torch.bfloat16), ("f16", torch.float16)):
            if dtype_name not in REACHED.get(i, ()):
                o = BUILDERS[c["entry"]](c, dtype)
                _, kernel = _run(o, o.inputs, o.packs())
                assert kernel == c["kernel"], "%s %s dispatched to %s" % (_case_id(i), dtype_name, kernel)
                REACHED.setdefault(i, set()).add(dtype_name)
        names.update(c["kernel"].split("+"))
    assert all(REACHED[i] == {"bf16", "f16"} for i in range(len(GUARD_CASES)))
    assert names == KERNELS, (sorted(names - KERNELS), sorted(KERNELS - names))


def test_a_scale_vector_one_element_short_shows_in_the_output():
    """The procedure on the device, with a real kernel as the dishonest party: ``scale`` is handed over one element short, so the
    kernel's (legitimate) read of channel Cout - 1 lands on the first guard element -- inside the test's own allocation.  That
    channel, and nothing else, must come back NaN."""
    import torch
    import torch.nn as nn
    from ssds import _native as N
    from ssds.modeling.layers import fused_conv as FC

    dtype = torch.bfloat16
    torch.manual_seed(2)
    cv, bn = nn.Conv2d(32, 16, 1, bias=False), nn.BatchNorm2d(16)
    _randomize([cv, bn], dtype)
    cv, bn = cv.cuda(), bn.cuda()
    x = _cl(torch.randn(3, 32, 33, 31).to(dtype))
    clean = FC.conv_native(x, FC.ConvPack(cv, bn, "none", dtype))
    assert N.last_kernel() == GEMM
    pack = FC.ConvPack(cv, bn, "none", dtype)
    G.guard_pack(pack)
    storage, short = G.guarded(pack.scale[:15].clone())
    pack.scale = short
    y = FC.conv_native(x, pack)
    torch.cuda.synchronize()
    assert bool(torch.isnan(y[:, 15]).all()) and not G.has_nan(y[:, :15]) and G.same_bits(y[:, :15], clean[:, :15])
    assert G.guards_intact(storage, short)


def test_output_keywords_are_validated():
    import torch
    import torch.nn as nn
    from ssds import _native as N
    from ssds.modeling.layers import fused_conv as FC

    dtype = torch.bfloat16
    conv_, bn = nn.Conv2d(32, 16, 1, bias=False).cuda(), nn.BatchNorm2d(16).cuda()
    pack = FC.ConvPack(conv_, bn, "none", dtype)
    x = _cl(torch.randn(2, 32, 5, 5).to(dtype))
    good = torch.empty((2, 16, 5, 5), device="cuda", dtype=dtype).contiguous(memory_format=torch.channels_last)
    assert FC.conv_native(x, pack, y=good).data_ptr() == good.data_ptr()
    assert torch.equal(good, FC.conv_native(x, pack))
    for bad in (torch.empty((2, 16, 5, 5), device="cuda", dtype=dtype),                      # NCHW memory
                good.to(torch.float16), torch.empty((2, 16, 5, 4), device="cuda", dtype=dtype).contiguous(memory_format=torch.channels_last),
                good.cpu()):
        with pytest.raises(N.SsdkError):
            FC.conv_native(x, pack, y=bad)
    with pytest.raises(N.SsdkError):
        FC.conv_native(x, pack, y=good, y2=good)  # no split head: there is no second output
    with pytest.raises(N.SsdkError):
        FC.maxpool_native(x, y=good)
    with pytest.raises(N.SsdkError):
        FC.fuse_native(x, x, y=good)


# ---- Part B: the plan executor on a poisoned arena ------------------------------------------------------------------------------
def _net_cases():
    rows = [("cases", name) for name in cases.NET_CASES if name != "ssd_stub"]  # (a stub backbone under SSD records no plan)
    rows += [("effnet", name) for name in cases_effnet.NET_CASES]
    rows += [("shelf", name) for name in cases_shelf.NET_CASES] + [("yolo", name) for name in cases_yolo.NET_CASES]
    rows = [(fam, name, None) for fam, name in rows]
    # The golden cases are small images: every pyramid level is below planner.SMALL_LEVEL_PIXELS, so no tower chain is recorded
    # for the side stream.  With the bar lowered (as tests/test_gpu_nets.py::test_small_levels_on_the_side_stream_change_nothing
    # lowers it) the levels split into big and small ones and the plan has side-stream chains with pinned buffers.
    rows += [("cases", "fpn_r18", 200), ("cases", "fpn_stub", 200), ("cases", "bifpn_stub", 100)]
    return [(fam, name, small, ("bfloat16", "float16")[k % 2]) for k, (fam, name, small) in enumerate(rows)]


def _build_net(fam, name, monkeypatch):
    if fam == "effnet":
        import mbseaudit

        return mbseaudit.build_case(name)
    if fam != "cases":
        monkeypatch.setattr(nethelp, "cases", cases_shelf if fam == "shelf" else cases_yolo)
    return nethelp.build(name)


@pytest.mark.parametrize("fam,name,small_pixels,dtype", _net_cases(),
                         ids=lambda v: v if isinstance(v, str) else ("chains%d" % v if v else "asis"))
def test_plan_does_not_depend_on_what_the_arena_holds(fam, name, small_pixels, dtype, monkeypatch):
    """The arena's buffers are torch.empty, handed from layer to layer and larger than the tensors they hold: whatever they
    contain -- NaN, zeros -- the outputs are the same bits, and every head element is written.  Plans with ops tagged for the
    side stream (small heads; with ``small_pixels`` the tower chains of the small levels, whose buffers are pinned) repeat the
    0xFF replay with the side lane forced on and forced off: a buffer handed out again while a side-lane op still reads it shows
    there."""
    import torch
    from ssds.modeling.layers import fused_conv as FC
    from ssds.modeling.layers import planner

    tdt = getattr(torch, dtype)
    if small_pixels is not None:
        monkeypatch.setattr(planner, "SMALL_LEVEL_PIXELS", small_pixels)
    model, x, _ = _build_net(fam, name, monkeypatch)
    model = model.cuda().to(tdt)
    xd = x.cuda().to(tdt)
    runs = FC.STATS["plan_runs"]
    with torch.no_grad():
        model(xd)
        A = [t.clone() for pair in model(xd) for t in pair]
    assert FC.STATS["plan_runs"] >= runs + 2, "the forward did not run as a recorded plan"
    if hasattr(model, "_plan"):
        plans = [model._plan(xd)]
    else:
        plans = [p for p in model.__dict__["_neck_plans"].values() if isinstance(p, FC.ConvPlan)]
    assert len(plans) == 1 and isinstance(plans[0], FC.ConvPlan)
    plan = plans[0]
    assert len(plan.arena.bufs) >= 2
    chain_ops = sum(1 for L in plan.layers if L.get("lane") == 2)
    assert plan.side_chain == (small_pixels is not None) and (chain_ops >= 10) == (small_pixels is not None), (plan.side_chain, chain_ops)
    for t in A:
        assert not G.has_nan(t)

    def same(outs, what, want=None):
        want = A if want is None else want
        outs = [t for pair in outs for t in pair]
        torch.cuda.synchronize()
        assert len(outs) == len(want)
        for k, (a, b) in enumerate(zip(outs, want)):
            assert not G.has_nan(a), "%s: NaN in output %d" % (what, k)
            assert G.same_bits(a, b), "%s: output %d differs" % (what, k)

    def fill(byte):
        for buf, _ in plan.arena.bufs:  # (plan.ws, the split-K tickets, is zero by contract and left alone)
            buf.fill_(byte)

    with torch.no_grad():
        for byte in (0xFF, 0x00):
            fill(byte)
            same(model(xd), "arena filled with %#04x" % byte)
        # every head element is written: prepare() hands out the head tensors, launch() fills them
        image = len(plan.inputs) == 1 and plan.inputs[0].shape == tuple(xd.shape)
        ins = (xd,) if image else tuple(model.backbone(xd))
        loc, conf = plan.prepare(*ins)
        for t in loc + conf:
            t.fill_(float("nan"))
        plan.launch()
        same((loc, conf), "heads filled with NaN")
        if any(L.get("lane") for L in plan.layers):  # side-lane heads / chains on the side stream, and the same ops in line
            for on in (True, False):
                plan.ctx.set_side_lane(on)
                # A side-lane HEAD (lane 1) may take another kernel than in line (ssdk_conv prefers the halo kernel there), so
                # the reference is this lane setting's own clean replay, itself repeatable; the chains (lane 2) pick their kernels
                # by their tag, so a plan that has them and no more must also give the bits of A either way.
                fill(0x00)
                base = [t.clone() for pair in model(xd) for t in pair]
                same(model(xd), "side lane %s, replay" % on, base)
                if not any(L.get("lane") == 1 for L in plan.layers):
                    same(model(xd), "side lane %s against the default" % on)
                fill(0xFF)
                same(model(xd), "arena filled with 0xff, side lane %s" % on, base)
            plan.ctx.set_side_lane(None)


# ---- Part C: decode / NMS -------------------------------------------------------------------------------------------------------
def _decode_heads(dtype, seed):
    """B = 3, two levels; level 0 holds 3 * 20 * 24 * 28 = 40320 scores per image -- 19.7 tiles of 256 lanes x 16 bytes in 16 bit
    (39.4 of the fp32 tile), seven units under SSDK_TILES_PER_UNIT=3 -- and level 1 a single, partial tile."""
    import torch
    from oracle import box_oracle as O

    rs = np.random.RandomState(seed)
    A, C, B = 3, 20, 3
    maps, strides = [(24, 28), (6, 7)], [8, 32]
    conf = [torch.from_numpy(cases.sigmoid(rs.standard_normal((B, A * C, h, w)).astype(np.float32) * np.float32(1.5) - np.float32(4.6))).to(dtype)
            for h, w in maps]
    loc = [torch.from_numpy((rs.standard_normal((B, A * 4, h, w)) * 0.5).astype(np.float32)).to(dtype) for h, w in maps]
    anchors = OrderedDict((s, torch.from_numpy(O.generate_anchors(s, [1, 2, 0.5], [2.0]))) for s in strides)
    return loc, conf, anchors


DECODE_ARGS = (0.01, 300, True, 0.6, 100, True)  # threshold, K per level, rescore, NMS threshold, detections, DIoU


def _decode_call(ctx, loc, conf, anchors, args, outs, mids, ws):
    """ssdk_decode_nms_ctx on the test's own pointers, as box.decode_nms calls it."""
    import torch
    from ssds import _native as N

    thr, K, rescore, nms_thr, nd, diou = args
    L, B, dt = len(loc), int(conf[0].shape[0]), N.dtype_code(conf[0])
    levels = (N.Level * L)()
    for i, (c, l, (stride, anchor)) in enumerate(zip(conf, loc, anchors.items())):
        levels[i] = N.make_level(c, l, stride, anchor)
    dev = conf[0].device
    with torch.cuda.device(dev):
        need = int(N.lib.ssdk_decode_nms_workspace_bytes(levels, L, B, dt, K, nd))
        assert need > 0
        if ws is None:
            return need
        assert ws.numel() >= need and ws.data_ptr() % 256 == 0
        ctx.set_tail_stream(None)
        rc = N.lib.ssdk_decode_nms_ctx(ctx.ptr, levels, L, B, dt, float(thr), K, int(rescore), float(nms_thr), nd, int(diou),
                                       outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), mids[0].data_ptr(),
                                       mids[1].data_ptr(), mids[2].data_ptr(), ws.data_ptr(), ws.numel(), N.stream_ptr(dev))
    N.check(rc, "decode_nms")
    torch.cuda.synchronize()
    return need


def _against_oracle(loc, conf, anchors, args, outs, mids, what):
    """tests/test_gpu_box.py::_decoder_vs_oracle on results already computed."""
    from oracle import box_oracle as O
    from test_gpu_box import BOX_ATOL

    oanch = OrderedDict((k, v.numpy()) for k, v in anchors.items())
    odec = O.Decoder(args[0], args[3], args[4], args[1], args[2], args[5])
    ol, oc = [t.float().cpu().numpy() for t in loc], [t.float().cpu().numpy() for t in conf]
    wm = odec.decode_levels(ol, oc, oanch)
    np.testing.assert_array_equal(mids[2].cpu().numpy(), wm[2], err_msg=what + " mid classes")
    np.testing.assert_allclose(mids[1].cpu().numpy(), wm[1], atol=BOX_ATOL, rtol=0, err_msg=what + " mid boxes")
    np.testing.assert_allclose(mids[0].cpu().numpy(), wm[0], atol=1e-4, rtol=1e-4, equal_nan=True, err_msg=what + " mid scores")
    want = odec(ol, oc, oanch)
    np.testing.assert_array_equal(outs[2].cpu().numpy(), want[2], err_msg=what + " classes")
    np.testing.assert_allclose(outs[1].cpu().numpy(), want[1], atol=BOX_ATOL, rtol=0, err_msg=what + " boxes")
    np.testing.assert_allclose(outs[0].cpu().numpy(), want[0], atol=1e-4, rtol=1e-4, err_msg=what + " scores")


@pytest.mark.parametrize("fused", ["1", "0"])
@pytest.mark.parametrize("dtype_name", ["bfloat16", "float16", "float32"])
def test_decode_stage_touches_only_its_buffers(dtype_name, fused, monkeypatch):
    """16-bit heads with a positive threshold and K <= 512 take scan16_kernel, fp32 heads scan_kernel; behind them
    levelsel_kernel + nmswalk_kernel, or with SSDK_DECODE_FUSED=0 (read on every call) level_kernel + nms_kernel.  The scores
    sit between +Inf guards -- a guard element the scan consumed would come back as the top candidate --, the deltas between NaN
    guards; outputs, per-level outputs and the workspace (of exactly the size the library asks for) are guarded as well.  The
    anchors travel by value inside ssdk_level, so there is no anchor buffer to guard.
    The scan dispatch is ASSUMED, not observed: the library reports the last kernel of a call only (asserted: the tail), and its
    profiling rings carry times without names.  The assumption is the rule of launch_scan (ssdk_decode.hip): 16-bit dtype,
    threshold > 0, K <= 512 and units of <= 255 tiles -- all four hold for these head sets by construction."""
    import torch
    from ssds import _native as N

    dtype = getattr(torch, dtype_name)
    monkeypatch.setenv("SSDK_TILES_PER_UNIT", "3")
    monkeypatch.setenv("SSDK_DECODE_FUSED", fused)
    loc, conf, anchors = _decode_heads(dtype, 17)
    assert conf[0][0].numel() % (256 * 16 // conf[0].element_size()) != 0
    B, L, K, nd = 3, 2, DECODE_ARGS[1], DECODE_ARGS[4]
    ctx = N.Context(torch.device("cuda", torch.cuda.current_device()))
    shapes = [(B, nd), (B, nd, 4), (B, nd)], [(B, L * K), (B, L * K, 4), (B, L * K)]
    # clean call: ordinary allocations
    dl, dc = [t.cuda() for t in loc], [t.cuda() for t in conf]
    outs, mids = ([torch.empty(s, device="cuda") for s in grp] for grp in shapes)
    need = _decode_call(ctx, dl, dc, anchors, DECODE_ARGS, outs, mids, None)
    _decode_call(ctx, dl, dc, anchors, DECODE_ARGS, outs, mids, torch.empty(need + 256, dtype=torch.uint8, device="cuda"))
    assert N.last_kernel() == ("nmswalk_kernel" if fused == "1" else "nms_kernel"), N.last_kernel()
    _against_oracle(loc, conf, anchors, DECODE_ARGS, outs, mids, "clean %s fused=%s" % (dtype_name, fused))
    assert float(outs[0].max()) > 0.05, "nothing was detected: the case tests nothing"
    # guarded call
    gs = G.GuardSet("cuda")
    gc = [gs.inp("conf%d" % i, t, fill=G.INF_FILL[dtype]) for i, t in enumerate(conf)]
    gl = [gs.inp("loc%d" % i, t) for i, t in enumerate(loc)]
    gouts = [gs.out("out%d" % i, s, torch.float32) for i, s in enumerate(shapes[0])]
    gmids = [gs.out("mid%d" % i, s, torch.float32) for i, s in enumerate(shapes[1])]
    gws = gs.out("workspace", (need,), torch.uint8)
    gs.arm()
    _decode_call(ctx, gl, gc, anchors, DECODE_ARGS, gouts, gmids, gws)
    assert gs.problems() == []
    for name, a, b in [("out%d" % i, a, b) for i, (a, b) in enumerate(zip(gouts, outs))] + [
            ("mid%d" % i, a, b) for i, (a, b) in enumerate(zip(gmids, mids))]:
        assert not G.has_nan(a) and G.same_bits(a, b), name
    _against_oracle(loc, conf, anchors, DECODE_ARGS, gouts, gmids, "guarded %s fused=%s" % (dtype_name, fused))


@pytest.mark.parametrize("fused", ["1", "0"])
@pytest.mark.parametrize("dtype_name", ["bfloat16", "float32"])
def test_decode_result_does_not_depend_on_what_the_workspace_holds(dtype_name, fused, monkeypatch):
    """N.workspace is torch.empty, grow-only and shared by every call on the stream: grown beyond this call's need and filled
    with 0xFF, with 0x00 and with the leftovers of a call with another K and batch, the results are the same bits."""
    import torch
    from ssds import _native as N
    from ssds.modeling.layers.box import decode_nms

    dtype = getattr(torch, dtype_name)
    monkeypatch.setenv("SSDK_TILES_PER_UNIT", "3")
    monkeypatch.setenv("SSDK_DECODE_FUSED", fused)
    loc, conf, anchors = _decode_heads(dtype, 23)
    dl, dc = [t.cuda() for t in loc], [t.cuda() for t in conf]
    other_l, other_c = [torch.cat([t, t.flip(0)])[:5].contiguous() for t in dl], [torch.cat([t, t.flip(0)])[:5].contiguous() for t in dc]
    dev = dc[0].device
    ctx = N.Context(dev)
    need = _decode_call(ctx, dl, dc, anchors, DECODE_ARGS, None, None, None)
    big = _decode_call(ctx, other_l, other_c, anchors, (0.01, 512, True, 0.6, 100, True), None, None, None)
    ws = N.workspace(dev, 2 * max(need, big) + 4096)
    assert ws.numel() >= 2 * need
    results = []
    for what in ("0xff", "0x00", "leftovers"):
        if what == "leftovers":
            decode_nms(other_l, other_c, anchors, 0.01, 512, True, 0.6, 100, True)
        else:
            ws.fill_(0xFF if what == "0xff" else 0)
        assert N.workspace(dev, need + 256).data_ptr() == ws.data_ptr(), "the call must run on the buffer that was filled"
        (s, b, c), mid = decode_nms(dl, dc, anchors, *DECODE_ARGS, return_mid=True)
        torch.cuda.synchronize()
        results.append((what, [s, b, c] + list(mid)))
    _against_oracle(loc, conf, anchors, DECODE_ARGS, results[0][1][:3], results[0][1][3:], "workspace " + dtype_name)
    for what, res in results[1:]:
        for k, (a, b) in enumerate(zip(res, results[0][1])):
            assert G.same_bits(a, b), "workspace filled with %s: output %d differs from the run on 0xff" % (what, k)
