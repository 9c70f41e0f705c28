"""The dilated 3x3 convolution (csrc/ssdk_dconv.hip behind a 'dilated' ConvPack / conv_native / an SSDK_OP_CONV whose res_mode carries
the dilation) and the RFB extras' plans on the GPU.

Kernel: against fp32 -- ``F.conv2d(..., padding = dilation = d)`` on the 16-bit input and the pack's 16-bit weights, * scale + bias,
activation (rfbaudit.dilated_reference) -- with planaudit's per-op bars ``BARS[dtype]["default"]``; the same output must MISS the bar
against the expression with dilation d - 1, d + 1 and with the taps transposed.  Guard bands around every buffer.

Block and nets: ``planner.record_rfb`` / the detectors' plans, audited op by op (tests/rfbaudit.py), and end to end against the
reference's fp32 outputs (tests/golden/net_*rfb*.npz) by the rule of tests/test_gpu_nets.py -- the floor of PyTorch-ROCm running the
same module in the same dtype."""
import os
import subprocess
import sys

import pytest

import cases_rfb
import guardband as G
import nethelp
import planaudit

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = ["bfloat16", "float16"]
ACTS = ["none", "relu"]
CHANNELS = [(16, 16), (40, 24), (128, 128), (64, 136)]
DILATIONS = [2, 3, 5, 8]
MAPS = range(5)


def _maps(d):
    """(n, h, w) per dilation: 1 x 1 (the centre tap alone); d x (d + 1) (no vertical tap is inside, and exactly the horizontal
    neighbours of the two edge columns are); (d + 1) x (2 d + 1); 13 x 13 at N = 3 (169 pixels: groups of 16 straddle rows and images);
    and a map ragged both ways against the kernel's tile (rows that are no divisor of the 16-pixel group, a pixel tail)."""
    from ssds import _native as N

    tp = N.DCONV_TILE_PIXELS
    return [(2, 1, 1), (2, d, d + 1), (2, d + 1, 2 * d + 1), (3, 13, 13), (2, tp // 2 + 1, tp + 3)]


def _channels_of(di, mi):
    """The pruned grid: (dilation index, map index) -> channel pair, a latin square -- every dilation and every map meets every pair."""
    return CHANNELS[(di + mi) % len(CHANNELS)]


def test_the_parametrisation_covers_the_predicate():
    from ssds import _native as N

    assert DILATIONS[0] == N.DCONV_MIN_DILATION and DILATIONS[-1] == N.DCONV_MAX_DILATION
    tp, fc, tc = N.DCONV_TILE_PIXELS, N.DCONV_FRAG_COUT, N.DCONV_TILE_COUT
    for di, d in enumerate(DILATIONS):
        maps = _maps(d)
        assert len(maps) == len(MAPS)
        assert maps[1][1] == d and maps[1][2] == d + 1 and maps[3] == (3, 13, 13) and (13 * 13) % tp and (3 * 13 * 13) % tp
        n, h, w = maps[4]
        assert tp % w and w > tp and (n * h * w) % tp and (h * w) % tp  # ragged: rows, images and the tail all cut a 16-pixel group
        assert {_channels_of(di, mi) for mi in MAPS} == set(CHANNELS)
        for mi in MAPS:
            cin, cout = _channels_of(di, mi)
            for dt in (N.BF16, N.F16):
                assert N.lib.ssdk_dconv3x3_supported(cin, cout, maps[mi][1], maps[mi][2], d, dt)
    for mi in MAPS:
        assert {_channels_of(di, mi) for di in range(len(DILATIONS))} == set(CHANNELS)
    # the channel pairs: one fragment; Cin with 9 Cin % 32 != 0 and a half-filled fragment; two full tiles of Cout; a Cout that is
    # neither a multiple of the fragment nor of the tile
    assert any((9 * ci) % 32 for ci, _ in CHANNELS) and any(co % fc for _, co in CHANNELS) and any(co > tc and co % tc for _, co in CHANNELS)
    assert any(co % tc == 0 for _, co in CHANNELS)
    assert not N.lib.ssdk_dconv3x3_supported(16, 16, 5, 5, DILATIONS[0] - 1, N.BF16)
    assert not N.lib.ssdk_dconv3x3_supported(16, 16, 5, 5, DILATIONS[-1] + 1, N.BF16)


def _gain(h, w, d):
    """On a small map most taps of the dilated 3x3 fall outside the image and the output shrinks with them: sqrt(9 / mean taps inside)
    (test_gpu_dkres._gain for dilation d), which the BatchNorm's weight is scaled by so that the output keeps the size of x."""
    rows = sum(1 + (y - d >= 0) + (y + d < h) for y in range(h))
    cols = sum(1 + (x - d >= 0) + (x + d < w) for x in range(w))
    return (9.0 * h * w / (rows * cols)) ** 0.5


def _layer(cin, cout, d, dtype, seed, gain=1.0, act="none"):
    """ConvPack of a seeded dilated Conv2d + BatchNorm (cases.seeded_state's distributions; ``gain`` scales the BatchNorm's weight)."""
    import torch
    from ssds.modeling.layers import fused_conv as FC

    g = torch.Generator().manual_seed(seed)
    conv = torch.nn.Conv2d(cin, cout, 3, 1, d, dilation=d, bias=False)
    bn = torch.nn.BatchNorm2d(cout, eps=1e-5, momentum=0.01).eval()
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) * (1.5 / (9 * cin)) ** 0.5)
        bn.weight.copy_((torch.rand(cout, generator=g) + 0.5) * gain)
        bn.bias.copy_(torch.randn(cout, generator=g) * 0.1)
        bn.running_mean.copy_(torch.randn(cout, generator=g) * 0.1)
        bn.running_var.copy_(torch.rand(cout, generator=g) * 0.5 + 0.5)
    pk = FC.ConvPack(conv.cuda(), bn.cuda(), act, dtype)
    assert pk.kind == "dilated" and pk.dilation == d
    return pk


def _input(n, c, h, w, dtype, seed):
    import torch

    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(n, c, h, w, generator=g) * 0.7).to(dtype).cuda()
    return x.contiguous(memory_format=torch.channels_last)


def _figures(got, want, dtype):
    med, p999, mx, _ = planaudit.stats(got, want)
    bar = planaudit.BARS[dtype]["default"]
    return (med, p999, mx), bar, bool(med <= bar[0] and p999 <= bar[1] and mx <= bar[2])


def _within(got, want, dtype, what):
    (med, p999, mx), bar, ok = _figures(got, want, dtype)
    print(what, "median / p99.9 / max = %.5f / %.5f / %.5f of the RMS, bar %s" % (med, p999, mx, bar))
    assert ok, (what, med, p999, mx, bar)


# ---- the kernel --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mi", MAPS)
@pytest.mark.parametrize("di", range(len(DILATIONS)))
@pytest.mark.parametrize("dtype", DTYPES)
def test_kernel_matches_the_fp32_expression(dtype, di, mi):
    import torch
    from rfbaudit import dilated_reference
    from ssds import _native as N
    from ssds.modeling.layers import fused_conv as FC

    tdt = getattr(torch, dtype)
    d = DILATIONS[di]
    n, h, w = _maps(d)[mi]
    cin, cout = _channels_of(di, mi)
    pk = _layer(cin, cout, d, tdt, seed=1000 * d + 10 * mi + cin, gain=_gain(h, w, d))
    x = _input(n, cin, h, w, tdt, seed=17 * cin + mi + d)
    rms = lambda t: float(t.float().pow(2).mean().sqrt())
    for act in ACTS:
        want = dilated_reference(x, pk, act=act)
        # the comparison decides something: the output is of the size of x, and a relu output neither dead nor untouched
        assert rms(want) >= 0.5 * rms(x), (rms(want), rms(x))
        if act == "relu":
            assert 0.05 <= float((want == 0).float().mean()) <= 0.95
        y = FC.conv_native(x, pk, act=act)
        y2 = FC.conv_native(x, pk, act=act)
        torch.cuda.synchronize()
        assert N.last_kernel() == "dconv3x3_kernel" and tuple(y.shape) == (n, cout, h, w) and y.dtype == tdt
        assert y.is_contiguous(memory_format=torch.channels_last) and torch.equal(y, y2), "two runs differ"
        _within(y, want, tdt, "dconv %d>%d d%d @%dx%d n%d %s %s" % (cin, cout, d, h, w, n, act, dtype))
        if mi == 3:  # negative controls, on the reference side only: the same output MISSES the bar against a wrong layer
            for what, kw in (("dilation d - 1", dict(dilation=d - 1)), ("dilation d + 1", dict(dilation=d + 1)),
                             ("taps transposed", dict(transpose=True))):
                figs, bar, ok = _figures(y, dilated_reference(x, pk, act=act, **kw), tdt)
                assert not ok and figs[0] > 10 * bar[0], (what, figs, bar)


def test_only_the_taps_inside_the_map_count():
    """d x (d + 1): no vertical neighbour is inside; the horizontal neighbours of the two edge columns are (x = 0 sees x = d and
    x = d sees x = 0).  With the centre tap's weights zeroed the middle columns are act(bias) exactly and the edge columns are not."""
    import torch
    from rfbaudit import dilated_reference
    from ssds.modeling.layers import fused_conv as FC

    d, cin, cout = 5, 40, 24
    pk = _layer(cin, cout, d, torch.bfloat16, seed=77, gain=3.0)
    pk.w[:, 1, 1, :] = 0
    pk._frag = None
    x = _input(2, cin, d, d + 1, torch.bfloat16, seed=78)
    y = FC.conv_native(x, pk).float()
    bias = pk.bias.view(1, -1, 1, 1).to(torch.bfloat16).float()
    assert torch.equal(y[:, :, :, 1:d], bias.expand(2, cout, d, d - 1))
    assert float((y[:, :, :, [0, d]] - bias).abs().mean()) > 0.1
    _within(y, dilated_reference(x, pk), torch.bfloat16, "edge columns")


@pytest.mark.parametrize("case", [(16, 16, 5, 2, 5, 6), (40, 24, 3, 3, 13, 13), (128, 128, 8, 2, 8, 9), (64, 136, 2, 2, 2, 3)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_guard_bands(dtype, case):
    """x, the weight image, scale, bias and y carved out of NaN-filled allocations: y is finite everywhere and fully written, the guards
    are intact, the inputs unchanged -- and the bits are those of ordinary allocations.  A lane that loaded outside the image, behind
    9 Cin or behind the last pixel and masked afterwards would have read a guard at the first or last pixels of x."""
    import torch
    from ssds.modeling.layers import fused_conv as FC

    tdt = getattr(torch, dtype)
    cin, cout, d, n, h, w = case
    pk = _layer(cin, cout, d, tdt, seed=cin + h, gain=_gain(h, w, d), act="relu")
    x = _input(n, cin, h, w, tdt, seed=h * w + d)
    clean = FC.conv_native(x, pk)
    gs = G.GuardSet("cuda")
    xg = gs.inp("x", x)
    for name, storage, view in G.guard_pack(pk):  # w, scale, bias (a 'dilated' pack has no frag() image: the kernel's is dfrag())
        gs.adopt(name, storage, view)
    pk._frag = None
    storage, view = G.guarded(pk.dfrag())
    pk._frag = ((pk.w.data_ptr(), pk.w._version), view)
    assert pk.dfrag().data_ptr() == view.data_ptr()
    gs.adopt("w_frag", storage, view)
    assert {name for name, _, _, _, _ in gs.items} == {"x", "w", "scale", "bias", "w_frag"}
    yg = gs.out("y", (n, cout, h, w), tdt, torch.channels_last)
    gs.arm()
    y = FC.conv_native(xg, pk, y=yg)
    torch.cuda.synchronize()
    assert y.data_ptr() == yg.data_ptr()
    assert gs.problems() == []
    assert not G.has_nan(yg) and bool(torch.isfinite(yg).all()) and G.same_bits(yg, clean)


def test_ssdk_conv_refuses_on_the_device_what_it_refuses_on_the_host():
    """A dilated pack with a residual, or as a head: SSDK_E_BADARG through the Python wrapper, nothing launched."""
    import torch
    from ssds import _native as N
    from ssds.modeling.layers import fused_conv as FC

    pk = _layer(16, 16, 3, torch.bfloat16, seed=3)
    x = _input(2, 16, 5, 5, torch.bfloat16, seed=4)
    with pytest.raises(N.SsdkError, match="dconv3x3"):
        FC.conv_native(x, pk, residual=x)
    with pytest.raises(N.SsdkError, match="dconv3x3"):
        FC.conv_native(x, pk, nchw_out=True)


# ---- the block -----------------------------------------------------------------------------------------------------------------------
def _seeded_block(cin, cout, stride, scale, visual, seed):
    import numpy as np
    import torch
    from ssds.modeling.layers.rfb_layers import BasicRFB

    blk = BasicRFB(cin, cout, stride=stride, scale=scale, visual=visual).eval()
    spec = [(k, tuple(v.shape)) for k, v in blk.state_dict().items()]
    state = cases_rfb.seeded_state(spec, seed)
    rs = np.random.RandomState(seed)
    for k in state:  # non-trivial BatchNorm statistics
        if k.endswith("running_mean"):
            state[k] = (rs.standard_normal(state[k].shape) * 0.1).astype(np.float32)
        elif k.endswith("running_var"):
            state[k] = rs.uniform(0.5, 1.0, state[k].shape).astype(np.float32)
    blk.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()})
    return blk


@pytest.mark.parametrize("cin,cout,stride,scale,visual,h,w", [(128, 128, 1, 1.0, 2, 7, 5), (256, 128, 2, 0.1, 2, 5, 3),
                                                             (128, 256, 2, 1.0, 1, 2, 1)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_block_op_by_op(dtype, cin, cout, stride, scale, visual, h, w, monkeypatch):
    """planner.record_rfb of one block, run as a plan: every op within its bar against fp32 on the op's actual input, the dilated ones
    included, and the block's output against the module in fp32 at the level of the ops it is made of."""
    import torch
    from rfbaudit import RfbAudit
    from ssds.modeling.layers import fused_conv as FC
    from ssds.modeling.layers import planner

    monkeypatch.delenv("SSDK_DCONV", raising=False)
    tdt = getattr(torch, dtype)
    blk = _seeded_block(cin, cout, stride, scale, visual, seed=cin + h).cuda()
    x = _input(2, cin, h, w, tdt, seed=cin * h + w)
    plan = FC.ConvPlan(x.device, tdt, x.shape)
    with torch.no_grad():
        out = planner.record_rfb(plan, plan.input_value(), blk, keep_input=True)
    plan.finalize()
    rows = RfbAudit(plan, [x]).run()
    print(planaudit.format_rows([dict(r, plan_kernel="") for r in rows]))
    assert len(rows) == 10 and [r["kernel"] for r in rows if r["dilated"]] == ["dconv3x3"] * 2
    assert [r["name"].split(" @")[0][-2:] for r in rows if r["dilated"]] == ["d%d" % (visual + 1), "d%d" % (2 * visual + 1)]
    assert not planaudit.failures(rows, tdt), planaudit.failures(rows, tdt)
    with torch.no_grad():
        plan.run(x)
        want = blk.float()(x.float())
    torch.cuda.synchronize()
    buf, n, c, ho, wo = out
    got = planaudit.PlanAudit.view(_View(plan, tdt), buf, n, c, ho, wo)
    assert tuple(want.shape) == (n, c, ho, wo) and 0.05 < float((want == 0).float().mean()) < 0.95
    med, p999, mx, _ = planaudit.stats(got, want)
    print("block %s: median / p99.9 / max = %.5f / %.5f / %.5f" % (dtype, med, p999, mx))
    # the longest path of the block is five rounded ops deep (1x1, 3x3, 3x3, dilated 3x3, ConvLinear): at most five times one op's bar
    # in each statistic (the errors add at worst linearly).  A wrong wire, a swapped branch or a lost ``scale`` is an error of the
    # size of the output itself: a maximum >= 1.
    bar = planaudit.BARS[tdt]["default"]
    assert med <= 5 * bar[0] and p999 <= 5 * bar[1] and mx <= 5 * bar[2], (med, p999, mx, bar)


class _View(object):
    """What planaudit.PlanAudit.view reads of its ``self``: the plan and its dtype."""

    def __init__(self, plan, dtype):
        self.plan, self.dtype = plan, dtype


# ---- the nets -----------------------------------------------------------------------------------------------------------------------
def _build(name, monkeypatch):
    monkeypatch.setattr(nethelp, "cases", cases_rfb)
    return nethelp.build(name)


class _Planned(object):
    """A case's model on the device with its recorded plan.  SSD on a stub backbone has no image plan (a stub has no planner), so its
    extras and heads are recorded on the backbone's maps (planner.build_ssd_plan(features=...)); the other cases are the model's own
    forward."""

    def __init__(self, name, tdt, monkeypatch):
        import torch
        from ssds.modeling.layers import fused_conv as FC
        from ssds.modeling.layers import planner

        self.FC, self.name, self.tdt = FC, name, tdt
        model, x, fx = _build(name, monkeypatch)
        self.model, self.x, self.fx = model.cuda().to(tdt), x, fx
        self.stub_ssd = name == "ssd_rfb_stub"
        xd = x.cuda().to(tdt)
        with torch.no_grad():
            if self.stub_ssd:
                self.plan = planner.build_ssd_plan(self.model, None, features=self.model.backbone(xd))
            else:
                self.model(xd)
                plans = self.model.__dict__.get("_plans") or self.model.__dict__.get("_neck_plans")
                found = [p for p in plans.values() if isinstance(p, FC.ConvPlan)]
                assert len(found) == 1, list(plans.values())
                self.plan = found[0]

    def inputs(self, xd):
        if self.stub_ssd or len(self.plan.inputs) > 1 or self.plan.inputs[0].shape[1] > 4:
            return list(self.model.backbone(xd))
        return [xd]

    def __call__(self, xd):
        import torch

        with torch.no_grad():
            if self.stub_ssd:
                return self.plan.run(*self.inputs(xd))
            runs = self.FC.STATS["plan_runs"]
            out = self.model(xd)
            assert self.FC.STATS["plan_runs"] == runs + 1, "the forward did not run as a recorded plan"
            return out


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(cases_rfb.NET_CASES))
def test_plan_matches_reference_module(name, dtype, monkeypatch):
    import torch
    from rfbaudit import RfbAudit
    from ssds.modeling.layers import fused_conv as FC
    from test_gpu_nets import POOL_DRAWS, SMALL, _check_against_floor, check_small_levels_pooled, floor_runs

    monkeypatch.delenv("SSDK_DCONV", raising=False)
    tdt = getattr(torch, dtype)
    p = _Planned(name, tdt, monkeypatch)
    model, x, fx, plan = p.model, p.x, p.fx, p.plan
    wl, wc = nethelp.want(fx)
    xd = x.cuda().to(tdt)
    loc, conf = p(xd)
    loc2, conf2 = p(xd)
    assert isinstance(plan, FC.ConvPlan)
    n_dilated = sum(1 for m in model.modules() if isinstance(m, torch.nn.Conv2d) and m.dilation != (1, 1))
    dilated = [L for L in plan.layers if L.get("kind") is None and L["pack"].kind == "dilated"]
    assert len(dilated) == n_dilated > 0 and len(plan.layer_table()) == len(plan.layers)
    for a, b in zip(loc + conf, loc2 + conf2):
        assert a.is_contiguous() and a.dtype == tdt and torch.equal(a, b), "replay is not deterministic"
    # the per-op audit: every op at its rounding level on the plan's own activations
    rows = RfbAudit(plan, p.inputs(xd)).run()
    print(planaudit.format_rows([dict(r, plan_kernel="") for r in rows]))
    assert len(rows) == len(plan.layers) and [r["kernel"] for r in rows if r["dilated"]] == ["dconv3x3"] * n_dilated
    assert not planaudit.failures(rows, tdt), planaudit.failures(rows, tdt)
    # SSDK_FUSED_CONV=0 gives the module path (floor_runs sets it): no plan, no HIP kernel of this library
    n0, p0 = FC.STATS["native_layers"], FC.STATS["plan_runs"]
    floor = floor_runs(model, xd)
    assert FC.STATS["native_layers"] == n0 and FC.STATS["plan_runs"] == p0
    report = _check_against_floor({"loc": loc, "conf": conf}, floor, {"loc": wl, "conf": wc}, name, dtype)
    print(name, dtype, "; ".join(report))
    # small levels: pooled over POOL_DRAWS more inputs, as tests/test_gpu_nets.py does it
    assert any(t.numel() < SMALL for t in wl + wc)
    cpu_model, _, _ = _build(name, monkeypatch)
    cpu = lambda t: t.float().cpu()
    plans_o, floors, wants = [{"loc": [cpu(t) for t in loc], "conf": [cpu(t) for t in conf]}], [
        {"loc": [cpu(t) for t in floor[0]["loc"]], "conf": [cpu(t) for t in floor[0]["conf"]]}], [{"loc": wl, "conf": wc}]
    g = torch.Generator().manual_seed(4711)
    stub = isinstance(cpu_model.backbone, nethelp.StubBackbone)
    for _ in range(POOL_DRAWS):
        xi = torch.rand(x.shape, generator=g)
        if stub:  # (a stub backbone ignores the image: draw its feature maps instead)
            feats = [torch.randn(f.shape, generator=g) * 0.7 for f in cpu_model.backbone.feats]
            cpu_model.backbone.feats = feats
            model.backbone.feats = feats
        with torch.no_grad():
            cl_, cc_ = cpu_model(xi)
        pl, pc = p(xi.cuda().to(tdt))
        fl = floor_runs(model, xi.cuda().to(tdt), runs=1)[0]
        wants.append({"loc": list(cl_), "conf": list(cc_)})
        plans_o.append({"loc": [cpu(t) for t in pl], "conf": [cpu(t) for t in pc]})
        floors.append({"loc": [cpu(t) for t in fl["loc"]], "conf": [cpu(t) for t in fl["conf"]]})
    assert check_small_levels_pooled(plans_o, floors, wants, name, dtype)


def test_graphed_inference_replays_eager_bit_for_bit(monkeypatch):
    from collections import OrderedDict

    import torch
    from ssds.modeling.layers import box
    from ssds.modeling.layers import fused_conv as FC
    from ssds.modeling.layers.decoder import Decoder
    from ssds.utils.graph import GraphedInference

    monkeypatch.delenv("SSDK_DCONV", raising=False)
    model, x, _ = _build("ssd_rfb_r18", monkeypatch)
    model = model.cuda().to(torch.float16)
    anchors = OrderedDict((s, box.generate_anchors(s, [1, 2, 0.5], [2.0, 2.828])) for s in (8, 16, 32, 53, 80))
    dec = Decoder(0.005, 0.6, 50, 100, True, True)
    x0 = x.cuda().to(torch.float16)
    g = GraphedInference(model, dec, anchors, x0)
    plan = model._plan(x0)
    assert isinstance(plan, FC.ConvPlan) and sum(L.get("kind") is None and L["pack"].kind == "dilated" for L in plan.layers) == 4
    torch.manual_seed(1)
    xi = torch.rand(x.shape, device="cuda").to(torch.float16)
    got = [t.clone() for t in g(xi)]
    with torch.no_grad():
        heads = model(xi)
        heads2 = model(xi)
        want = dec(*heads, anchors)
    for a, b in zip(heads[0] + heads[1], heads2[0] + heads2[1]):
        assert torch.equal(a, b), "two eager runs differ"
    for a, b in zip(got, want):
        assert torch.equal(a, b)


_CHILD = r'''
import os, sys
sys.path[:0] = [ROOT, os.path.join(ROOT, "ssds.pytorch_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")]
import torch
import cases_rfb, nethelp
nethelp.cases = cases_rfb
from ssds.modeling.layers import fused_conv as FC
model, x, fx = nethelp.build("ssd_rfb_r18")
model = model.cuda().to(torch.bfloat16)
xd = x.cuda().to(torch.bfloat16)
runs = FC.STATS["plan_runs"]
with torch.no_grad():
    loc, conf = model(xd)
torch.cuda.synchronize()
plan = model._plan(xd)
torch.save({"loc": [t.float().cpu() for t in loc], "conf": [t.float().cpu() for t in conf], "plan": plan if isinstance(plan, str) else
            [r["name"] for r in plan.layer_table()], "plan_runs": FC.STATS["plan_runs"] - runs}, OUT)
'''


def test_ssdk_dconv_switch_in_a_fresh_process(tmp_path, monkeypatch):
    """SSDK_DCONV=0 (docs/SWITCHES.md), as tests/test_gpu_switches.py runs a switch: the plan is the named string, the forward is the
    module path (backbone on PyTorch-ROCm, fused heads), and its outputs meet the same floor rule."""
    import torch
    from test_gpu_nets import _check_against_floor, floor_runs

    out = str(tmp_path / "off.pt")
    env = dict(os.environ)
    env["SSDK_DCONV"] = "0"
    code = "ROOT = %r\nOUT = %r\n" % (ROOT, out) + _CHILD
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    off = torch.load(out)
    assert isinstance(off["plan"], str) and "SSDK_DCONV=0" in off["plan"] and "PyTorch-ROCm" in off["plan"] and off["plan_runs"] == 0
    model, x, fx = _build("ssd_rfb_r18", monkeypatch)
    wl, wc = nethelp.want(fx)
    model = model.cuda().to(torch.bfloat16)
    floor = floor_runs(model, x.cuda().to(torch.bfloat16))
    dev = lambda ts: [t.cuda() for t in ts]
    _check_against_floor({"loc": dev(off["loc"]), "conf": dev(off["conf"])}, floor, {"loc": wl, "conf": wc}, "SSDK_DCONV=0", "bfloat16")


def test_ssd_detector_on_the_shipped_config():
    import numpy as np

    from ssds.modeling.layers import fused_conv as FC
    from ssds.ssds import SSDDetector

    det = SSDDetector(os.path.join(ROOT, "experiments", "cfgs", "ssd_resnet18_rfb_512.yml"))
    imgs = np.random.RandomState(0).randint(0, 256, (2, 512, 512, 3)).astype(np.uint8)
    runs = FC.STATS["plan_runs"]
    out = det(imgs)
    assert FC.STATS["plan_runs"] == runs + 1 and FC.STATS["torch_fallback_layers"] == 0
    assert len(out) == 3 and out[0].shape == (2, 100) and out[1].shape == (2, 100, 4) and out[2].shape == (2, 100)
    rows = [r["name"] for p in det.model.__dict__["_plans"].values() for r in p.layer_table()]
    assert [n for n in rows if " d" in n] == ["conv 128>128 k3 s1 d3 @8x8", "conv 128>128 k3 s1 d5 @8x8",
                                             "conv 128>128 k3 s1 d3 @4x4", "conv 128>128 k3 s1 d5 @4x4"]
