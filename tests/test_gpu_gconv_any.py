"""Grouped 3x3 convolutions of any supported group width on the GPU (csrc/ssdk_gconv_any.hip): single layers against the
fp32 CPU layer on the same rounded operands, the inertness of the K / row padding, whole image -> heads plans on backbones
of three width classes, and the two grouped configs at bench size."""
import os
import subprocess
import sys

import pytest

import guardband as G

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ref(x, conv, bn, act):
    """The fp32 layer on the CPU (the twin of tests/test_gpu_conv.py::_ref, restated here)."""
    import torch.nn.functional as F
    from ssds.modeling.layers.fused_conv import fold_bn

    w = conv.weight.detach().float().cpu()
    y = F.conv2d(x.float().cpu(), w, None, conv.stride, conv.padding, 1, conv.groups)
    scale, bias = fold_bn(conv, bn)
    y = y * scale.cpu().view(1, -1, 1, 1) + bias.cpu().view(1, -1, 1, 1)
    assert act == "relu"
    return y.clamp(min=0)


def _check(got, want, dtype, what, floor=0.125):
    """Per ELEMENT: |got - want| <= tol * max(|want|, floor * max|want|) + 1e-3, tol = 2^-7 (bf16) | 2^-9 (fp16): the
    project's bar for single layers (tests/test_gpu_conv.py::_check, restated here)."""
    import torch

    tol = 2.0 ** -7 if dtype == torch.bfloat16 else 2.0 ** -9
    g = got.float().cpu().contiguous()
    assert g.shape == want.shape, (what, g.shape, want.shape)
    scale = max(float(want.abs().max()), 1e-3)
    excess = (g - want).abs() - (tol * want.abs().clamp(min=floor * scale) + 1e-3)
    worst = int(excess.argmax())
    assert float(excess.max()) <= 0, "%s: element %d got %.6g want %.6g (scale %.3g)" % (
        what, worst, float(g.flatten()[worst]), float(want.flatten()[worst]), scale)


def _layer(gw, groups, stride, dtype, seed):
    import torch
    import torch.nn as nn

    c = gw * groups
    torch.manual_seed(seed)
    conv = nn.Conv2d(c, c, 3, stride, 1, groups=groups, bias=False)
    bn = nn.BatchNorm2d(c)
    bn.running_mean.normal_(0, 0.2)
    bn.running_var.uniform_(0.5, 1.5)
    bn.weight.data.uniform_(0.5, 1.5)
    bn.bias.data.normal_(0, 0.2)
    conv.weight.data = conv.weight.data.to(dtype).float()
    return conv, bn


# gw, groups, stride, h, w, n.  The channel run of a workgroup is floor(256 B / 2 gw) groups at stride 1, floor(128 B / 2 gw)
# at stride 2, at least one; width classes: S = one 16-row block (gw 4 -> 8, 8), M = two (24, 32), L = three and more.
LAYERS = [
    # class S
    (4, 32, 1, 20, 24, 2),    # ResNeXt50 layer1: 32 groups of 4, merged into 16 of 8 = one full run
    (4, 32, 2, 33, 31, 3),    # ragged map, n = 3; two runs of 8 merged groups
    (8, 19, 1, 33, 31, 3),    # ragged, n = 3, 19 groups = a run of 16 + a partial run of 3 (RegNetX002 stage 3)
    (8, 19, 2, 40, 24, 2),    # runs of 8 + 8 + 3
    (8, 46, 1, 7, 5, 2),      # 5 outputs wide: 8-wide fragments; 46 = 16 + 16 + 14
    (8, 46, 2, 8, 8, 1),      # 4 outputs wide: 4-wide fragments (RegNetX002 stage 4 at 128 px)
    # class M
    (24, 7, 1, 33, 31, 3),    # ragged, n = 3, a run of 5 + a partial run of 2
    (24, 17, 2, 28, 20, 2),   # runs of 2: eight full, one partial (RegNetX016 stage 3)
    (24, 38, 1, 7, 7, 2),     # 7 outputs wide
    (24, 10, 2, 9, 7, 1),     # 4 outputs wide
    (32, 32, 1, 20, 24, 2),   # ResNeXt50 layer4 / ResNeXt101 layer3
    (32, 5, 2, 33, 31, 3),    # ragged, runs of 2 + 2 + 1
    # class L
    (40, 6, 1, 33, 31, 3),    # three row blocks, the last half padding; ragged, n = 3
    (40, 14, 2, 14, 14, 1),   # 7 outputs wide, one group per run
    (48, 4, 1, 24, 20, 2),
    (48, 9, 2, 33, 31, 2),
    (56, 7, 1, 20, 24, 2),    # runs of 2: three full, one partial (RegNetX064 stage 2)
    (56, 3, 2, 28, 28, 3),
    (64, 5, 1, 16, 12, 2),    # runs of 2 + 2 + 1
    (64, 4, 2, 33, 31, 1),
    (112, 2, 1, 33, 31, 3),   # seven row blocks = two items per fragment pair, the second partial
    (112, 4, 2, 14, 14, 1),
    (120, 2, 1, 20, 24, 2),   # eight row blocks, the last half padding
    (120, 6, 2, 28, 20, 1),
    (120, 16, 1, 7, 5, 1),    # 5 outputs wide (RegNetX080 stage 4)
    (128, 2, 1, 16, 16, 2),   # one group = exactly the 256-byte run
    (128, 4, 2, 33, 31, 1),
    (168, 2, 1, 33, 31, 2),   # eleven row blocks, the last half padding, K = 1512 (48 k-steps); 61 KiB halo
    (168, 4, 2, 28, 28, 1),   # stride 2: the patch shrinks to two fragments to keep the halo under 64 KiB
    (168, 15, 1, 4, 4, 2),    # RegNetX320 stage 4 at 128 px: 4 x 4 map, 15 groups
    (256, 2, 1, 20, 24, 2),   # the widest supported: sixteen row blocks, K = 2304 (72 k-steps), patch of four fragments (56 KiB)
    (256, 3, 2, 33, 31, 2),   # stride 2: the only halo above 64 KiB (85 KiB with two fragments); ragged
    (256, 2, 2, 9, 7, 1),     # 4 outputs wide
]


@pytest.mark.parametrize("gw,groups,stride,h,w,n", LAYERS)
@pytest.mark.parametrize("dtype_name", ["bf16", "f16"])
def test_grouped_conv_any_width(gw, groups, stride, h, w, n, dtype_name):
    """The twin of test_grouped_conv_16_per_group for every other width of the registered backbones: 3x3, groups = C / gw
    (+ BN + ReLU) against the fp32 layer, per element."""
    import torch
    from ssds import _native as N
    from ssds.modeling.layers import fused_conv as FC

    dtype = torch.bfloat16 if dtype_name == "bf16" else torch.float16
    conv, bn = _layer(gw, groups, stride, dtype, gw * groups + stride)
    x = torch.randn(n, gw * groups, h, w).to(dtype)
    want = _ref(x, conv, bn, "relu")
    conv, bn = conv.cuda(), bn.cuda()
    pack = FC.ConvPack(conv, bn, "relu", dtype)
    assert pack.kind == "gany" and pack.groups == groups
    y = FC.conv_native(x.cuda(), pack)
    assert "gconv3x3_any" in N.last_kernel(), N.last_kernel()
    assert y.is_contiguous(memory_format=torch.channels_last)
    _check(y, want, dtype, "grouped conv gw=%d groups=%d s%d %dx%d" % (gw, groups, stride, h, w))
    assert torch.equal(y, FC.conv_native(x.cuda(), pack)), "no atomics, fixed k order: bit-reproducible"


def test_sixteen_wide_groups_stay_on_their_own_kernels():
    import torch
    from ssds import _native as N
    from ssds.modeling.layers import fused_conv as FC

    dtype = torch.bfloat16
    conv, bn = _layer(16, 8, 1, dtype, 5)
    x = torch.randn(2, 128, 20, 24).to(dtype)
    want = _ref(x, conv, bn, "relu")
    pack = FC.ConvPack(conv.cuda(), bn.cuda(), "relu", dtype)
    assert pack.kind == "g16"
    y = FC.conv_native(x.cuda(), pack)
    assert "gconv3x3_g16" in N.last_kernel(), N.last_kernel()
    _check(y, want, dtype, "grouped conv gw=16")


@pytest.mark.parametrize("gw,groups", [(24, 3), (16, 4)])
def test_grouped_conv_without_batchnorm(gw, groups):
    """A grouped Conv2d (with bias) + ReLU and no BatchNorm, as a FusedSequential could hold one: the grouped kernels have no
    scale-free form, so the pack passes a scale of ones instead of failing at launch."""
    import torch
    import torch.nn as nn
    from ssds import _native as N
    from ssds.modeling.layers import fused_conv as FC

    dtype = torch.bfloat16
    torch.manual_seed(gw)
    c = gw * groups
    conv = nn.Conv2d(c, c, 3, 1, 1, groups=groups, bias=True)
    conv.weight.data = conv.weight.data.to(dtype).float()
    x = torch.randn(2, c, 12, 10).to(dtype)
    want = _ref(x, conv, None, "relu")
    pack = FC.ConvPack(conv.cuda(), None, "relu", dtype)
    assert pack.scale is not None and bool((pack.scale == 1).all())
    y = FC.conv_native(x.cuda(), pack)
    assert ("gconv3x3_any" if gw != 16 else "gconv3x3_g16") in N.last_kernel(), N.last_kernel()
    _check(y, want, dtype, "grouped conv without BatchNorm")


def test_the_image_does_not_depend_on_the_wfrag_switch(monkeypatch):
    """SSDK_WFRAG=0 is an A/B of the dense kernels (FC.USE_WFRAG); the grouped image is the only weight tensor
    gconv3x3_any_kernel reads and is passed whatever the switch says."""
    import torch
    from ssds import _native as N
    from ssds.modeling.layers import fused_conv as FC

    dtype = torch.bfloat16
    conv, bn = _layer(24, 3, 1, dtype, 9)
    x = torch.randn(1, 72, 12, 12).to(dtype)
    want = _ref(x, conv, bn, "relu")
    pack = FC.ConvPack(conv.cuda(), bn.cuda(), "relu", dtype)
    monkeypatch.setattr(FC, "USE_WFRAG", False)
    y = FC.conv_native(x.cuda(), pack)
    assert "gconv3x3_any" in N.last_kernel()
    _check(y, want, dtype, "grouped conv without dense fragment images")
    d = FC.fill_desc(N.ConvDesc(), x.cuda().data_ptr(), 1, 12, 12, pack, N.dtype_code(x), "relu", y.data_ptr())
    d.w_frag = None
    rc = N.lib.ssdk_conv(__import__("ctypes").byref(d), None, 0, N.stream_ptr(y.device))
    assert rc != 0 and "w_frag" in N.lib.ssdk_last_error().decode()


@pytest.mark.parametrize("gw,groups,stride", [(24, 7, 1), (24, 7, 2), (168, 2, 1), (168, 2, 2)])
def test_padding_is_inert(gw, groups, stride):
    """x is a view into ONE larger allocation whose every other element is NaN -- a guard band before, neighbouring
    'images' between and after -- and a clean copy of the same values: results NaN-free and bit-identical.  A padded
    tap, a padded row or a halo pixel outside the image that multiplied live memory by a zero weight would show here."""
    import torch
    from ssds.modeling.layers import fused_conv as FC

    dtype = torch.bfloat16
    c, n, h, w = gw * groups, 2, 13, 11
    conv, bn = _layer(gw, groups, stride, dtype, 3)
    pack = FC.ConvPack(conv.cuda(), bn.cuda(), "relu", dtype)
    xs = torch.randn(n, h, w, c).to(dtype)  # NHWC values
    per = h * w * c
    # (tests/guardband.py: 4096 elements + one image of 0xFF bytes -- NaN -- on either side; [N,C,H,W] in channels_last memory)
    big, view = G.guarded(xs.cuda().permute(0, 3, 1, 2))
    assert view.is_contiguous(memory_format=torch.channels_last) and view.data_ptr() - big.data_ptr() >= 2 * (4096 + per)
    assert bool(torch.isnan(big.view(dtype)[:4096 + per]).all())
    y_view = FC.conv_native(view, pack)
    clean = xs.cuda().permute(0, 3, 1, 2)
    y_clean = FC.conv_native(clean, pack)
    assert not torch.isnan(y_view).any() and not torch.isnan(y_clean).any()
    assert torch.equal(y_view, y_clean)
    # one image alone, between NaN neighbours: the halo must not reach into the next image of the batch
    big2 = torch.full((3 * per,), float("nan"), dtype=dtype, device="cuda")
    big2[per:2 * per] = xs[0].reshape(-1).cuda()
    y_one = FC.conv_native(big2[per:2 * per].view(1, h, w, c).permute(0, 3, 1, 2), pack)
    assert torch.equal(y_one, y_clean[:1])
    _check(y_clean, _ref(xs.permute(0, 3, 1, 2), conv.cpu(), bn.cpu(), "relu"), dtype, "padding case")


def _rel_l2(outs, wants):
    return [float((g.float().cpu() - w).norm() / w.norm().clamp(min=1e-6)) for g, w in zip(outs, wants)]


@pytest.mark.parametrize("net,outs,depth", [("RegNetX002", [2, 3, 4], [56, 152, 368]), ("RegNetX006", [2, 3, 4], [96, 240, 528]),
                                            ("RegNetX040", [2, 3, 4], [240, 560, 1360]), ("RegNetX080", [2, 3, 4], [240, 720, 1920]),
                                            ("ResNeXt50_32x4d", [4, 5], [1024, 2048])])
def test_ssd_on_grouped_backbone_plan_matches_torch(net, outs, depth):
    """SSD heads on grouped backbones that cover the three width classes of the kernel -- RegNetX002 (gw 8: class S), RegNetX006
    (24: M), RegNetX040 (40: L, three row blocks), RegNetX080 (120: L, eight row blocks = two work items per fragment pair, and
    a dense 80 -> 80 3x3 in stage 1), ResNeXt50 (4, 8, 16, 32: S, M and the 16-wide kernels) --, built as
    test_ssd_on_resnet_plan_matches_torch builds its three: image -> heads is ONE recorded plan, nothing falls back to
    torch, the op list holds gconv3x3_any, eight replays are bit-identical, and the relative L2 error of every output
    against the fp32 CPU module is within max(0.06, 2 x floor), floor = the same quantity for PyTorch-ROCm executing the same
    bf16 module (2 x: the margin tests/planaudit.py leaves over its measured floors).

    Measured on an MI355X, relative L2 error per output, smallest .. largest over the outputs (the floor moves with
    MIOpen's choice of algorithms):
        RegNetX002       plan 0.0022 .. 0.0052   floor 0.0073 .. 0.0104
        RegNetX006       plan 0.0022 .. 0.0050   floor 0.0082 .. 0.0099
        RegNetX040       plan 0.0022 .. 0.0053   floor 0.0057 .. 0.0099
        RegNetX080       plan 0.0022 .. 0.0050   floor 0.0059 .. 0.0107
        ResNeXt50_32x4d  plan 0.0022 .. 0.0077   floor 0.0063 .. 0.0095
    so the bar that binds is 0.06, as for ResNet18 / 50 and RegNetX008."""
    import torch
    from ssds.modeling import nets, ssds
    from ssds.modeling.layers import fused_conv as FC

    torch.manual_seed(4)
    fl = [outs + ["Conv:S"], depth + [256]]
    nets_outputs, extras, hd = ssds.SSD.add_extras(fl, [6] * (len(outs) + 1), 5)
    model = ssds.SSD(getattr(nets, net)(outputs=nets_outputs), extras, hd, 5).eval()
    for m in model.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.normal_(0, 0.05)
            m.running_var.uniform_(0.9, 1.1)
    x = torch.rand(2, 3, 96, 128)
    with torch.no_grad():
        rl, rc = model(x)
    want = list(rl) + list(rc)
    model = model.cuda().to(torch.bfloat16)
    xd = x.cuda().to(torch.bfloat16)
    plans, fallback = FC.STATS["plan_runs"], FC.STATS["torch_fallback_layers"]
    with torch.no_grad():
        loc, conf = model(xd)
    assert FC.STATS["plan_runs"] == plans + 1, "the forward did not run as one plan"
    assert FC.STATS["torch_fallback_layers"] == fallback, "part of the network fell back to torch"
    plan = model._plan(xd)
    assert not isinstance(plan, str), plan
    plan.ctx.set_op_profiling(True)
    with torch.no_grad():
        model(xd)
    torch.cuda.synchronize()
    names = [k for k, _ in plan.ctx.op_timings()]
    plan.ctx.set_op_profiling(False)
    assert any("gconv3x3_any" in k for k in names), sorted(set(names))
    first = [t.clone() for t in tuple(loc) + tuple(conf)]
    for _ in range(8):
        with torch.no_grad():
            l2, c2 = model(xd)
        for a, b in zip(first, tuple(l2) + tuple(c2)):
            assert torch.equal(a, b), "replay is not deterministic"
    # the floor: PyTorch-ROCm executing the same bf16 module
    os.environ["SSDK_FUSED_CONV"] = "0"
    try:
        with torch.no_grad():
            tl, tc = model(xd)
    finally:
        del os.environ["SSDK_FUSED_CONV"]
    got, floor = _rel_l2(first, want), _rel_l2(list(tl) + list(tc), want)
    line = "%s plan %s floor %s" % (net, " ".join("%.4f" % v for v in got), " ".join("%.4f" % v for v in floor))
    print(line)
    for g, w in zip(first, want):
        assert g.shape == w.shape
    for e, fl_ in zip(got, floor):
        assert e <= max(0.06, 2.0 * fl_), line


def _seeded_model(cfg_name, seed=321):
    """create_model(cfg) with seeded weights, an untrained-looking score distribution and BatchNorm statistics calibrated
    on two random batches -> (fp32 CPU module in eval mode, cfg): tests/test_gpu_bench_sizes.py::_seeded_model, restated."""
    import torch
    import cases
    import nethelp
    from ssds.core import config
    from ssds.modeling import model_builder

    config.reset_cfg()
    cfg = config.cfg_from_file(os.path.join(ROOT, "experiments", "cfgs", cfg_name))
    torch.manual_seed(seed)
    model = model_builder.create_model(cfg.MODEL)
    spec = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
    state = cases.seeded_state(spec, seed)
    touched = nethelp.untrained_score_prior(state)
    assert touched == (2 * len(model.conf) if isinstance(model.conf, torch.nn.ModuleList) else 2), touched
    model.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()})
    for m in model.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.momentum = None
    model.train()
    g = torch.Generator().manual_seed(7)
    h, w = cfg.MODEL.IMAGE_SIZE
    with torch.no_grad():
        for _ in range(2):
            model(torch.rand((2, 3, h, w), generator=g))
    return model.eval(), cfg


@pytest.mark.parametrize("cfg_name,batch,dtype,expect", [
    ("fpn_resnext50_640.yml", 8, "bfloat16", ("stem7", "gconv3x3_any", "gconv3x3_g16", "conv3x3_halo")),
    ("bifpn_regnetx016_896.yml", 8, "float16", ("gconv3x3_any", "fuse", "conv3x3_halo")),
])
def test_grouped_configs_at_bench_size_against_the_fp32_module(cfg_name, batch, dtype, expect):
    """The two grouped configs at their image size, batch 8, by the procedure of
    test_forward_at_bench_size_against_the_fp32_module: the recorded plan (kernels asserted by name) against the fp32 CPU
    forward of the same module on 4 of the images, under the noise-floor-relative bar of tests/test_gpu_nets.py
    (PyTorch-ROCm executing the module in the same dtype, three executions).

    CPU cost of one case on 16 threads, by this test's own timer (printed): building the module and calibrating its
    BatchNorm statistics 1.7 s / 1.5 s, the fp32 forward of the 4 images 1.4 s (FPN-ResNeXt50@640) / 2.2 s
    (BiFPN-RegNetX016@896); a whole case took 10 - 15 s.  A job's timeout of 120 s per case is ample."""
    import time

    import torch
    from test_gpu_nets import _check_against_floor, floor_runs
    from ssds.modeling.layers import fused_conv as FC

    tdt = getattr(torch, dtype)
    t0 = time.time()
    cpu_model, cfg = _seeded_model(cfg_name)
    t1 = time.time()
    h, w = cfg.MODEL.IMAGE_SIZE
    g = torch.Generator().manual_seed(99)
    x = torch.rand((batch, 3, h, w), generator=g)
    pick = [0, batch // 3, (2 * batch) // 3, batch - 1]
    with torch.no_grad():
        wl, wc = cpu_model(x[pick])
    print("%s: model + calibration %.1f s, cpu forward of 4 images %.1f s" % (cfg_name, t1 - t0, time.time() - t1))
    model = cpu_model.cuda().to(tdt)
    xd = x.cuda().to(tdt)
    runs, fallback = FC.STATS["plan_runs"], FC.STATS["torch_fallback_layers"]
    with torch.no_grad():
        loc, conf = model(xd)
    torch.cuda.synchronize()
    assert FC.STATS["plan_runs"] == runs + 1, "the forward did not run as one recorded plan"
    assert FC.STATS["torch_fallback_layers"] == fallback, "part of the network fell back to torch"
    plan = model._plan(xd) if hasattr(model, "_plan") else next(iter(model._neck_plans.values()))
    assert not isinstance(plan, str), plan
    plan.ctx.set_op_profiling(True)
    with torch.no_grad():
        loc2, conf2 = model(xd)
    torch.cuda.synchronize()
    names = [k for k, _ in plan.ctx.op_timings()]
    plan.ctx.set_op_profiling(False)
    for kern in expect:
        assert any(kern in n for n in names), "%s was not selected at this size: %s" % (kern, sorted(set(names)))
    for a, b in zip(tuple(loc) + tuple(conf), tuple(loc2) + tuple(conf2)):
        assert torch.equal(a, b), "replay is not deterministic"
    floor = floor_runs(model, xd[pick])
    got = {"loc": [t[pick] for t in loc], "conf": [t[pick] for t in conf]}
    for i, c in enumerate(wc):
        p = c.float().clamp(1e-7, 1.0 - 1e-7)
        assert float((torch.log(p) - torch.log1p(-p)).std()) > 0.3, "conf level %d of the fp32 reference is dead" % i
    _check_against_floor(got, floor, {"loc": wl, "conf": wc}, "bench size %s B=%d" % (cfg_name, batch), dtype, tail_factor=3.0)


SWITCH_CHILD = r'''
import os, sys
sys.path[:0] = [ROOT, os.path.join(ROOT, "ssds.pytorch_amd")]
import torch
from ssds.modeling import nets, ssds
from ssds.modeling.layers import fused_conv as FC
assert FC.conv_kind(torch.nn.Conv2d(72, 72, 3, 1, 1, groups=3)) is None
assert FC.conv_kind(torch.nn.Conv2d(64, 64, 3, 1, 1, groups=4)) == "g16"
torch.manual_seed(4)
nets_outputs, extras, hd = ssds.SSD.add_extras([[2, 3, 4, "Conv:S"], [56, 152, 368, 256]], [6] * 4, 5)
model = ssds.SSD(nets.RegNetX002(outputs=nets_outputs), extras, hd, 5).eval().cuda().to(torch.bfloat16)
x = torch.rand(2, 3, 96, 128).cuda().to(torch.bfloat16)
plans = FC.STATS["plan_runs"]
with torch.no_grad():
    loc, conf = model(x)
torch.cuda.synchronize()
plan = model._plan(x)
assert isinstance(plan, str) and "not covered" in plan, plan  # (the planner's PlanUnsupported message)
assert FC.STATS["plan_runs"] == plans, "the image -> heads plan ran although its grouped layers are switched off"
assert all(bool(torch.isfinite(t.float()).all()) for t in tuple(loc) + tuple(conf))
print("SWITCH_OK")
'''


def test_switch_puts_the_backbone_back_on_torch():
    """SSDK_GCONV_ANY=0 (docs/SWITCHES.md; read once per process, hence the subprocess): the widths other than 16 are
    'not covered' again, no image -> heads plan is recorded for SSD on RegNetX002 (the planner's message is kept in its
    place) and the backbone runs on PyTorch-ROCm; 16 is untouched."""
    e = dict(os.environ)
    e["SSDK_GCONV_ANY"] = "0"
    r = subprocess.run([sys.executable, "-c", "ROOT = %r\n" % ROOT + SWITCH_CHILD], env=e, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "SWITCH_OK" in r.stdout, (r.stdout[-1500:], r.stderr[-1500:])
