"""EfficientNet backbones and the MBConv tail op (``ssdk_mbse``), the parts that need no GPU: names, shapes and the reference's
``state_dict`` schema, the fp32 module against the reference's outputs (tests/golden/net_*eff*.npz), ``MbSePack`` against the
module in fp64, the judge of tests/mbseaudit.py on an fp32 model of the kernels and on four planted defects, the C-ABI, the
planner's walk and the training Solver's routing."""
import ctypes
import os
import subprocess

import pytest
import torch

import cases_effnet
import mbseaudit
import nethelp
from solverhelp import run_solver_script

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["EfficientNetB%d" % i for i in range(6)]


# ---- 1. names and shapes -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_every_variant_builds_through_the_registry(name):
    from ssds.modeling import nets

    assert name in nets.efficientnet.__all__ and hasattr(nets, name)
    with torch.device("meta"):
        net = getattr(nets, name)(outputs=[3, 5, 7], num_images=1)
    assert not any(k.startswith(("head_conv.", "classifier.")) for k in net.state_dict())
    assert "conv1.0.weight" in net.state_dict() and "stage3.1.conv.2.se.1.weight" in net.state_dict()
    assert "stage1.0.conv.1.se.1.weight" in net.state_dict()  # the expand-free first block: indices one lower
    assert net.initialize() is None


@pytest.mark.parametrize("name,widths", [("EfficientNetB0", (40, 112, 320)), ("EfficientNetB2", (48, 120, 352))])
def test_output_levels(name, widths):
    from ssds.modeling import nets

    net = getattr(nets, name)(outputs=[3, 5, 7]).eval()
    with torch.no_grad():
        maps = net(torch.rand(1, 3, 64, 96))
    assert [tuple(m.shape) for m in maps] == [(1, widths[0], 8, 12), (1, widths[1], 4, 6), (1, widths[2], 2, 3)]


def test_create_model_with_the_shipped_config():
    from ssds.core import config
    from ssds.modeling import model_builder
    from ssds.modeling.nets.efficientnet import EfficientEx

    cfg = config.cfg_from_file(os.path.join(ROOT, "experiments", "cfgs", "bifpn_efficientnetb0_512.yml"))
    model = model_builder.create_model(cfg.MODEL)
    assert isinstance(model.backbone, EfficientEx) and model.backbone.outputs == [3, 5, 7]


def test_drop_connect_is_per_sample_in_training_and_the_identity_in_eval():
    blk = mbseaudit.make_block(16, 16, 6, 3, 1, seed=3)
    x = torch.randn(64, 16, 5, 5)
    with torch.no_grad():
        assert torch.equal(blk._drop_connect(x), x)
        blk.train()
        torch.manual_seed(0)
        y = blk._drop_connect(x)
    kept = (y.flatten(1).abs().sum(1) > 0)
    assert 0 < int(kept.sum()) < 64  # rate 0.2: some samples dropped whole, the others scaled by 1 / 0.8
    torch.testing.assert_close(y[kept], x[kept] / 0.8)
    assert float(y[~kept].abs().max()) == 0.0


# ---- 2. golden cases -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cases_effnet.NET_CASES))
def test_module_matches_reference_fp32(name):
    model, x, fx = mbseaudit.build_case(name)  # (asserts the schema: equal keys and shapes, only the UNUSED_TAILS missing)
    nt = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        with torch.no_grad():
            loc, conf = model(x)
    finally:
        torch.set_num_threads(nt)
    wl, wc = nethelp.want(fx)
    assert len(loc) == len(wl) and len(conf) == len(wc)
    for i, (l, a, c, b) in enumerate(zip(loc, wl, conf, wc)):  # the check of tests/test_nets_golden.py
        assert l.shape == a.shape and c.shape == b.shape, (name, i)
        torch.testing.assert_close(l, a, rtol=1e-3, atol=5e-4 * float(a.abs().max()))
        torch.testing.assert_close(c, b, rtol=1e-3, atol=2e-4)


# ---- 3. the pack ---------------------------------------------------------------------------------------------------------------
# every (k, stride, expand, residual) combination of EfficientNet-B0's blocks: (cin, cout, expand, k, stride)
B0_BLOCKS = [(32, 16, 1, 3, 1), (16, 24, 6, 3, 2), (24, 24, 6, 3, 1), (24, 40, 6, 5, 2), (40, 40, 6, 5, 1), (80, 112, 6, 5, 1),
             (192, 320, 6, 3, 1)]


def test_the_block_table_names_every_combination_of_b0():
    from ssds.modeling import nets
    from ssds.modeling.nets.efficientnet import MBConvBlock

    with torch.device("meta"):
        net = nets.EfficientNetB0(outputs=[7])
    seen = set()
    for m in net.modules():
        if isinstance(m, MBConvBlock):
            _, dw, _, _, _ = m.parts()
            seen.add((dw[0].kernel_size[0], dw[0].stride[0], m.parts()[0] is not None, m.use_residual))
    assert seen == {(k, s, e != 1, ci == co and s == 1) for ci, co, e, k, s in B0_BLOCKS}


@pytest.mark.parametrize("cin,cout,expand,k,stride", B0_BLOCKS)
def test_pack_and_three_stage_reference_equal_the_module_in_fp64(cin, cout, expand, k, stride):
    from ssds.modeling.layers.fused_conv import MbSePack

    blk = mbseaudit.make_block(cin, cout, expand, k, stride, seed=cin + k).double()
    assert MbSePack.supported(blk)
    pk = MbSePack(blk, torch.float64)
    assert (pk.cin, pk.cout, pk.k, pk.stride, pk.residual) == (cin * expand, cout, k, stride, cin == cout and stride == 1)
    x = torch.randn(2, cin, 9, 7, dtype=torch.float64)
    with torch.no_grad():
        want = blk(x)
        mid = blk.parts()[0](x) if blk.parts()[0] is not None else x
        got = mbseaudit.reference(pk, mid, x if blk.use_residual else None)["y"]
    torch.testing.assert_close(got, want, rtol=1e-9, atol=1e-9 * float(want.abs().max()))


def test_pack_rejects_what_the_kernels_do_not_take():
    from ssds.modeling.layers.fused_conv import MbSePack
    from ssds.modeling.nets.mobilenet import InvertedResidual

    assert not MbSePack.supported(mbseaudit.make_block(4, 8, 3, 3, 1, seed=1))   # C = 12: no multiple of 8
    assert not MbSePack.supported(mbseaudit.make_block(8, 12, 1, 3, 1, seed=1))  # Cout = 12
    assert not MbSePack.supported(InvertedResidual(16, 16, 1, 6))
    blk = mbseaudit.make_block(8, 8, 1, 5, 1, seed=1)
    blk.parts()[1][0].padding = (1, 1)
    assert not MbSePack.supported(blk)


# ---- 4. the judge --------------------------------------------------------------------------------------------------------------
def _judge_case(dtype, k=5):
    from ssds.modeling.layers.fused_conv import MbSePack

    blk = mbseaudit.make_block(40, 40, 6, k, 1, seed=11)  # C = 240 (K tail 16), residual, 7 x 7 maps: 49 pixels per image
    pk = MbSePack(blk, dtype)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(3, 240, 7, 7, generator=g).to(dtype)
    res = torch.randn(3, 40, 7, 7, generator=g).to(dtype)
    return pk, x, res


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("reround", [True, False])
def test_an_fp32_model_of_the_kernels_passes_the_bars(dtype, reround):
    pk, x, res = _judge_case(dtype)
    lines = []
    bad = mbseaudit.judge(pk, x, res, mbseaudit.cpu_model(pk, x, res, dtype, reround=reround), dtype, lines=lines)
    print("\n".join(lines))
    assert not bad, bad


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("mutation,stage", [("pool", "pool"), ("gate", "y"), ("ktail", "y"), ("shift", "t")])
def test_the_bars_catch_planted_defects(dtype, mutation, stage):
    pk, x, res = _judge_case(dtype)
    bad = mbseaudit.judge(pk, x, res, mbseaudit.cpu_model(pk, x, res, dtype, mutate=mutation), dtype)
    assert any(b.startswith(stage + " ") for b in bad), (mutation, bad)


# ---- 5. the C-ABI --------------------------------------------------------------------------------------------------------------
def test_abi_sizes_and_version():
    from ssds import _native as N

    assert N.lib.ssdk_version() == 245 and N.ABI_VERSION == 245
    assert ctypes.sizeof(N.MbSeDesc) == N.lib.ssdk_mbse_desc_bytes()
    assert N.lib.ssdk_struct_size(7) == ctypes.sizeof(N.Op) and N.lib.ssdk_struct_size(8) == 0
    assert N.OP_MBSE == 6 and N.Op._fields_[-1][0] == "mbse"
    header = open(os.path.join(ROOT, "include", "ssdk.h")).read()
    for name in ("ssdk_mbse", "ssdk_mbse_pool_tiles", "ssdk_mbse_desc_bytes"):
        assert name in N.EXPORTS and (name + "(") in header and hasattr(N.lib, name), name
    assert "SSDK_OP_MBSE = 6" in header


def test_struct_sizes_as_gcc_sees_the_header(tmp_path):
    from ssds import _native as N

    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include "ssdk.h"\nint main(void) { printf("%zu %zu %d\\n", sizeof(ssdk_mbse_desc), '
                   'sizeof(ssdk_op), (int)SSDK_OP_MBSE); return 0; }\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert [int(v) for v in out] == [ctypes.sizeof(N.MbSeDesc), ctypes.sizeof(N.Op), N.OP_MBSE]


def test_pool_tiles_mirror():
    from ssds import _native as N
    from ssds.modeling.layers import fused_conv as FC

    for h, w, k, s in [(1, 1, 3, 1), (16, 16, 3, 1), (17, 16, 5, 1), (33, 31, 5, 2), (67, 35, 3, 2), (256, 256, 3, 1)]:
        assert N.lib.ssdk_mbse_pool_tiles(h, w, k, s) == FC.mbse_pool_tiles(h, w, k, s) > 0
    assert N.lib.ssdk_mbse_pool_tiles(8, 8, 4, 1) == 0 and N.lib.ssdk_mbse_pool_tiles(8, 8, 3, 3) == 0


def test_bad_arguments_are_refused_before_any_launch():
    from ssds import _native as N

    F = 0x1000  # never dereferenced: every call below fails validation first

    def call(**kw):
        d = N.MbSeDesc()
        for name in ("x", "t", "pool_partial", "gate", "y", "w_dw", "scale_dw", "bias_dw", "w_se1", "b_se1", "w_se2", "b_se2",
                     "w_proj", "scale_proj", "bias_proj"):
            setattr(d, name, F)
        d.N, d.H, d.W, d.C, d.R, d.Cout, d.k, d.stride, d.dtype, d.stages = 2, 8, 8, 16, 4, 16, 3, 1, N.BF16, 0
        for k, v in kw.items():
            setattr(d, k, v)
        rc = N.lib.ssdk_mbse(ctypes.byref(d), None)
        return rc, N.lib.ssdk_last_error().decode()

    for kw in (dict(C=12), dict(k=4), dict(stride=3), dict(R=0), dict(gate=None), dict(Cout=12), dict(dtype=N.F32), dict(H=0),
               dict(stages=8), dict(x=F + 2)):
        rc, msg = call(**kw)
        assert rc == -1 and msg.startswith("mbse:"), (kw, rc, msg)
    assert N.lib.ssdk_mbse(None, None) == -1


# ---- 6. the planner ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cases_effnet.NET_CASES))
def test_planner_records_one_mbse_op_per_block(name, monkeypatch):
    from ssds.modeling.layers import planner
    from ssds.modeling.layers.fused_conv import ConvPlan
    from ssds.modeling.nets.efficientnet import MBConvBlock

    monkeypatch.delenv("SSDK_MBSE", raising=False)
    model, x, _ = mbseaudit.build_case(name)
    model = model.to(torch.bfloat16)
    plan = ConvPlan(x.device, torch.bfloat16, x.shape)
    feats = planner.record_backbone(plan, plan.input_value(), model.backbone)
    net = model.backbone
    blocks = [b for j in range(1, max(net.outputs) + 1) for b in getattr(net, "stage%d" % j)]
    assert all(isinstance(b, MBConvBlock) for b in blocks)
    kinds = [L.get("kind") for L in plan.layers]
    assert kinds[0] is None and plan.layers[0]["pack"].kind == "stem" and plan.layers[0]["act"] == "silu"
    want = []
    for b in blocks:
        want += ([None] if b.parts()[0] is not None else []) + ["mbse"]
    assert kinds[1:] == want
    i = 1
    for b in blocks:
        if b.parts()[0] is not None:
            assert plan.layers[i]["pack"].k == 1 and plan.layers[i]["act"] == "silu"
            i += 1
        L = plan.layers[i]
        assert (L["res"] is not None) == b.use_residual and L["pack"].k == b.parts()[1][0].kernel_size[0]
        i += 1
    strides = {3: 8, 5: 16, 7: 32}
    assert [(f[3], f[4]) for f in feats] == [(x.shape[2] // strides[l], x.shape[3] // strides[l]) for l in net.outputs]
    rows = [r for r in plan.layer_table() if r["kind"] == "mbconv"]
    assert len(rows) == len(blocks) and all(r["name"].startswith("mbse ") and r["flops"] > 0 and r["bytes"] > 0 for r in rows)
    # the whole detector records and finalizes too (descriptors filled; nothing is launched)
    full = {"SSD": planner.build_ssd_plan}.get(type(model).__name__)
    full_plan = full(model, x.to(torch.bfloat16)) if full else model._build_neck_plan(None, image=x.to(torch.bfloat16))
    ops = [op for op in full_plan.ops if op.kind == 6]
    assert len(ops) == len(blocks) and all(op.lane == 0 and op.mbse.t and op.mbse.gate and op.mbse.pool_partial and op.mbse.y
                                           for op in ops)


def test_the_switch_sends_the_backbone_to_torch(monkeypatch):
    from ssds.modeling import nets
    from ssds.modeling.layers import planner
    from ssds.modeling.layers.fused_conv import ConvPlan

    net = nets.EfficientNetB0(outputs=[3]).eval().to(torch.bfloat16)
    monkeypatch.setenv("SSDK_MBSE", "0")
    plan = ConvPlan(torch.device("cpu"), torch.bfloat16, (1, 3, 64, 64))
    with pytest.raises(planner.PlanUnsupported):
        planner.record_backbone(plan, plan.input_value(), net)
    monkeypatch.setenv("SSDK_MBSE", "1")
    plan = ConvPlan(torch.device("cpu"), torch.bfloat16, (1, 3, 64, 64))
    assert len(planner.record_backbone(plan, plan.input_value(), net)) == 1


def test_wider_stems_are_reported_not_planned():
    """B3 ... B5 have 40- / 48-channel stems, which the image-stem kernel (16 / 32 / 64) does not take: PlanUnsupported."""
    from ssds.modeling import nets
    from ssds.modeling.layers import planner
    from ssds.modeling.layers.fused_conv import ConvPlan

    net = nets.EfficientNetB3(outputs=[3]).eval().to(torch.bfloat16)
    plan = ConvPlan(torch.device("cpu"), torch.bfloat16, (1, 3, 64, 64))
    with pytest.raises(planner.PlanUnsupported):
        planner.record_backbone(plan, plan.input_value(), net)


# ---- 7. the training Solver ----------------------------------------------------------------------------------------------------
_SOLVER = r"""
from ssds.core import config
from ssds.utils import train_ddp
import torch.nn as nn
cfg = config.cfg_from_file(%(cfg)r)
s = train_ddp.Solver(cfg, 0, torch.device("cpu"))
from ssds.modeling.nets.efficientnet import PlainConv2d, SqueezeExcitation
dw5 = [m for m in s.model.modules() if isinstance(m, nn.Conv2d) and m.kernel_size == (5, 5)]
se = [m for q in s.model.modules() if isinstance(q, SqueezeExcitation) for m in q.modules() if isinstance(m, nn.Conv2d)]
print("RESULT", len(dw5), sum(type(m) is PlainConv2d for m in dw5), len(se), sum(type(m) is PlainConv2d for m in se))
"""


def test_solver_builds_and_leaves_the_new_layer_types_to_torch():
    n5, plain5, nse, plainse = run_solver_script(_SOLVER, "bifpn_efficientnetb0_512.yml")
    assert n5 == plain5 == 9 and nse == plainse == 32  # B0: 2 + 3 + 4 blocks with 5x5 windows; 16 blocks x 2 SE convolutions
