"""The DenseNet dense-block training step (csrc/ssdk_densetrain.hip, include/ssdk_densetrain.h, ssds/modeling/layers/densetrain.py),
the parts that need no GPU: the header and its bound entry points, their argument checks (all made before any device call), which
blocks ``use_native_dense_block`` switches, that a switched model computes bit for bit what the module does on the CPU, what
``supported`` refuses, the Solver's routing, and the summation-depth twins against the library's workspace queries."""
import copy
import os

import pytest

import densejudge as DJ
from solverhelp import run_solver_script

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ssdk_dense_train_place_workspace_bytes", "ssdk_dense_train_place", "ssdk_dense_train_pw_forward", "ssdk_dense_train_pw_wgrad",
       "ssdk_dense_train_bn1_workspace_bytes", "ssdk_dense_train_bn1_reduce", "ssdk_dense_train_bn1_apply")


def test_header_parses_and_every_symbol_is_bound():
    from ssds import _native as N

    with open(os.path.join(ROOT, "include", "ssdk_densetrain.h")) as f:
        h = N.parse_header(f.read())
    assert tuple(h.functions) == NEW == N.DENSETRAIN_EXPORTS and not h.structs and not h.constants
    assert N.DENSETRAIN_HEADER_PATH.endswith("ssdk_densetrain.h")
    for name in NEW:
        fn = getattr(N.lib, name)
        assert (fn.restype, list(fn.argtypes)) == (h.functions[name][0], h.functions[name][1]), name
        assert name not in N.EXPORTS
    assert len(N.EXPORTS) == 127 and N.lib.ssdk_version() == 245 and N.ABI_VERSION == 245


def test_bad_arguments_are_refused_before_any_launch():
    from ssds import _native as N

    L = N.lib
    F = 0x1000  # never dereferenced: every call below fails validation first
    err = lambda: L.ssdk_last_error().decode()  # noqa: E731
    BAD, WORKSPACE = -1, -2
    assert (N._K["SSDK_E_BADARG"], N._K["SSDK_E_WORKSPACE"]) == (BAD, WORKSPACE)
    big = 1 << 40

    def place(t=F, y=F, ys=96 * 63, sums=F, ws=F, wsb=big, n=2, c=64, hw=63, dt=N.BF16):
        return L.ssdk_dense_train_place(t, y, ys, sums, ws, wsb, n, c, hw, dt, None)

    for kw in (dict(t=None), dict(y=None), dict(sums=None), dict(ws=None), dict(t=F + 1), dict(y=F + 1), dict(sums=F + 2), dict(ws=F + 8),
               dict(n=0), dict(c=0), dict(hw=0), dict(ys=64 * 63 - 1), dict(ys=0), dict(dt=N.F32), dict(dt=7), dict(ys=1 << 32),
               dict(n=1 << 16, ys=1 << 16)):
        assert place(**kw) == BAD and "dense_train_place" in err(), (kw, err())
    need = L.ssdk_dense_train_place_workspace_bytes(2, 64, 63)
    assert need > 0 and L.ssdk_dense_train_place_workspace_bytes(0, 64, 63) == 0 and L.ssdk_dense_train_place_workspace_bytes(2, 0, 63) == 0
    assert place(wsb=need - 1) == WORKSPACE and "workspace" in err()

    def fwd(x=F, xs=96 * 63, coef=F, a=F, lda=64, m=F, sums=None, ws=None, wsb=0, b=2, k=64, cm=128, hw=63, dt=N.BF16):
        return L.ssdk_dense_train_pw_forward(x, xs, coef, a, lda, m, sums, ws, wsb, b, k, cm, hw, dt, None)

    for kw in (dict(x=None), dict(coef=None), dict(a=None), dict(m=None), dict(x=F + 1), dict(m=F + 1), dict(a=F + 8), dict(coef=F + 4),
               dict(k=7), dict(cm=7), dict(k=0), dict(b=0), dict(hw=0), dict(lda=56), dict(lda=68), dict(xs=64 * 63 - 1), dict(xs=0),
               dict(dt=N.F32), dict(dt=5), dict(xs=1 << 32), dict(b=1 << 16, xs=1 << 16), dict(sums=F), dict(sums=F, ws=F + 4, wsb=big)):
        assert fwd(**kw) == BAD and "dense_train_pw_forward" in err(), (kw, err())
    need = L.ssdk_pws_stats_workspace_bytes(2, 64, 128, 63)
    assert need > 0 and fwd(sums=F, ws=F, wsb=need - 1) == WORKSPACE and "workspace" in err()

    def wg(dm=F, x=F, xs=96 * 63, coef=F, dw=F, ws=F, wsb=big, b=2, cm=128, k=64, hw=63, dt=N.BF16):
        return L.ssdk_dense_train_pw_wgrad(dm, x, xs, coef, dw, ws, wsb, b, cm, k, hw, dt, None)

    for kw in (dict(dm=None), dict(x=None), dict(coef=None), dict(dw=None), dict(ws=None), dict(x=F + 1), dict(dm=F + 1), dict(coef=F + 8),
               dict(b=0), dict(cm=7), dict(k=7), dict(hw=0), dict(xs=64 * 63 - 1), dict(dt=N.F32), dict(dt=4), dict(xs=1 << 32),
               dict(b=1 << 16, xs=1 << 16)):
        assert wg(**kw) == BAD and "dense_train_pw_wgrad" in err(), (kw, err())
    need = L.ssdk_pws_wgrad_workspace_bytes(2, 128, 64, 63)
    assert need > 0 and wg(wsb=need - 1) == WORKSPACE and "workspace" in err()

    def red(s=F, x=F, xs=96 * 63, coef=F, mean=F, invstd=F, out=F, ws=F, wsb=big, n=2, k=64, hw=63, dt=N.BF16):
        return L.ssdk_dense_train_bn1_reduce(s, x, xs, coef, mean, invstd, out, ws, wsb, n, k, hw, dt, None)

    for kw in (dict(s=None), dict(x=None), dict(coef=None), dict(mean=None), dict(invstd=None), dict(out=None), dict(ws=None), dict(s=F + 1),
               dict(x=F + 1), dict(ws=F + 8), dict(n=0), dict(k=0), dict(hw=0), dict(xs=64 * 63 - 1), dict(dt=N.F32), dict(dt=9),
               dict(xs=1 << 32), dict(n=1 << 16, xs=1 << 16)):
        assert red(**kw) == BAD and "dense_train_bn1_reduce" in err(), (kw, err())
    need = L.ssdk_dense_train_bn1_workspace_bytes(2, 64, 63)
    assert need > 0 and L.ssdk_dense_train_bn1_workspace_bytes(2, 64, 0) == 0
    assert red(wsb=need - 1) == WORKSPACE and "workspace" in err()

    def app(s=F, x=F, xs=96 * 63, coef=F, mean=F, invstd=F, weight=F, r=F, g=F, gs=96 * 63, n=2, k=64, hw=63, dt=N.BF16):
        return L.ssdk_dense_train_bn1_apply(s, x, xs, coef, mean, invstd, weight, r, g, gs, n, k, hw, dt, None)

    for kw in (dict(s=None), dict(x=None), dict(coef=None), dict(mean=None), dict(invstd=None), dict(weight=None), dict(r=None), dict(g=None),
               dict(g=F + 1), dict(x=F + 1), dict(n=0), dict(k=0), dict(hw=0), dict(xs=64 * 63 - 1), dict(gs=64 * 63 - 1), dict(gs=0),
               dict(dt=N.F32), dict(dt=3), dict(gs=1 << 32), dict(n=1 << 16, gs=1 << 16)):
        assert app(**kw) == BAD and "dense_train_bn1_apply" in err(), (kw, err())


def test_depth_twins_restate_the_library():
    """reduce_split is dense_split of csrc/ssdk_densetrain.hip (held against both workspace queries), the GEMM entries keep the plans
    of ssdk_pws_forward / ssdk_pws_wgrad (their workspace rules), and the depth functions are what their derivations say."""
    from ssds import _native as N
    from ssds.modeling.layers import densetrain as DT
    from ssds.modeling.layers import shuffletrain as ST

    L = N.lib
    for n, c, hw in ((2, 64, 63), (3, 128, 169), (2, 32, 25), (1, 256, 128), (32, 32, 1600), (32, 1024, 400), (64, 8, 25600), (5, 3000, 9),
                     (200, 16, 4)):
        s = DT.reduce_split(n, c)
        assert 1 <= s <= min(n, 64)
        assert L.ssdk_dense_train_place_workspace_bytes(n, c, hw) == c * s * 2 * 4 == L.ssdk_dense_train_bn1_workspace_bytes(n, c, hw)
        items = -(-n // s) * -(-hw // 8)
        assert DT.place_sum_depth(n, c, hw) == DT.bn1_sum_depth(n, c, hw) == 8 * -(-items // 256) + 6 + 3 + (s - 1) + 1
    assert DT.reduce_split(2, 64) == 2 and DT.reduce_split(32, 32) == 32 and DT.reduce_split(200, 16) == 64 and DT.reduce_split(4, 4096) == 1
    assert DT.place_sum_depth(2, 64, 63) == 8 + 9 + 1 + 1
    for case in DJ.CASES:
        b, _, k, m, h, w = case
        tiled, splits, cps = ST.wgrad_plan(b, m, k, h * w)
        assert (splits + (splits + 63) // 64) * m * k * 4 == L.ssdk_pws_wgrad_workspace_bytes(b, m, k, h * w)
        assert DT.pw_wgrad_sum_depth(b, m, k, h * w) == ST.wgrad_sum_depth(cps) == 32 + 4 * cps + 36
        assert DT.pw_gemm_sum_depth(k) == 32 + (k + 31) // 32 and DT.pw_stats_sum_depth(1) == ST.stats_sum_depth(1)


def test_exact_operands_cover_the_zero_pre_activation():
    """The operands of the GPU kernel tests, made here on the CPU: exact pre-activations, 1 % .. 20 % of them exactly zero, op(x)
    non-negative and zero wherever the mask is closed."""
    for case in DJ.CASES:
        for name in DJ.DTYPE_NAMES:
            r = DJ.exact_case(case, name)
            assert 0.01 <= r["zero_share"] <= 0.20
            assert bool((r["op"].float() >= 0).all()) and r["op"].dtype == DJ.DTYPES[name]
            assert float((r["op"].float() > 0).float().mean()) > 0.3


def test_use_native_dense_block_switches_four_blocks():
    from ssds.modeling.layers import densetrain as DT
    from ssds.modeling.nets.densenet import DenseNet121, _DenseBlock

    model = DenseNet121(outputs=[2, 3, 4])
    state = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
    before = dict(DT.STATS)
    assert DT.use_native_dense_block(model) == 4
    blocks = [m for m in model.modules() if isinstance(m, _DenseBlock)]
    assert len(blocks) == 4 and all(type(b) is DT.TrainDenseBlock for b in blocks)
    assert [len(b) for b in blocks] == [6, 12, 24, 16]
    assert [(k, tuple(v.shape)) for k, v in model.state_dict().items()] == state
    assert DT.STATS["swapped"] == before["swapped"] + 4
    assert DT.use_native_dense_block(model) == 0  # a second call switches nothing more
    assert DT.DEFAULT in ("0", "1")


def test_swapped_model_equals_the_module_on_cpu():
    """fp32 on the CPU, train mode: every block falls back -- outputs, the input gradient, every parameter gradient and every
    buffer bit for bit, each fallback counted with its reason.  Eval mode the same."""
    import torch
    from ssds.modeling.layers import densetrain as DT
    from ssds.modeling.nets.densenet import DenseNet

    torch.manual_seed(3)
    ref = DenseNet(32, (2, 3), 64, outputs=[1, 2]).train()
    swapped = copy.deepcopy(ref)
    assert DT.use_native_dense_block(swapped) == 2
    x = torch.randn(2, 3, 48, 48)
    before, reasons = dict(DT.STATS), dict(DT.FALLBACK_REASONS)
    outs = []
    for m in (ref, swapped):
        xi = x.clone().requires_grad_(True)
        ys = m(xi)
        sum((t * t).mean() for t in ys).backward()
        outs.append((ys, dict({k: p.grad for k, p in m.named_parameters()}, input=xi.grad), dict(m.named_buffers())))
    (ya, ga, ba), (yb, gb, bb) = outs
    assert len(ya) == len(yb) == 2 and all(torch.equal(u, v) for u, v in zip(ya, yb))
    assert list(ga) == list(gb) and all(g is not None for g in ga.values())
    assert all(torch.equal(ga[k], gb[k]) for k in ga), [k for k in ga if not torch.equal(ga[k], gb[k])]
    assert list(ba) == list(bb) and all(torch.equal(ba[k], bb[k]) for k in ba)
    assert DT.STATS["fallback"] == before["fallback"] + 2 and DT.STATS["native_forward"] == before["native_forward"]
    assert DT.FALLBACK_REASONS["not a 4-d tensor on a HIP device"] == reasons.get("not a 4-d tensor on a HIP device", 0) + 2
    ref.eval(), swapped.eval()
    with torch.no_grad():
        assert all(torch.equal(u, v) for u, v in zip(ref(x), swapped(x)))
    assert DT.FALLBACK_REASONS["eval mode"] == reasons.get("eval mode", 0) + 2


def test_supported_refuses_by_name():
    import torch.nn as nn
    from ssds.modeling.layers import densetrain as DT
    from ssds.modeling.nets.densenet import _DenseBlock

    assert DT.supported(_DenseBlock(3, 64, 4, 32, 0)) and DT.unsupported_reason(_DenseBlock(3, 64, 4, 32, 0)) is None
    assert not DT.supported(_DenseBlock(3, 64, 4, 32, 0.2)) and "drop_rate" in DT.unsupported_reason(_DenseBlock(3, 64, 4, 32, 0.2))
    assert not DT.supported(_DenseBlock(3, 64, 4, 48, 0)) and "growth 48" in DT.unsupported_reason(_DenseBlock(3, 64, 4, 48, 0))
    assert "bottleneck width 64" in DT.unsupported_reason(_DenseBlock(3, 64, 2, 32, 0))
    assert not DT.supported(nn.Sequential()) and not DT.supported(_DenseBlock(0, 64, 4, 32, 0))
    model = nn.Sequential(_DenseBlock(2, 64, 4, 48, 0), _DenseBlock(2, 64, 4, 32, 0.1))
    assert DT.use_native_dense_block(model) == 0 and all(type(m) is _DenseBlock for m in model)


_SOLVER = r"""
from ssds.core import config
from ssds.utils import train_ddp
from ssds.modeling.layers import densetrain as DT
from ssds.modeling.nets.densenet import _DenseBlock
cfg = config.cfg_from_file(%(cfg)r)
s = train_ddp.Solver(cfg, 0, torch.device("cpu"), sync_bn=%(sync)r)
blocks = [m for m in s.model.modules() if isinstance(m, _DenseBlock)]
print("RESULT", len(blocks), sum(type(m) is DT.TrainDenseBlock for m in blocks), DT.STATS["swapped"])
"""


def _solver(cfg_name, switch, sync=False):
    return run_solver_script(_SOLVER, cfg_name, env={"SSDK_DENSE_TRAIN": switch}, text=True, sync=sync)


@pytest.mark.parametrize("switch", [None, "0", "1"])
def test_solver_routing(switch):
    """train_ddp.Solver on a DenseNet config (the switch is read when the Solver is built: a subprocess per setting): with the switch
    on the four blocks are TrainDenseBlock, with 0 none is.  Unset follows densetrain.DEFAULT."""
    from ssds.modeling.layers import densetrain as DT

    on = (DT.DEFAULT if switch is None else switch) == "1"
    res, _ = _solver("fpn_densenet121_640.yml", switch)
    assert res == ([4, 4, 4] if on else [4, 0, 0])


def test_solver_keeps_sync_bn_on_the_module_path():
    res, text = _solver("fpn_densenet121_640.yml", "1", sync=True)
    assert res == [4, 0, 0] and text.count("SSDK_DENSE_TRAIN: --sync-bn keeps the dense blocks on the module path") == 1


@pytest.mark.parametrize("switch", ["0", "1"])
def test_solver_leaves_other_backbones_alone(switch):
    res, _ = _solver("ssd_mobilenetv2_512.yml", switch)
    assert res == [0, 0, 0]
