"""The 7x7 stem convolution of the training step (csrc/ssdk_stem7train.hip, ssds/modeling/layers/stemconv.py), the parts that need no
GPU: which layers ``use_native_stem7`` switches, that a switched layer keeps its parameter, its ``state_dict`` and its CPU result,
what the explicit function does with host tensors, the argument checks of the C entry points (all made before any device call),
the Solver's routing under SSDK_STEM7_TRAIN and the benchmark's JSON line."""
import io
import json
import os
import subprocess
import sys

import pytest

from solverhelp import run_solver_script

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW = ("ssdk_stem7x7s2_wgrad_workspace_bytes", "ssdk_stem7x7s2_fwd", "ssdk_stem7x7s2_wgrad")


def _model(cfg_name):
    from ssds.core import config
    from ssds.modeling import model_builder

    cfg = config.cfg_from_file(os.path.join(ROOT, "experiments", "cfgs", cfg_name))
    return model_builder.create_model(cfg.MODEL)


@pytest.mark.parametrize("cfg_name,want", [("fpn_resnet50_640.yml", 1), ("fpn_resnext50_640.yml", 1), ("ssd_mobilenetv2_300.yml", 0),
                                           ("bifpn_regnetx008_896.yml", 0)])
def test_use_native_stem7_switches_exactly_the_stem(cfg_name, want):
    import torch
    import torch.nn as nn
    from ssds.modeling.layers import stemconv as S

    torch.manual_seed(0)
    model = _model(cfg_name)
    before = {k: v.clone() for k, v in model.state_dict().items()}
    classes = [type(m) for m in model.modules()]
    swapped = S.STATS["swapped"]
    assert S.use_native_stem7(model) == want and S.STATS["swapped"] == swapped + want
    after = [type(m) for m in model.modules()]
    assert [(a, b) for a, b in zip(classes, after) if a is not b] == [(nn.Conv2d, S.StemConv7x7s2)] * want
    if want:
        assert type(model.backbone.conv1) is S.StemConv7x7s2
    assert S.use_native_stem7(model) == 0  # a second call switches nothing more
    state = model.state_dict()
    assert list(state.keys()) == list(before.keys()) and all(torch.equal(state[k], before[k]) for k in before)
    if want:
        # a checkpoint round-trips: saved from the switched model, loaded into a fresh plain one and back
        buf = io.BytesIO()
        torch.save(state, buf)
        buf.seek(0)
        loaded = torch.load(buf)
        fresh = _model(cfg_name)
        fresh.load_state_dict(loaded)
        assert torch.equal(fresh.backbone.conv1.weight, model.backbone.conv1.weight)
        model.load_state_dict(fresh.state_dict())
        assert all(torch.equal(model.state_dict()[k], before[k]) for k in before)


def test_other_7x7_layers_are_left_alone():
    import torch.nn as nn
    from ssds.modeling.layers import stemconv as S

    others = nn.Sequential(nn.Conv2d(3, 64, 7, 2, 3, bias=True), nn.Conv2d(3, 64, 7, 1, 3, bias=False), nn.Conv2d(4, 64, 7, 2, 3, bias=False),
                           nn.Conv2d(3, 96, 7, 2, 3, bias=False), nn.Conv2d(3, 64, 7, 2, 2, bias=False), nn.Conv2d(3, 64, 5, 2, 2, bias=False),
                           nn.Conv2d(3, 64, 7, 2, 3, bias=False, padding_mode="reflect"))
    assert S.use_native_stem7(others) == 0 and all(type(m) is nn.Conv2d for m in others)
    assert S.use_native_stem7(nn.Sequential(nn.Conv2d(1, 16, 7, 2, 3, bias=False), nn.Conv2d(3, 64, 7, 2, 3, bias=False))) == 2


def test_switched_layer_on_cpu_tensors_is_conv2d():
    import torch
    import torch.nn as nn
    import torch.nn.functional as F
    from ssds.modeling.layers import stemconv as S

    torch.manual_seed(1)
    seq = nn.Sequential(nn.Conv2d(3, 64, 7, 2, 3, bias=False))
    assert S.use_native_stem7(seq) == 1 and type(seq[0]) is S.StemConv7x7s2
    x = torch.randn(2, 3, 19, 23)
    calls = dict(S.STATS)
    y = seq(x)
    assert torch.equal(y, F.conv2d(x, seq[0].weight, None, 2, 3))
    y.sum().backward()
    assert seq[0].weight.grad is not None
    assert [S.STATS[k] - calls[k] for k in ("native_forward", "native_wgrad", "fallback")] == [0, 0, 1]


def test_explicit_function_refuses_host_tensors():
    import torch
    from ssds import _native as N
    from ssds.modeling.layers import stemconv as S

    with pytest.raises(N.SsdkError, match="no CPU fallback"):
        S.stem_conv7x7s2(torch.zeros(1, 3, 8, 8, dtype=torch.bfloat16), torch.zeros(64, 3, 7, 7))


def test_c_entry_points_are_exported_and_refuse_bad_arguments():
    from ssds import _native as N

    header = open(os.path.join(ROOT, "include", "ssdk.h")).read()
    for name in NEW:
        assert name in N.EXPORTS and (name + "(") in header and hasattr(N.lib, name), name
    assert N.lib.ssdk_version() == 245 and N.ABI_VERSION == 245
    L = N.lib
    F = 0x1000  # never dereferenced: every call below fails validation first
    err = lambda: L.ssdk_last_error().decode()  # noqa: E731
    need = int(L.ssdk_stem7x7s2_wgrad_workspace_bytes(2, 64, 64, 64))
    assert need > 0 and need % 16 == 0
    for bad in ((0, 64, 64, 64), (2, 0, 64, 64), (2, 64, 0, 64), (2, 64, 64, 0), (2, 64, 64, 65), (-1, 64, 64, 64)):
        assert L.ssdk_stem7x7s2_wgrad_workspace_bytes(*bad) == 0, bad

    def fwd(x=F, w=F, y=F, n=2, cin=3, h=64, wd=64, cout=64, dt=N.BF16):
        return L.ssdk_stem7x7s2_fwd(x, w, y, n, cin, h, wd, cout, dt, None)

    def wgrad(x=F, dy=F, dw=F, ws=F, nbytes=need, n=2, cin=3, h=64, wd=64, cout=64, dt=N.BF16):
        return L.ssdk_stem7x7s2_wgrad(x, dy, dw, ws, nbytes, n, cin, h, wd, cout, dt, None)

    shared = [dict(x=None), dict(cin=0), dict(cin=4), dict(cout=0), dict(cout=65), dict(dt=N.F32), dict(dt=3), dict(n=0), dict(h=0), dict(wd=0)]
    for kw in shared + [dict(w=None), dict(y=None)]:
        assert fwd(**kw) == -1 and "stem7x7s2_fwd" in err(), (kw, err())
    for kw in shared + [dict(dy=None), dict(dw=None), dict(ws=None), dict(nbytes=need - 1), dict(nbytes=0), dict(ws=F + 8), dict(ws=F + 4)]:
        assert wgrad(**kw) == -1 and "stem7x7s2_wgrad" in err(), (kw, err())


_SOLVER = r"""
import torch.nn as nn
from ssds.core import config
from ssds.utils import train_ddp
from ssds.modeling.layers import stemconv as S
cfg = config.cfg_from_file(%(cfg)r)
s = train_ddp.Solver(cfg, 0, torch.device("cpu"))
mods = list(s.model.modules())
sevens = [m for m in mods if isinstance(m, nn.Conv2d) and m.kernel_size == (7, 7)]
print("RESULT", len(sevens), sum(type(m) is S.StemConv7x7s2 for m in mods), sum(type(m) is nn.Conv2d for m in sevens), S.STATS["swapped"])
"""


@pytest.mark.parametrize("cfg_name,stems", [("fpn_resnext50_640.yml", 1), ("bifpn_regnetx016_896.yml", 0)])
@pytest.mark.parametrize("switch", [None, "1", "0"])
def test_solver_routing(cfg_name, stems, switch):
    """train_ddp.Solver switches the 7x7 stem of a ResNet / ResNeXt backbone according to SSDK_STEM7_TRAIN (read when the Solver is
    built; a subprocess per value; unset is stemconv.DEFAULT); with 0 the layer stays a plain nn.Conv2d; a RegNetX model has none."""
    from ssds.modeling.layers import stemconv as S

    sevens, native, plain, swapped = run_solver_script(_SOLVER, cfg_name, env={"SSDK_STEM7_TRAIN": switch})
    assert sevens == stems
    on = (S.DEFAULT if switch is None else switch) != "0"
    if on:
        assert (native, plain, swapped) == (stems, 0, stems)
    else:
        assert (native, plain, swapped) == (0, stems, 0)


def test_bench_train_json_line_carries_stem7_train():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "bench_train.py"), "--cpu", "1", "--steps", "1", "--warmup", "0"],
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    line = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert line["stem7_train"] is False and "neck_train" in line
