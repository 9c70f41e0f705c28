"""Depthwise 3x3 convolutions of the TRAINING step on the GPU (csrc/ssdk_dwplane.hip: whole-row kernels; csrc/ssdk_dwtrain.hip: the
entry points and the 32 x 64-tile kernels; behind ssds/modeling/layers/dwconv.py), per element against ``F.conv2d`` autograd in fp64
on the CPU.  The operands, the truth, the bars and the case lists are tests/dwjudge.py; every test prints ``worst |err| / bar`` per
tensor.

Three routes to the kernels, each with the kernel names asserted through the entry points on the test thread:
  * the whole-row family under the default dispatch, its coverage (several images per workgroup with a ragged last group, bands,
    a ragged last band, rows that are and are not a multiple of eight) pinned by ssdk_dwconv_plan;
  * the tiled family by the switch: SSDK_DW_PLANE=0 is read once per process, so ONE child process runs the whole family and the
    parent reads its ``RESULT`` line (the pattern of tests/test_gpu_necktrain.py::test_the_switch);
  * the tiled family by the dispatcher: rows too wide for the whole-row kernels' LDS budget, in process.
Beyond the random-data bars: exact tests (all ones: every tensor is a count; one-hot gradients on both sides of every band, group
and tile seam), the statistics hand-over against the fp64 sums of the unrounded output, the deferred-BatchNorm variants called
directly with operands whose staged tensor is exact, and misaligned tensors between NaN guards."""
import json
import os
import subprocess
import sys

import pytest

import dwjudge as J

pytestmark = pytest.mark.gpu
DTYPE_NAMES = ["f32", "bf16", "f16"]
HALF_NAMES = ["bf16", "f16"]


def _settle(rec):
    print("\n".join(rec["lines"]))
    if rec["names"] is not None:
        print("%s: kernels %s" % (rec["what"], rec["names"]))
    assert not rec["failures"], "%s: %s" % (rec["what"], rec["failures"])
    return rec


def test_depths_are_under_the_cap():
    sum_depth, stats_depth = J.depths()
    assert sum_depth <= 256 and stats_depth <= 256


# ---- the whole-row family --------------------------------------------------------------------------------------------------------
def test_whole_row_family_covers_what_the_plan_can_do():
    """by the library's own answer: several images per workgroup with a ragged last group, bands, a ragged last band, rows of whole
    and of partial eight-pixel segments; the 16-bit passes of every shape stay on this family, the fp32 forward and weight gradient
    of the 3000-pixel row do not"""
    plans = []
    for shape in J.WHOLE_ROW:
        for stride in J.STRIDES:
            for dt in DTYPE_NAMES:
                for kind in range(3):
                    p = J.plan(kind, shape, stride, dt)
                    if dt != "f32" or shape != J.WIDE:
                        assert p is not None, (shape, stride, dt, kind)
                    elif kind != 1:
                        assert p is None, (shape, stride, dt, kind)
                    if p is not None:
                        wt = shape[3] if kind == 1 else J.out_hw(shape[2], shape[3], stride)[1]
                        plans.append(dict(p, N=shape[0], Wt=wt))
    assert any(p["G"] > 1 and p["N"] % p["G"] != 0 for p in plans)
    assert any(p["T"] > 1 for p in plans)
    assert any(p["T"] > 1 and p["Ht"] % p["TR"] != 0 for p in plans)
    assert any(p["Wt"] % 8 == 0 for p in plans) and any(p["Wt"] % 8 != 0 for p in plans)


@pytest.mark.parametrize("dtype_name", DTYPE_NAMES)
@pytest.mark.parametrize("stride", J.STRIDES)
@pytest.mark.parametrize("shape", J.WHOLE_ROW, ids=J.sid)
def test_whole_row_family(shape, stride, dtype_name):
    rec = _settle(J.check_random(shape, stride, dtype_name, "whole"))
    if dtype_name != "f32" or shape != J.WIDE:
        assert rec["names"] == J.WHOLE_NAMES
    else:  # the fp32 forward and weight gradient of the 3000-pixel row run on the tiles
        assert rec["names"][0] == J.TILED_NAMES[0] and rec["names"][2] == J.TILED_NAMES[2]


@pytest.mark.parametrize("dtype_name", DTYPE_NAMES)
@pytest.mark.parametrize("stride", J.STRIDES)
@pytest.mark.parametrize("shape", J.ONES["whole"], ids=J.sid)
def test_whole_row_all_ones_are_counts(shape, stride, dtype_name):
    _settle(J.check_ones(shape, stride, dtype_name, "whole"))


@pytest.mark.parametrize("dtype_name", DTYPE_NAMES)
@pytest.mark.parametrize("stride", J.STRIDES)
@pytest.mark.parametrize("shape", J.ONEHOT["whole"], ids=J.sid)
def test_whole_row_one_hot_gradient_is_exact(shape, stride, dtype_name):
    _settle(J.check_onehot(shape, stride, dtype_name, "whole"))


@pytest.mark.parametrize("dtype_name", HALF_NAMES)
@pytest.mark.parametrize("stride", J.STRIDES)
@pytest.mark.parametrize("shape", J.WHOLE_ROW, ids=J.sid)
def test_statistics_hand_over(shape, stride, dtype_name):
    _settle(J.check_stats(shape, stride, dtype_name))


@pytest.mark.parametrize("act", J.ACTS)
@pytest.mark.parametrize("dtype_name", HALF_NAMES)
@pytest.mark.parametrize("stride", J.STRIDES)
@pytest.mark.parametrize("shape", J.AFFINE, ids=J.sid)
def test_deferred_batchnorm_variants(shape, stride, dtype_name, act):
    _settle(J.check_affine(shape, stride, dtype_name, act))


@pytest.mark.parametrize("dtype_name", HALF_NAMES)
@pytest.mark.parametrize("stride", J.STRIDES)
@pytest.mark.parametrize("shape", J.ALIGN, ids=J.sid)
def test_whole_row_misaligned_tensors_between_guards(shape, stride, dtype_name):
    rec = _settle(J.check_alignment(shape, stride, dtype_name, "whole"))
    assert rec["names"] == J.WHOLE_NAMES


# ---- the tiled family, by the dispatcher -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype_name", DTYPE_NAMES)
@pytest.mark.parametrize("stride", J.STRIDES)
@pytest.mark.parametrize("shape", J.TILED_DISPATCH, ids=J.sid)
def test_tiled_family_by_the_dispatcher(shape, stride, dtype_name):
    from ssds import _native as N

    for kind in range(3):
        assert J.plan(kind, shape, stride, dtype_name) is None, kind
    assert int(N.lib.ssdk_dwconv_fwd_stats_workspace_bytes(*shape, stride, J.CODES[dtype_name])) == 0
    rec = _settle(J.check_random(shape, stride, dtype_name, "whole"))
    assert rec["names"] == J.TILED_NAMES


@pytest.mark.parametrize("dtype_name", DTYPE_NAMES)
@pytest.mark.parametrize("stride", J.STRIDES)
@pytest.mark.parametrize("shape", J.ONEHOT["dispatch"], ids=J.sid)
def test_tiled_by_the_dispatcher_one_hot_gradient_is_exact(shape, stride, dtype_name):
    _settle(J.check_onehot(shape, stride, dtype_name, "dispatch"))


# ---- the tiled family, by the switch: one child process --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiled_child():
    env = dict(os.environ, SSDK_DW_PLANE="0")
    out = subprocess.run([sys.executable, os.path.join(J.ROOT, "tests", "dwjudge.py"), "--family", "tiled"], env=env, capture_output=True,
                         text=True, timeout=600)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-3000:])
    lines = [l for l in out.stdout.splitlines() if l.startswith("RESULT ")]
    assert len(lines) == 1, out.stdout[-2000:]
    return json.loads(lines[0][len("RESULT "):])


@pytest.mark.parametrize("case", J.tiled_cases(), ids=J.case_id)
def test_tiled_family_by_the_switch(tiled_child, case):
    rec = _settle(tiled_child[J.case_id(case)])
    if case[0] in ("random", "align"):
        assert rec["names"] == J.TILED_NAMES and not any(n.startswith("dwp_") for n in rec["names"])


def test_the_child_ran_every_case_and_only_tiled_kernels(tiled_child):
    assert sorted(tiled_child) == sorted(J.case_id(c) for c in J.tiled_cases())
    names = {n for rec in tiled_child.values() if rec["names"] for n in rec["names"]}
    print("kernels of the child process:", sorted(names))
    assert names == set(J.TILED_NAMES)
