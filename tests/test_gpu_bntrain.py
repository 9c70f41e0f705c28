"""The BatchNorm training kernels on the GPU (csrc/ssdk_bntrain.hip), per channel and per element against fp64 on the CPU.  The
operands, the truth, the bars (every one derived: none is a measured number), the case list and the checks are tests/bnjudge.py;
every test prints ``worst |err| / bar`` per quantity.

Three runs, each with the kernel names asserted through ``ssdk_last_kernel()`` on the test thread:
  * the default dispatch in process: the flat reduction everywhere, the flat apply pass exactly where the plane size is no multiple
    of the vector width or a pointer is misaligned, bn_fwd_finalize_kernel for handed-over sums;
  * SSDK_BN_FLAT=0 (only bn_reduce_kernel / bn_apply_kernel) and SSDK_BN_FLAT=1 (only the flat pair): the switch is read once per
    process, so ONE child process per value runs its whole case list and the parent reads its ``RESULT`` line (the pattern of
    tests/test_gpu_dwtrain.py::tiled_child), one child after the other.
Beyond the random-data bars: the stats-only entry and the statistics hand-over, exact counts (dy = 1, integer x, constant x),
one-hot gradients on both sides of every seam, misaligned tensors between NaN guards, and the split path per channel."""
import json
import os
import subprocess
import sys

import pytest

import bnjudge as J

pytestmark = pytest.mark.gpu
_SEEN = {}  # family -> kernel names its run reported


def _settle(rec, family):
    print("\n".join(rec["lines"]))
    if rec["names"] is not None:
        print("%s: kernels %s" % (rec["what"], sorted(set(rec["names"]))))
        _SEEN.setdefault(family, set()).update(n for joined in rec["names"] for n in joined.split("+"))
    assert not rec["failures"], "%s: %s" % (rec["what"], rec["failures"])
    return rec


def test_this_process_runs_the_default_dispatch():
    assert J.family_of_this_process() == "default", "SSDK_BN_FLAT is set: the in-process tests assert the default dispatch"


# ---- the default dispatch, in process ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype_name", J.DTYPE_NAMES)
@pytest.mark.parametrize("shape", J.CASES, ids=J.sid)
def test_random_data_per_channel_and_element(shape, dtype_name):
    rec = _settle(J.check_random(shape, dtype_name, "default"), "default")
    hw = shape[2] * shape[3]
    flat = hw % J.vec_width(dtype_name) != 0
    assert all(n == "bn_reduce_flat_kernel+" + ("bn_apply_flat_kernel" if flat else "bn_apply_kernel") for n in rec["names"])


@pytest.mark.parametrize("dtype_name", J.DTYPE_NAMES)
@pytest.mark.parametrize("shape", J.CASES, ids=J.sid)
def test_stats_only_and_hand_over(shape, dtype_name):
    rec = _settle(J.check_stats(shape, dtype_name, "default"), "default")
    assert rec["names"][0] == "bn_reduce_flat_kernel" and rec["names"][1] == "bn_fwd_finalize_kernel"
    assert rec["names"][2].startswith("bn_fwd_finalize_kernel+bn_apply_")


@pytest.mark.parametrize("dtype_name", J.DTYPE_NAMES)
@pytest.mark.parametrize("shape", J.CASES, ids=J.sid)
def test_exact_counts(shape, dtype_name):
    _settle(J.check_counts(shape, dtype_name, "default"), "default")


@pytest.mark.parametrize("dtype_name", J.DTYPE_NAMES)
@pytest.mark.parametrize("shape", J.ONEHOT_CASES, ids=J.sid)
def test_one_hot_gradient(shape, dtype_name):
    _settle(J.check_onehot(shape, dtype_name, "default"), "default")


@pytest.mark.parametrize("dtype_name", J.DTYPE_NAMES)
@pytest.mark.parametrize("shape", J.ALIGN_CASES, ids=J.sid)
def test_misaligned_tensors_between_guards(shape, dtype_name):
    rec = _settle(J.check_alignment(shape, dtype_name, "default"), "default")
    assert rec["names"] == ["bn_reduce_flat_kernel+bn_apply_flat_kernel"] * 2  # (a misaligned pointer: the flat apply)


@pytest.mark.parametrize("dtype_name", J.DTYPE_NAMES)
@pytest.mark.parametrize("sizes", J.SPLIT_RANKS, ids=lambda s: "ranks" + "_".join(str(v) for v in s))
@pytest.mark.parametrize("shape", J.SPLIT_CASES, ids=J.sid)
def test_split_path_per_channel(shape, sizes, dtype_name):
    _settle(J.check_split(shape, dtype_name, sizes), "default")


# ---- the two forced families: one child process each, one after the other ------------------------------------------------------------
def _child(family):
    env = dict(os.environ, SSDK_BN_FLAT=J.FAMILIES[family])
    out = subprocess.run([sys.executable, os.path.join(J.ROOT, "tests", "bnjudge.py"), "--family", family], env=env, capture_output=True,
                         text=True, timeout=600)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-3000:])
    lines = [l for l in out.stdout.splitlines() if l.startswith("RESULT ")]
    assert len(lines) == 1, out.stdout[-2000:]
    return json.loads(lines[0][len("RESULT "):])


@pytest.fixture(scope="module")
def per_plane_child():
    return _child("per_plane")


@pytest.fixture(scope="module")
def flat_child(per_plane_child):  # (depends on the other child: never both at once)
    return _child("flat")


@pytest.mark.parametrize("case", J.child_cases(), ids=J.case_id)
def test_per_plane_family_by_the_switch(per_plane_child, case):
    rec = _settle(per_plane_child[J.case_id(case)], "per_plane")
    if rec["names"] is not None:
        assert set(rec["names"]) == {"bn_reduce_kernel+bn_apply_kernel"}, rec["names"]


@pytest.mark.parametrize("case", J.child_cases(), ids=J.case_id)
def test_flat_family_by_the_switch(flat_child, case):
    rec = _settle(flat_child[J.case_id(case)], "flat")
    if rec["names"] is not None:
        assert set(rec["names"]) == {"bn_reduce_flat_kernel+bn_apply_flat_kernel"}, rec["names"]


def test_the_children_ran_every_case_and_the_three_runs_reached_every_kernel(per_plane_child, flat_child):
    want = sorted(J.case_id(c) for c in J.child_cases())
    assert sorted(per_plane_child) == want and sorted(flat_child) == want
    for family, child in (("per_plane", per_plane_child), ("flat", flat_child)):
        for rec in child.values():
            _SEEN.setdefault(family, set()).update(n for joined in (rec["names"] or []) for n in joined.split("+"))
    # (the default dispatch's own share again, so that this test does not depend on which tests ran before it)
    for rec in (J.check_random((4, 32, 16, 24), "bf16", "default"), J.check_random((5, 7, 19, 19), "bf16", "default"),
                J.check_stats((3, 5, 3, 3), "bf16", "default")):
        _settle(rec, "default")
    print("kernels per run:", {k: sorted(v) for k, v in _SEEN.items()})
    assert _SEEN["per_plane"] == {"bn_reduce_kernel", "bn_apply_kernel"}
    assert _SEEN["flat"] == {"bn_reduce_flat_kernel", "bn_apply_flat_kernel"}
    assert _SEEN.get("default", set()) == {"bn_reduce_flat_kernel", "bn_apply_kernel", "bn_apply_flat_kernel", "bn_fwd_finalize_kernel"}
