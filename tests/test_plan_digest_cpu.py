"""Every byte the C executor sees of a recorded plan, against tests/golden/plan_digest.json (written by
tests/golden/make_plan_digest.py at the commit whose recordings are the reference): the ``ssdk_op`` array with its addresses resolved
to arena buffers and pack tensors, the ``layer_table()`` rows, the patch list, the head list, the arena's buffer sizes and the pinned
buffers of every plan of ``plandigest.PLANS``.  No device is needed: the plans are recorded on the CPU device at the golden cases'
sizes, and recording calls only host predicates of the library."""
import json
import os

import pytest

import plandigest
from ssds.modeling.layers import fused_conv as FC

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "plan_digest.json")


@pytest.fixture(scope="module")
def recorded():
    """{key: (canonical text, plan)} of every plan, each model built once."""
    models = {}
    return {key: plandigest.record(key, models) for key in plandigest.PLANS}


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_golden_names_the_plans(golden):
    assert list(golden) == list(plandigest.PLANS)
    cases = plandigest.all_cases()
    assert {v.case for k, v in plandigest.PLANS.items() if k.endswith("/bf16")} == set(cases)  # every case, no switch set, in bf16
    assert len(plandigest.FP16) >= 6 and set(plandigest.FP16) <= set(cases)
    envs = [v.env for v in plandigest.PLANS.values() if v.env]
    for env in ({"SSDK_DKRES": "0"}, {"SSDK_DKRES": "1"}, {"SSDK_WFRAG": "0"}):
        assert env in envs
    assert any(env.get("SSDK_LEVEL_LANES") == "0" for env in envs)


@pytest.mark.parametrize("key", list(plandigest.PLANS))
def test_plan_is_what_the_reference_commit_recorded(key, recorded, golden):
    canon, _ = recorded[key]
    want = golden[key]
    if "unsupported" in want or "unsupported" in canon:
        assert canon == want
        return
    got = plandigest.digest(canon)
    for i, (g, w) in enumerate(zip(got["ops"], want["ops"])):
        if g != w:
            print("%s: op %d differs\n  recorded now: %s\n  golden:       %s\n  its words now: %s" % (key, i, g, w, canon["ops"][i][4]))
            break
    assert got["ops"] == want["ops"]
    for part in ("patches", "heads", "bufs", "pinned"):
        assert got[part] == want[part], (key, part)


def test_the_plans_cover_every_op_kind_and_path(recorded):
    """Conditions on the chosen plans, not measurements: a later change of the cases cannot hollow the comparison out."""
    plans = [p for _, p in recorded.values() if p is not None]
    layers = [L for p in plans for L in p.layers]
    kinds = {L.get("kind") for L in layers}
    assert kinds == {None, "mb", "mbse", "convt", "cat", "spp", "xpair", "dkres", "dense", "densepool", "denseplace", "shuffle",
                     "shuffledown", "stem7", "pool", "fuse"}
    assert kinds == set(getattr(FC, "OP_KINDS", kinds))  # (the op table, where the code under test has one)
    assert {op.lane for p in plans for op in p.ops} == {0, 1, 2}
    assert {h[6] for p in plans for h in p.heads} == {"both", "loc", "conf"}
    assert {L["res_mode"] for L in layers if L.get("kind") is None and L["res"] is not None} == {0, 1, 2}
    assert {L["res"] is not None for L in layers if L.get("kind") == "mbse"} == {True, False}
    # a concatenation of zero-padded maps: only behind one does a pack carry more than one (real, physical) segment
    assert any(len(getattr(L.get("pack"), "in_segs", None) or ()) > 1 for L in layers)
    assert any(L.get("kind") == "cat" for p in plans for L in p.layers if any(
        len(getattr(M.get("pack"), "in_segs", None) or ()) > 1 for M in p.layers))
    fields = {f for p in plans for _, f, _ in p.patches}
    # (conv.residual, fuse.a / fuse.b / fuse.c, xpair.x, mbse.x and pool.x are patched only where an EXTERNAL input is a residual,
    #  a fusion source or the input of such an op: no planner walk of the golden cases records that -- every neck starts with a
    #  convolution on each backbone map)
    assert fields == {"conv.x", "mb.x", "stem.x"}, fields
