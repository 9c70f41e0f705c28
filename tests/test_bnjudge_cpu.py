"""The judge of the BatchNorm training kernels (tests/bnjudge.py) on the CPU: an fp32 model of the passes (pivot sums in the kernels'
order, bn_fwd_out, bn_bwd_coef, apply, one rounding to the dtype) passes every check on every case and dtype; each mutation of the
model fails at least one check; the depths stay under the cap and every case is between 5 % and 95 % open; the mirrored split
agrees with the library's workspace size; the reciprocal division of bn_apply_flat_kernel is exact over its whole domain."""
import numpy as np
import pytest
import torch

import bnjudge as J


def _runner(dtype_name, family="flat", mutation=None):
    return lambda op, act: J.model(op, act, dtype_name, family, None, mutation)


def _stats_runner(dtype_name, mutation=None):
    return lambda op, act, sums: J.model(op, act, dtype_name, "flat", sums, mutation)


def _show(rec):
    print("\n".join(rec["lines"]))
    return rec


@pytest.mark.parametrize("dtype_name", J.DTYPE_NAMES)
@pytest.mark.parametrize("shape", J.CASES, ids=J.sid)
def test_fp32_model_passes_every_check(shape, dtype_name):
    worst = {}
    recs = [J.check_random(shape, dtype_name, "flat", _runner(dtype_name, "flat")),
            J.check_random(shape, dtype_name, "per_plane", _runner(dtype_name, "per_plane")),
            J.check_stats(shape, dtype_name, "flat", _stats_runner(dtype_name)),
            J.check_counts(shape, dtype_name, "flat", _runner(dtype_name))]
    if shape in J.ONEHOT_CASES:
        recs.append(J.check_onehot(shape, dtype_name, "flat", _runner(dtype_name)))
    for rec in recs:
        _show(rec)
        assert not rec["failures"], (rec["what"], rec["failures"])
        for k, v in rec["ratios"].items():
            q = k.split(" ")[-1]
            worst[q] = max(worst.get(q, 0.0), v)
    print("model %s %s: worst |err| / bar per quantity: %s" % (J.sid(shape), dtype_name,
                                                              ", ".join("%s %.3f" % kv for kv in sorted(worst.items()))))
    assert {"mean", "invstd", "rm", "rv", "a", "b", "y", "dbeta", "dgamma", "dx"} <= set(worst)


# mutation -> [(check, shape, dtype)]: at least one of them must fail
MUTATIONS = {
    "tail": [("counts", (5, 7, 19, 19), "bf16"), ("random", (2, 6, 150, 150), "f32")],     # last element of each plane not reduced
    "straddle": [("random", (3, 5, 3, 3), "bf16"), ("random", (5, 7, 19, 19), "f32")],     # neighbour channel's coefficients
    "biased": [("random", (3, 5, 3, 3), "f32"), ("random", (5, 7, 19, 19), "bf16")],       # running_var without M / (M - 1)
    "short": [("random", (5, 7, 19, 19), "f32"), ("random", (70, 3, 10, 10), "f16")],      # M short by one plane
    # ReLU6 mask closed at 6 (bf16: a few pre-activations per case round to 6 exactly, in fp32 none does)
    "mask6": [("random", (5, 7, 19, 19), "bf16"), ("random", (66, 16, 8, 8), "bf16")],
    "slice": [("random", (66, 16, 8, 8), "f32"), ("counts", (70, 3, 10, 10), "bf16")],     # one slice omitted, N % split != 0
    "pivot0": [("random", (2, 6, 150, 150), "f32"), ("random", (5, 7, 19, 19), "bf16")],   # pivot 0 on the 50 / 0.1 channel
}


@pytest.mark.parametrize("mutation", sorted(MUTATIONS))
def test_mutations_of_the_model_fail(mutation):
    caught = 0
    for kind, shape, dtype_name in MUTATIONS[mutation]:
        clean = J.CHECKS[kind](shape, dtype_name, "flat", _runner(dtype_name))
        assert not clean["failures"], clean["failures"]
        rec = J.CHECKS[kind](shape, dtype_name, "flat", _runner(dtype_name, mutation=mutation))
        print("%s on %s %s %s: %d failures, first: %s" % (mutation, kind, J.sid(shape), dtype_name, len(rec["failures"]),
                                                         rec["failures"][:1]))
        caught += bool(rec["failures"])
    assert caught == len(MUTATIONS[mutation]), "the judge let the mutation %r pass somewhere" % mutation


def test_pivot0_misses_the_pivot_bar_on_the_50_01_channel_only():
    shape, dtype_name = (2, 6, 150, 150), "f32"
    rec = J.check_random(shape, dtype_name, "flat", _runner(dtype_name, mutation="pivot0"))
    assert rec["ratios"]["act0 invstd"] > 10, rec["ratios"]["act0 invstd"]


def test_depths_are_under_the_cap_and_every_case_is_open():
    for shape in J.CASES + J.SPLIT_CASES:
        n, c, h, w = shape
        for dt in J.DTYPE_NAMES:
            d = J.depth(n, c, h * w, dt, ranks=4)
            assert 10 <= d <= J.DEPTH_CAP, (shape, dt, d)
            for special in (True, False):
                shares = J.open_shares(J.operands(shape, dt, special))
                assert all(0.05 <= s <= 0.95 for s in shares), (shape, dt, shares)
    assert J.depth(2, 6, 22500, "bf16") == 89 + 6 + 3 + 2 and J.depth(70, 3, 100, "bf16") == 9 + 6 + 3 + 64


def test_the_mirrored_split_agrees_with_the_library():
    assert J.bn_split(70, 3) == 64 and J.bn_split(3, 1100) == 1 and J.bn_split(4, 32) == 4 and J.bn_split(1, 2) == 1
    try:
        from ssds import _native as N
    except (ImportError, OSError) as e:
        print("libssdk.so does not load here (%s): the mirror is checked against its own formula only" % e)
        return
    for n, c in [(s[0], s[1]) for s in J.CASES + J.SPLIT_CASES] + [(64, 16), (65, 16), (7, 1024), (7, 1025), (200, 1), (1, 1)]:
        assert int(N.lib.ssdk_bn_workspace_bytes(n, c)) == J.workspace_bytes(n, c), (n, c)


def test_reciprocal_division_of_the_flat_apply_pass_is_exact():
    """bn_div_small: (int)((v + 0.5f) * (1.0f / d)) == v // d in float32 -- exhaustively for the plane division (d = HW < 8192, v < 8200:
    an offset inside one workgroup's 8192 elements plus a vector), and for the channel wrap (d = C < 2^19, v < C + 8200) on every C
    below 5000, powers of two and their neighbours, and a seeded sample"""
    v = np.arange(0, 8200, dtype=np.int64)
    vf = v.astype(np.float32) + np.float32(0.5)
    bad = [d for d in range(1, 8192) if not np.array_equal((vf * (np.float32(1.0) / np.float32(d))).astype(np.int64), v // d)]
    assert not bad, bad[:5]
    rng = np.random.default_rng(0)
    p2 = 1 << np.arange(1, 19)
    cs = np.unique(np.concatenate([np.arange(1, 5000), rng.integers(1, 1 << 19, 3000), p2, p2 - 1, p2 + 1, [(1 << 19) - 1]]))
    for c in cs:
        vv = np.arange(0, c + 8200, dtype=np.int64) if c < 20000 else np.concatenate([np.arange(c - 50, c + 8200), np.arange(0, 100)])
        q = ((vv.astype(np.float32) + np.float32(0.5)) * (np.float32(1.0) / np.float32(c))).astype(np.int64)
        assert np.array_equal(q, vv // c), int(c)


def test_one_hot_positions_sit_on_both_sides_of_the_seams():
    pos = set(J.onehot_positions((2, 6, 150, 150), "bf16"))
    assert {(1, 5, 8191), (1, 5, 8192), (1, 5, 16383), (1, 5, 16384), (1, 5, 22499), (0, 1, 0), (0, 0, 2047), (0, 0, 2048)} <= pos
    pos = set(J.onehot_positions((70, 3, 10, 10), "bf16"))
    assert {(26, 2, 99), (27, 0, 0), (63, 1, 99), (64, 1, 0), (69, 2, 99)} <= pos
