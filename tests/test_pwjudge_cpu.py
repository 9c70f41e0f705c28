"""The judge of the 1x1 training kernels and their 3x3 users (tests/pwjudge.py) on the CPU: it must be able to fail.  An fp32 model
of each pass -- 128-pixel chunk partials added in index order, the partial rows through a model of pw_wgrad_reduce_kernel, stores
rounded to the dtype -- passes every check at every case in both dtypes, the exact family included; each mutation of one pass fails
the check named for it.  The plan of every case is the library's own answer (the workspace queries are host code): the splits,
statistics rows and fold decisions the case lists pin are asserted here as well as on the GPU."""
import pytest
import torch

import pwjudge as J

ALL = [(kind, case) for kind in ("pw", "c3", "head") for case in J.CASES[kind]]


def _id(kc):
    return "%s-%s" % (kc[0], J.sid(kc[1]))


def _run(kind, case, dtype_name, family, mut=()):
    g = J.geo(kind, case)
    plan = J.plan_of(g)
    tr = J.truth(kind, case, dtype_name, family)
    got = J.model(g, tr["ops"], dtype_name, plan, mut)
    rec = J.new_rec("model %s %s %s %s %s" % (kind, J.sid(case), dtype_name, family, "+".join(mut)))
    if family == "random":
        return J.judge(rec, g, got, tr, dtype_name, plan)
    return J.judge_exact(rec, got, tr, dtype_name)


def _failed(rec):
    return sorted({f.split(":")[0] for f in rec["failures"]})


def test_the_queries_invert():
    """rows + ceil(rows / 64) is strictly increasing, and rows_from_total inverts it for 1 ... 4096"""
    totals = [s + (s + 63) // 64 for s in range(1, 4097)]
    assert all(b > a for a, b in zip(totals, totals[1:]))
    assert [J.rows_from_total(t) for t in totals] == list(range(1, 4097))


def test_the_plans_the_case_lists_pin():
    for case, (splits, _, _, rows) in J.PW.items():
        plan = J.plan_of(J.geo("pw", case))
        assert plan["wgrad"] == [(0, case[2], splits)], (case, plan)
        assert rows is None or plan["rows"] == rows, (case, plan)
    for kind in ("c3", "head"):
        for case, fold in J.CASES[kind].items():
            assert J.plan_of(J.geo(kind, case))["fold"] == fold, case
    two_pass = [c for c, v in J.PW.items() if v[0] > 64]
    assert len(two_pass) >= 3 and any(v[3] is not None and v[3] > 64 for v in J.PW.values())
    # D covers the longest split of every plan: cps_ub >= the chunks a split can hold
    for case, (splits, _, _, _) in J.PW.items():
        chunks = J.chunks_of(case[0], case[3] * case[4])
        cps = chunks if splits == 1 else -(-chunks // splits)
        assert J.depth_w(case[0], case[3] * case[4], splits) >= 128 * cps + 20


@pytest.mark.parametrize("dtype_name", J.DTYPE_NAMES)
@pytest.mark.parametrize("kc", ALL, ids=_id)
def test_the_model_passes_every_check(kc, dtype_name):
    kind, case = kc
    rec = _run(kind, case, dtype_name, "random")
    print("\n".join(rec["lines"]))
    assert not rec["failures"], rec["failures"]
    assert set(rec["ratios"]) == {"y", "dx", "dW", "dbias"} | ({"sum", "sumsq"} if kind == "pw" else set())
    for variant in J.VARIANTS:
        bad = J.exact_conditions(J.geo(kind, case), J.truth(kind, case, dtype_name, variant), dtype_name)
        assert not bad, (variant, bad)
        rec = _run(kind, case, dtype_name, variant)
        assert not rec["failures"], (variant, rec["failures"])


def test_the_exact_family_is_not_empty():
    """most outputs of a ternary case are non-zero, the all-ones dW is the per-tap count of in-plane outputs at both strides, and a
    one-hot dy gives one scaled pixel column of x and one scaled column of w"""
    tr = J.truth("head", (5, 512, 8, 8), "bf16", "ternary")
    assert float((tr["y"] != 0).double().mean()) > 0.85 and float((tr["dx"] != 0).double().mean()) > 0.85
    for case in ((2, 8, 16, 7, 9, 1), (2, 3, 32, 12, 10, 2)):
        g = J.geo("c3", case)
        dw = J.truth("c3", case, "bf16", "ones")["dw"]
        for ky in range(3):
            for kx in range(3):
                rows = sum(1 for oy in range(g.ho) if 0 <= oy * g.stride - 1 + ky < g.h)
                cols = sum(1 for ox in range(g.wo) if 0 <= ox * g.stride - 1 + kx < g.w)
                assert torch.equal(dw[:, :, ky, kx], torch.full((g.cout, g.cin), float(g.n * rows * cols), dtype=torch.float64))
    case = (2, 16, 40, 1, 7)
    g, tr = J.geo("pw", case), J.truth("pw", case, "bf16", "onehot")
    x, w, _, _ = tr["ops"]
    n, co, oy, ox = J.onehot_position(g)
    assert torch.equal(tr["dw"][co, :, 0, 0], J.ONE_HOT * x[n, :, oy, ox].double()) and float(tr["dw"].abs().sum()) > 0
    assert torch.equal(tr["dx"][n, :, oy, ox], J.ONE_HOT * w[co, :, 0, 0].double())
    assert int((tr["dw"] != 0).any(1).sum()) == 1 and int((tr["dx"] != 0).any(1).sum()) <= 1


MUTATIONS = [
    ("drop_pixel", "pw", (2, 16, 40, 1, 7), "dW"), ("drop_pixel", "pw", (3, 32, 48, 23, 126), "dW"),
    ("drop_pixel", "c3", (1, 24, 24, 12, 11, 1), "dW"),
    ("drop_chunk", "pw", (1, 24, 48, 3, 43), "dW"), ("drop_chunk", "pw", (3, 40, 960, 1, 4355), "dW"),
    ("omit_split", "pw", (67, 8, 16, 1, 1), "dW"), ("omit_split", "pw", (3, 32, 48, 23, 126), "dW"),
    ("double_split", "pw", (67, 8, 16, 1, 1), "dW"), ("double_split", "pw", (2, 64, 64, 13, 10), "dW"),
    ("transpose", "pw", (2, 64, 64, 13, 10), "dW"),
    ("swap_tap", "c3", (2, 8, 16, 7, 9, 1), "y"), ("parity", "c3", (2, 3, 32, 12, 10, 2), "y"), ("border", "c3", (2, 8, 16, 8, 8, 1), "y"),
    ("mix_fold", "c3", (8, 16, 40, 9, 6, 2), "dW"),
    ("sumsq_rounded", "pw", (2, 8, 32, 2, 5), "sumsq"),
    ("idle_garbage", "pw", (1, 8, 8, 1, 1), "sum"), ("idle_garbage", "pw", (2, 40, 24, 9, 15), "sum"),
]


@pytest.mark.parametrize("dtype_name", J.DTYPE_NAMES)
@pytest.mark.parametrize("mut,kind,case,check", MUTATIONS, ids=lambda v: J.sid(v) if isinstance(v, tuple) else str(v))
def test_a_mutation_of_one_pass_fails_its_check(mut, kind, case, check, dtype_name):
    assert not _run(kind, case, dtype_name, "random")["failures"]
    rec = _run(kind, case, dtype_name, "random", (mut,))
    assert check in _failed(rec), (mut, rec["failures"], rec["lines"])
    if mut in ("drop_pixel", "drop_chunk", "omit_split", "double_split", "transpose", "mix_fold"):  # one pass: nothing else moves
        assert _failed(rec) == ["dW"], rec["failures"]
    if mut == "sumsq_rounded":
        assert _failed(rec) == ["sumsq"], rec["failures"]
    # the exact family tells as well (the pixel a ternary case drops may hold a zero: the all-ones case cannot miss it)
    variant = "ones" if mut in ("drop_pixel", "drop_chunk", "omit_split", "double_split") else "ternary"
    if mut != "sumsq_rounded":  # (integers up to 256 are their own rounding)
        assert _failed(_run(kind, case, dtype_name, variant, (mut,))), mut


@pytest.mark.parametrize("dtype_name", J.DTYPE_NAMES)
def test_a_partial_rounded_to_bf16_passes_the_mass_bar_and_fails_the_exact_family(dtype_name):
    """what each family is for: the first of 65 splits' partials rounded to bf16 before the reduce moves an element by 2^-9 of ONE
    split's sum of 256 pixels, which the mass bar (a rounding per added pixel of all 16 143) lets through.  Integer operands tell:
    all ones with the first pixel of every image doubled make that partial 257 -- nine significant bits -- and bit equality fails.
    (Plain all-ones partials of a 1x1 layer are multiples of 128, which bf16 holds.)"""
    kind, case = "pw", (3, 256, 256, 1, 5381)
    rec = _run(kind, case, dtype_name, "random", ("bf16_partial",))
    print("\n".join(rec["lines"]))
    assert not rec["failures"], rec["failures"]
    g = J.geo(kind, case)
    plan = J.plan_of(g)
    assert plan["wgrad"][0][2] == 65
    x, w, bias, dy = J.exact_operands(kind, case, dtype_name, "ones")
    x = x.clone()
    x[:, :, 0, 0] = 2
    tr = J._truth(g, x, w, bias, dy, masses=("y", "dx"))
    assert not J.exact_conditions(g, tr, dtype_name)
    assert float(tr["dw"].min()) == float(tr["dw"].max()) == 3 * 5381 + 3
    for mut, want in (((), []), (("bf16_partial",), ["dW"])):
        got = J.model(g, (x, w, bias, dy), dtype_name, plan, mut)
        assert _failed(J.judge_exact(J.new_rec("doubled first pixel"), got, tr, dtype_name)) == want, mut
