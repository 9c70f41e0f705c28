"""The judge of the depthwise training kernels (tests/dwjudge.py) on the CPU: an fp32 model of the three passes, rounded once to the
dtype, passes every bar on every case of both kernel families; single-element mutations of that model's result fail; the all-ones
predictions tell a missing image, row or column; the value set of the deferred-BatchNorm cases is exact in both 16-bit types; the
summation depths cover the test shapes."""
import pytest
import torch

import dwjudge as J

ALL_SHAPES = J.WHOLE_ROW + J.TILED_SWITCH + J.TILED_DISPATCH
BIG = (2, 4, 150, 150)


def _judged(got, tr, dtype_name, what="mutant"):
    return J.judge(J.new_rec(what), got, tr, dtype_name)


@pytest.mark.parametrize("dtype_name", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("stride", J.STRIDES)
@pytest.mark.parametrize("shape", ALL_SHAPES, ids=J.sid)
def test_fp32_model_passes_every_bar(shape, stride, dtype_name):
    x, wt, dy = J.operands(shape, stride, dtype_name)
    tr = J.truth(x, wt, dy, stride)
    rec = _judged(J.model(x, wt, dy, stride, dtype_name), tr, dtype_name, "model %s s%d %s" % (J.sid(shape), stride, dtype_name))
    print("\n".join(rec["lines"]))
    assert not rec["failures"], rec["failures"]
    assert set(rec["ratios"]) == {"y", "dx", "dW", "sum", "sumsq"}


def test_depths_are_derived_and_capped():
    """the named depths stay under the cap, and their one shape-dependent term -- the partial sums one lane of the second-stage
    reduction adds -- covers every shape of the tests, by the library's own plan"""
    sum_depth, stats_depth = J.depths()
    assert sum_depth <= J.DEPTH_CAP and stats_depth <= J.DEPTH_CAP
    for shape in ALL_SHAPES:
        for stride in J.STRIDES:
            for dt in ("f32", "bf16", "f16"):
                p = J.plan(2, shape, stride, dt)
                ho, wo = J.out_hw(shape[2], shape[3], stride)
                partials = p["groups"] if p else shape[0] * ((ho + 31) // 32) * ((wo + 63) // 64)
                if shape not in J.WHOLE_ROW:  # (the switch sends these to the tiles whatever the plan says)
                    partials = max(partials, shape[0] * ((ho + 31) // 32) * ((wo + 63) // 64))
                assert partials <= 4 * 64, (shape, stride, dt, partials)
                f = J.plan(0, shape, stride, dt)
                assert f is None or (f["G"] * f["UP"] <= 1024 and f["groups"] <= 4096)


@pytest.mark.parametrize("dtype_name", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("stride", J.STRIDES)
def test_mutations_of_the_model_fail(stride, dtype_name):
    x, wt, dy = J.operands(BIG, stride, dtype_name)
    tr = J.truth(x, wt, dy, stride)
    base = J.model(x, wt, dy, stride, dtype_name)
    assert not _judged(base, tr, dtype_name)["failures"]
    dtype = J.DTYPES[dtype_name]

    def mutant(**kw):
        got = {k: v.clone() for k, v in base.items()}
        got.update(kw)
        return _judged(got, tr, dtype_name)

    # one border tap (2, 2) dropped at one pixel of the first row of y
    prod = (wt[0, 0, 2, 2].double() * x[0, 0, 1, 1::stride].double()[:tr["y"].shape[3] - 1]).detach()
    ox = int(prod.abs().argmax())
    y = base["y"].clone()
    y[0, 0, 0, ox] = (tr["y"][0, 0, 0, ox] - prod[ox]).to(dtype)
    assert abs(float(prod[ox])) > 0
    rec = mutant(y=y)
    assert [f for f in rec["failures"] if f.startswith("y:")] and len(rec["failures"]) == 1, rec["failures"]
    # one row of dx shifted by one pixel
    dx = base["dx"].clone()
    dx[1, 2, 75] = torch.roll(dx[1, 2, 75], 1)
    rec = mutant(dx=dx)
    assert [f for f in rec["failures"] if f.startswith("dx:")] and len(rec["failures"]) == 1, rec["failures"]
    # one product of typical size removed from one dW[c, t]: 1 of the 45 000 (stride 1) that make up the tap
    c, ky, kx = 3, 0, 2
    ho, wo = tr["y"].shape[2:]
    xp = torch.nn.functional.pad(x.double(), (1, 1, 1, 1))
    win = xp[:, c, ky:ky + stride * (ho - 1) + 1:stride, kx:kx + stride * (wo - 1) + 1:stride] * dy[:, c].double()
    assert abs(float(win.sum()) - float(tr["dw"][c, 0, ky, kx])) <= 1e-9 * float(tr["Mw"][c, 0, ky, kx])
    pick = int((win.abs() - win.abs().mean()).abs().argmin())
    dw = base["dw"].clone()
    dw[c, 0, ky, kx] -= float(win.reshape(-1)[pick])
    rec = mutant(dw=dw)
    assert [f for f in rec["failures"] if f.startswith("dW:")] and len(rec["failures"]) == 1, rec["failures"]
    # one output row left out of the statistics of one channel
    sums = base["sums"].clone()
    row = tr["y"][1, 2, ho // 2]
    sums[2, 0] -= float(row.sum())
    sums[2, 1] -= float(row.pow(2).sum())
    rec = mutant(sums=sums)
    assert any(f.startswith("sumsq:") for f in rec["failures"]), rec["failures"]
    assert all(f.startswith("sum") for f in rec["failures"]), rec["failures"]
    # one channel's dW scaled by 1.01
    dw = base["dw"].clone()
    dw[1] *= 1.01
    rec = mutant(dw=dw)
    assert [f for f in rec["failures"] if f.startswith("dW:")] and len(rec["failures"]) == 1, rec["failures"]


@pytest.mark.parametrize("stride", J.STRIDES)
@pytest.mark.parametrize("shape", J.ONES["whole"] + J.ONES["tiled"], ids=J.sid)
def test_all_ones_counts_tell_a_missing_image_row_or_column(shape, stride):
    """x = w = dy = 1: every tap of dW and both statistics are counts below 2^24 that change when one image, one row or one column
    of the input is left out -- a kernel that skips one cannot equal the truth"""
    n, c, h, w = shape
    ho, wo = J.out_hw(h, w, stride)
    x, wt = torch.ones(shape), torch.ones(c, 1, 3, 3)
    full = J.truth(x, wt, torch.ones(n, c, ho, wo), stride)
    assert float(full["dw"].max()) < 2 ** 24 and float(full["sums"].max()) < 2 ** 24
    for k in ("y", "dx", "dw", "sums"):
        assert torch.equal(full[k], full[k].round()), k
    assert int(full["y"].min()) == 4 and int(full["y"].max()) == 9
    cuts = [(slice(n - 1, n), slice(None), slice(None)), (slice(None), slice(0, 1), slice(None)), (slice(None), slice(ho - 1, ho), slice(None)),
            (slice(None), slice(ho // 2, ho // 2 + 1), slice(None)), (slice(None), slice(None), slice(0, 1)),
            (slice(None), slice(None), slice(wo - 1, wo)), (slice(None), slice(None), slice(wo // 2, wo // 2 + 1))]
    for ni, ri, qi in cuts:  # the outputs of one image / row / column never summed
        dy = torch.ones(n, c, ho, wo)
        dy[ni, :, ri, qi] = 0
        part = J.truth(x, wt, dy, stride)
        assert bool((part["dw"] != full["dw"]).reshape(c, 9).any(1).all()), (ni, ri, qi)
        assert bool((part["dx"] != full["dx"]).any()), (ni, ri, qi)
        kept = full["y"] * dy
        sums = torch.stack([kept.sum((0, 2, 3)), kept.pow(2).sum((0, 2, 3))], 1)
        assert bool((sums != full["sums"]).all()), (ni, ri, qi)


@pytest.mark.parametrize("dtype_name", ["bf16", "f16"])
def test_affine_value_set_is_exact(dtype_name):
    dtype = J.DTYPES[dtype_name]
    v = J.affine_value_set()
    assert v.numel() == 65 * 3 * 33 and float(v.min()) == -9.0 and float(v.max()) == 11.0
    for act in J.ACTS:
        a = J.apply_act(v, act)
        assert torch.equal(a.to(dtype).double(), a), act
    for shape in J.AFFINE:
        x, coef, staged, _, _ = J.affine_operands(shape, 1, dtype_name, 0)
        assert torch.equal(x.double() * 8, (x.double() * 8).round()) and float(x.abs().max()) <= 4
        assert bool((coef[:, 1] > 0).any()) and bool((coef[:, 1] < 0).any())
        assert set(coef[:, 0].tolist()) <= {0.5, 1.0, 2.0} and torch.equal(coef[:, 1] * 8, (coef[:, 1] * 8).round())
        assert torch.equal(staged.to(dtype).double(), staged)


def test_one_hot_truth_is_the_convolution():
    """the written-out one-hot expectation equals fp64 autograd on the same one-hot gradient, rounded once"""
    for stride in J.STRIDES:
        shape = (2, 3, 8, 17)
        x, wt, dy = J.operands(shape, stride, "bf16")
        for pos in J.seam_positions(shape, stride, "bf16", "whole"):
            g = torch.zeros_like(dy)
            g[pos] = J.ONE_HOT
            tr = J.truth(x, wt, g, stride)
            dx, dw = J.one_hot_truth(x, wt, pos, stride, "bf16")
            assert torch.equal(dw.double(), tr["dw"]) and torch.equal(dx.double(), tr["dx"].to(torch.bfloat16).double()), pos


def test_seam_positions_sit_on_both_sides_of_the_plans_seams():
    shape, stride = (2, 4, 150, 150), 1
    p = J.plan(0, shape, stride, "bf16")
    assert p["T"] > 1
    rows = {pos[2] for pos in J.seam_positions(shape, stride, "bf16", "whole")}
    assert {p["TR"] - 1, p["TR"]} <= rows
    shape = (27, 4, 19, 19)
    p = J.plan(2, shape, stride, "bf16")
    assert 1 < p["G"] < 27
    imgs = {pos[0] for pos in J.seam_positions(shape, stride, "bf16", "whole")}
    assert {p["G"] - 1, p["G"]} <= imgs
    cols = {pos[3] for pos in J.seam_positions((1, 2, 70, 130), 1, "bf16", "tiled")}
    rows = {pos[2] for pos in J.seam_positions((1, 2, 70, 130), 1, "bf16", "tiled")}
    assert {63, 64, 127, 128} <= cols and {31, 32, 63, 64} <= rows
