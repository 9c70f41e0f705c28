"""tests/lossjudge.py turned on itself, on the CPU: the preconditions of every case hold, the fp32 model of the documented closed forms
passes every bar (so the bars are reachable in fp32), every mutation of it fails, and torch's own fp32 FocalLoss gradient fails the
saturated family -- which is why fp64 is the truth."""
import pytest

import lossjudge as J


@pytest.mark.parametrize("case", J.ALL_CASES, ids=J.cid)
def test_the_model_passes_every_check(case):
    J.preconditions(case)
    ops = J.operands(case)
    problems = J.judge(case, ops, J.model(case, ops))
    assert not problems, "\n".join(problems)


def test_the_case_list_reaches_what_it_claims():
    geos = {c.geo for c in J.ALL_CASES}
    assert geos == set(range(J.N_GEOS))
    assert J.rows_of(7) == 260 and J.rows_of(5) == 2 and J.rows_of(6) == 6
    assert {c.dtype for c in J.FOCAL_CASES} == {"bf16", "f16", "f32"}
    assert {c.family for c in J.FOCAL_CASES} == {"prior", "centred", "saturated", "ties"}
    for kind in J.LOC_KINDS:
        assert {c.dtype for c in J.FOCAL_CASES if c.loc_loss == kind and c.spread == 0.3} == {"bf16", "f16", "f32"}
        assert sum(1 for c in J.FOCAL_CASES if c.loc_loss == kind and c.spread == 1.5) == 1
    # the mining thresholds of the ``ties`` cases fall inside tie groups that span several 1024-key chunks of mine_select_kernel
    case = J.MUTATIONS["ties_desc"]
    ops = J.operands(case)
    hard, mined = J.hardness(case, ops), J.model(case, ops)
    import torch
    got = (mined.gc.view(2, 6, 7, 20, 24) != 0).any(2) & (ops.asg.depth == 0)
    thr = hard[0][got[0].reshape(-1)].min()
    tied = torch.nonzero(hard[0] == thr).reshape(-1)
    assert int(tied.min()) // 1024 != int(tied.max()) // 1024 and 0 < int(got[0].reshape(-1)[tied].sum()) < tied.numel()


@pytest.mark.parametrize("mutation", sorted(J.MUTATIONS))
def test_a_mutation_of_the_model_fails(mutation):
    case = J.MUTATIONS[mutation]
    ops = J.operands(case)
    assert not J.judge(case, ops, J.model(case, ops))
    problems = J.judge(case, ops, J.model(case, ops, mutate=mutation))
    assert problems, "the judge accepts the mutation %s" % mutation


@pytest.mark.parametrize("dtype", ["bf16", "f32"])  # (in fp16 the gradients of saturated logits lie below the flush threshold)
def test_the_fp32_torch_focal_gradient_fails_the_saturated_family(dtype):
    case = J._case(0, dtype=dtype, family="saturated")
    ops = J.operands(case)
    assert not J.judge(case, ops, J.model(case, ops))
    problems = J.judge(case, ops, J.torch_focal_fp32(case, ops))
    assert any(p.startswith("d_conf") for p in problems), problems
    # ... and passes where the existing tests look: logits centred on zero, fp32, under the bar of tests/test_gpu_train.py
    centred = J._case(0, dtype="f32", family="centred")
    ops = J.operands(centred)
    got = J.torch_focal_fp32(centred, ops).gc.double()
    want = J.scale_of(ops.asg) * J.truth(centred, ops).d_conf.reshape(got.shape)
    assert float(((got - want).abs() - 1e-5 * want.abs()).max()) <= 1e-5
