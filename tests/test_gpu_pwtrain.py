"""The 1x1 training kernels (csrc/ssdk_pwtrain.hip, ssdk_pwtrain_kernels.h) and their direct users on the GPU, per element against
``F.conv2d`` autograd in fp64 on the CPU: the 1x1 layers (forward, input gradient, weight gradient, the statistics hand-over), the 3x3
layers that run as im2col / col2im around the same kernels (plain and folded), and the loc | conf pair of an SSD level.  Operands,
truth, bars, case lists and checks are tests/pwjudge.py; tests/test_pwjudge_cpu.py shows that judge failing on mutations of a model.

Every layer runs under autocast on fp32 master parameters that hold 16-bit values -- the product path: ssdk_pw_prepare, an fp32 dW
that nobody rounds -- in two families: random operands against derived bars, and integer operands (ternary, all ones, one-hot dy)
whose every partial sum is exact in any order, against ``torch.equal``.  The plan of each case (splits of the weight gradient,
rows of the statistics workspace, fold decision) is recovered from the public workspace queries and must be the listed one; the
kernel names are asserted wherever ssdk_last_kernel can tell (the entry points on the test thread, bit-equal to the layer).  The
guard-band tests call the C-ABI entry points on views between 0xFF (NaN) guards: nothing outside is touched, nothing depends on
what the workspace held, and element-aligned tensors give the bits of 16-byte aligned ones.

How loose the derived bars turned out: worst |err| / bar over all cases of one MI355X run (profiles/r26_pwjudge_ratios.jsonl, written
with PWJUDGE_RATIOS=<file>; the bars are the derived ones, not fitted to it), bf16 / fp16:
  y, dx (one store)        0.50 / 0.25   1x1 layers and head pair; the 4 eps rms term carries the small elements
  dx of NativeConv3x3      0.18 / 0.10   of the factor-3 bar
  dW                       0.016 / 0.015 and below: the mass bar allows a rounding per added pixel, the kernels' error is 60 - 200 x smaller
  sum y, sum y^2           0.013 / 0.016
  dbias of the pair        0.008 / 0.025
  ssdk_col2im3x3 alone     0.996 / 0.499 of its one-rounding bar (eps is the full relative half-ulp of bf16, twice that of fp16)
The mass bars are that loose by construction, which is what the exact family is for."""
import pytest

import pwjudge as J

pytestmark = pytest.mark.gpu
FAMILIES = ["random"] + list(J.VARIANTS)


def _settle(rec):
    print("\n".join(rec["lines"]))
    if rec["names"] is not None:
        print("%s: kernels %s" % (rec["what"], rec["names"]))
    if rec["plan"] is not None:
        print("%s: plan %s" % (rec["what"], rec["plan"]))
    J.log_ratios(rec)
    assert not rec["failures"], "%s: %s" % (rec["what"], rec["failures"])
    return rec


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("dtype_name", J.DTYPE_NAMES)
@pytest.mark.parametrize("case", list(J.PW), ids=J.sid)
def test_pointwise_layer(case, dtype_name, family):
    """y, dx, dW and both statistics of a 1x1 layer; splits, statistics rows and the three kernel names as listed"""
    rec = _settle(J.check_case("pw", case, dtype_name, family))
    splits, fwd, dxk, rows = J.PW[case]
    assert rec["plan"]["wgrad"][0][2] == splits and rec["names"] == [fwd, dxk, J.REDUCE]
    assert rows is None or rec["plan"]["rows"] == rows
    if family == "random":
        assert set(rec["ratios"]) == {"y", "dx", "dW", "sum", "sumsq"}


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("dtype_name", J.DTYPE_NAMES)
@pytest.mark.parametrize("case", list(J.C3), ids=J.sid)
def test_native_conv3x3_layer(case, dtype_name, family):
    """y, dx (three 16-bit roundings: see pwjudge.dx_factor) and dW of a 3x3 layer on im2col + the 1x1 kernels + col2im"""
    rec = _settle(J.check_case("c3", case, dtype_name, family))
    assert rec["plan"]["fold"] == J.C3[case]
    if family == "random":
        assert set(rec["ratios"]) == {"y", "dx", "dW"}


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("dtype_name", J.DTYPE_NAMES)
@pytest.mark.parametrize("case", list(J.HEAD), ids=J.sid)
def test_head_pair(case, dtype_name, family):
    """both outputs and dx per element, both dweights against the mass bar of the ssdk_pw_wgrad call _weight_gradients makes
    (folded or not), dbias against 16 u sum|dy|"""
    rec = _settle(J.check_case("head", case, dtype_name, family))
    assert rec["plan"]["fold"] == J.HEAD[case] and len(rec["plan"]["wgrad"]) == 2
    if family == "random":
        assert set(rec["ratios"]) == {"y", "dx", "dW", "dbias"}


@pytest.mark.parametrize("dtype_name", J.DTYPE_NAMES)
@pytest.mark.parametrize("case", J.GUARD_PW, ids=J.sid)
def test_pointwise_entry_points_between_guards(case, dtype_name):
    """ssdk_pw_forward (y, dx), ssdk_pw_forward_stats and ssdk_pw_wgrad: inputs bit-identical afterwards, guards intact, no NaN in any
    output; the same bits with the workspaces pre-filled with 0xFF (a partial row nobody wrote would surface) and with x / dy / y /
    dx at element offsets 1 and 3 into their allocations"""
    base_rec, base = J.guard_pw(case, dtype_name, 0, 0)
    _settle(base_rec)
    for off, fill in ((0, 0xFF), (1, 0), (3, 0xFF)):
        rec, outs = J.guard_pw(case, dtype_name, off, fill)
        J.same_results(rec, base, outs, "offset %d, workspace 0x%02x" % (off, fill))
        _settle(rec)


@pytest.mark.parametrize("fold", [False, True], ids=["plain", "folded"])
@pytest.mark.parametrize("dtype_name", J.DTYPE_NAMES)
@pytest.mark.parametrize("case", J.GUARD_C3, ids=J.sid)
def test_im2col_col2im_entry_points_between_guards(case, dtype_name, fold):
    """ssdk_im2col3x3 / ssdk_col2im3x3 and the two _folded: col is the definition's copy bit for bit (zero rows Kp - 9 C included),
    dx the fp64 gather of the same 16-bit terms to one rounding; guards intact, inputs unchanged, no NaN, the same bits at element
    offsets 1 and 3"""
    base_rec, base = J.guard_c3(case, dtype_name, 0, fold)
    _settle(base_rec)
    for off in (1, 3):
        rec, outs = J.guard_c3(case, dtype_name, off, fold)
        J.same_results(rec, base, outs, "offset %d" % off)
        _settle(rec)
