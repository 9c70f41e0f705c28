"""The inference convolutions behind ``ssdk_conv`` on the device under the judge of tests/convjudge.py (its docstring states the numerical
model, the fp64 truth, every bar with its derivation and the exact family).  Per case x dtype the dispatch (``last_kernel``) and the template
instance (``last_variant``, include/ssdk_variant.h) are asserted first; then the random family against the bars and the exact family --
ternary, ones, one-hot input at every listed position, one-hot weight -- bit for bit.  A closing test holds the table against INSTANCES, the
hand-written list of the launchers' instances; a wrong-truth check proves the device path of the judge can fail; every split-K case runs
twice and must repeat its bits.  CONVJUDGE_RATIOS=<file> keeps the worst |err| / bar per case, dtype and family.

DURATIONS.  A row's random family (with the split re-run) and its exact family are two tests, so that none takes more than a few seconds:
on one MI355X box with 16 CPU threads the slowest are test_conv_case_exact[g256_ragged] 2.4 s, [g256_c194] 2.1 s, [gemmp_rem] 1.8 s (the
fp64 contraction of the ternary variant on the CPU), every test_conv_case below 1.3 s."""
import pytest
import torch

import convjudge as J

pytestmark = pytest.mark.gpu

# The instances the table must reach, written by hand from the launchers' branches (the part of ssdk_last_variant() before " | ").
INSTANCES = {
    # csrc/ssdk_conv.hip launch_gemm: `if (n64) SSDK_GEMM(4, 1, 2, 4, ..); else if (p.Cout > 64) SSDK_GEMM(2, 2, 4, 4, ..); else if (p.Cout > 32)
    # SSDK_GEMM(4, 1, 2, 4, ..); else if (p.Cout > 16) SSDK_GEMM(4, 1, 2, 2, 1); else SSDK_GEMM(4, 1, 2, 1, 1);` and inside SSDK_GEMM
    # `if (gz > 1) <.., true>; else if (resv) <.., false, true>; else <.., false>` -- n64 needs gz == 1, resv needs Cout > 32: twelve in all
    "gemm bn=128 n64=0 resv=0 unsplit", "gemm bn=64 n64=1 resv=0 unsplit", "gemm bn=64 n64=0 resv=0 unsplit", "gemm bn=32 n64=0 resv=0 unsplit",
    "gemm bn=16 n64=0 resv=0 unsplit", "gemm bn=128 n64=0 resv=1 unsplit", "gemm bn=64 n64=1 resv=1 unsplit", "gemm bn=64 n64=0 resv=1 unsplit",
    "gemm bn=128 n64=0 resv=0 split", "gemm bn=64 n64=0 resv=0 split", "gemm bn=32 n64=0 resv=0 split", "gemm bn=16 n64=0 resv=0 split",
    # ssdk_conv: `p.ksplits = ws;` from wave_plan (`s = min(768 / tiles, KT / 4, 16)`), one kernel, split at run time
    "wave split", "wave unsplit",
    # launch_gemm256: one instance per dtype
    "gemm256",
    # csrc/ssdk_gemmp.hip: `gp.tq = tiles / grid; gp.tr = tiles % grid;` -- the first tr workgroups walk one tile more
    "gemmp even", "gemmp remainder",
    # csrc/ssdk_pwflow.hip: `ksi = ks <= 2 ? 2 : (ks <= 4 ? 4 : 8)` (8 needs Cin > 128: SSDK_PWFLOW=2 only) and `nf = 16; while (nf > 4 &&
    # Cout % (16 nf)) nf >>= 1;`
    "pwflow ks=2 nf=4", "pwflow ks=2 nf=8", "pwflow ks=2 nf=16", "pwflow ks=4 nf=4", "pwflow ks=4 nf=8", "pwflow ks=4 nf=16",
    # csrc/ssdk_conv3x3.hip launch_conv3x3_halo: `if (persist && hp.ksplits == 1 && (nchw_out ? (tw % 4 == 0 && Wo % 4 == 0) : (tw % 4 == 0
    # && Cout % 4 == 0)) && ..) conv3x3_halop_kernel<DT, !nchw_out>` else conv3x3_halo_kernel<DT>, whose NCHW stores branch on
    # `hp.vec_nchw`.  ("first nchw unsplit vec_nchw=1" needs a 4-aligned map the persistent form refuses: > 4 GiB outputs only.)
    "halo persistent nhwc unsplit", "halo persistent nchw unsplit", "halo first nhwc unsplit", "halo first nchw unsplit vec_nchw=0",
    "halo first nhwc split", "halo first nchw split vec_nchw=0", "halo first nchw split vec_nchw=1",
    # csrc/ssdk_conv3x3s.hip: `SSDK_S3C: cs == 1 .. 4, else 8` x `SSDK_S3A: nchw && wide | nchw | nhwc` -- fifteen products of two
    # independent template arguments; the table reaches every value of each
    "short cs=1 nchw", "short cs=2 nhwc", "short cs=3 nchw-wide", "short cs=4 nhwc", "short cs=8 nhwc",
    # csrc/ssdk_smallmap.hip SSDK_SM: `if (s2) <CS, 4, 9, true, 2, 2>; else if (P == 1) SSDK_SM1(4, 1); else if (na == 2 && kw == 2)
    # SSDK_SMK2; else if (na == 2) ..(kw: SSDK_CONV_SMALLMAP_KW=1 only); else if (mfr == 8) SSDK_SM1(8, 9); else SSDK_SM1(4, 9);` with
    # SSDK_SM1 = packed | KRSC; mfr 8 is `big && na == 1`, and na == 1 on a big layer means KRSC.  (cs = Cin / 32 stands behind " | ".)
    "smallmap mfr=4 taps=9 packed=1 na=2 stride=2 kw=1", "smallmap mfr=4 taps=1 packed=1 na=1 stride=1 kw=1",
    "smallmap mfr=4 taps=1 packed=0 na=1 stride=1 kw=1", "smallmap mfr=4 taps=9 packed=1 na=2 stride=1 kw=2",
    "smallmap mfr=8 taps=9 packed=0 na=1 stride=1 kw=1", "smallmap mfr=4 taps=9 packed=1 na=1 stride=1 kw=1",
    "smallmap mfr=4 taps=9 packed=0 na=1 stride=1 kw=1",
    # ssdk_conv, stem: `SSDK_FIRST(DT, 16 | 32 | 64)`, `p.in_layout` read per load
    "first cout=16 nchw", "first cout=16 nhwc", "first cout=32 nchw", "first cout=32 nhwc", "first cout=64 nchw", "first cout=64 nhwc",
    # ssdk_conv, depthwise: `dwconv3x3_kernel<DT, 1 | 2>`
    "dw stride=1", "dw stride=2",
}
SMALLMAP_CS = {4, 8, 16}  # `if (cs == 4) .. else if (cs == 8) .. else SSDK_SM(DT, 16)`: every form's CS argument, behind " | "
REACHED = {}     # instance -> set of dtypes that reached it
REACHED_CS = {}  # conv_smallmap's cs -> set of dtypes
DONE = set()     # (case, dtype) whose dispatch was seen


def _note(c, dtype_name, kernel, variant):
    REACHED.setdefault(J.instance_of(variant), set()).add(dtype_name)
    if kernel == J.SMALLMAP:
        REACHED_CS.setdefault(int(variant.rsplit("cs=", 1)[1]), set()).add(dtype_name)
    DONE.add((c.name, dtype_name))


def _finish(rec):
    J.log_ratios(rec)
    for line in rec["lines"]:
        print(line)
    assert not rec["failures"], (rec["what"], rec["variant"], rec["failures"])


@pytest.mark.parametrize("dtype_name", J.DTYPE_NAMES)
@pytest.mark.parametrize("name", [c.name for c in J.CASES])
def test_conv_case(name, dtype_name):
    c = J.BY_NAME[name]
    rec, got = J.check_case(name, dtype_name, "random")
    _note(c, dtype_name, rec["kernel"], rec["variant"])
    print("%s %s: %s, %s" % (name, dtype_name, rec["kernel"], rec["variant"]))
    # the dispatch and the instance first
    assert rec["kernel"] == c.kernel, (rec["kernel"], rec["variant"])
    assert J.instance_of(rec["variant"]) == c.variant, rec["variant"]
    _finish(rec)
    if c.splits > 1:  # a split repeats its bits: the slabs are added in a fixed order, whoever arrives last
        assert J.splits_of(rec["variant"]) > 1, rec["variant"]
        again, _, _ = J.native(c, J.truth(name, dtype_name, "random")["ops"], dtype_name)
        assert torch.equal(got, again), "two runs of a split-K case differ"


@pytest.mark.parametrize("dtype_name", J.DTYPE_NAMES)
@pytest.mark.parametrize("name", [c.name for c in J.CASES])
def test_conv_case_exact(name, dtype_name):
    """the exact family of a row, a test of its own so that no test of this file takes more than a few seconds (DURATIONS in the module docstring)"""
    c = J.BY_NAME[name]
    for variant in J.VARIANTS:
        for pos in range(len(J.onehot_x_positions(c)) if variant == "onehot_x" else 1):
            rec, _ = J.check_case(name, dtype_name, variant, pos)
            # the dispatch and the instance first (check_case lists them first among the failures)
            assert rec["kernel"] == c.kernel and J.instance_of(rec["variant"]) == c.variant, (variant, rec["kernel"], rec["variant"])
            _finish(rec)


def test_a_truth_with_one_product_missing_fails_the_judge():
    """The device path of the judge can fail: ONE product at the last pixel of the last image is taken out of the TRUTH (not of the
    device's work), and the kernel's real output must then leave the bar (random family, K = 24: the product stands far above it) and
    differ from the exact family's truth."""
    name, dtype_name = "gemm_bn64", "bf16"
    c = J.BY_NAME[name]
    for family in ("random", "ternary"):
        tr = J.truth(name, dtype_name, family)
        got, kernel, variant = J.native(c, tr["ops"], dtype_name)
        assert kernel == c.kernel and J.instance_of(variant) == c.variant
        bad, prod = J.wrong_truth(tr, c)
        assert prod != 0.0
        honest, wrong = J.new_rec("honest"), J.new_rec("wrong truth")
        if family == "random":
            J.judge(honest, c, got, tr, dtype_name, 1)
            J.judge(wrong, c, got, bad, dtype_name, 1)
        else:
            J.judge_exact(honest, got, tr, dtype_name)
            J.judge_exact(wrong, got, bad, dtype_name)
        assert not honest["failures"], honest["failures"]
        assert len(wrong["failures"]) == 1 and ("1 elements" in wrong["failures"][0]), wrong["failures"]


def test_every_instance_is_reached_in_both_dtypes_and_nothing_else():
    """The table against INSTANCES.  Cases whose test ran before this one in the same process have left their instance in REACHED; any
    other (this test selected alone, another order) is dispatched here once more, so the test stands on its own."""
    for c in J.CASES:
        for dtype_name in J.DTYPE_NAMES:
            if (c.name, dtype_name) not in DONE:
                _, kernel, variant = J.native(c, J.operands(c, dtype_name), dtype_name)
                _note(c, dtype_name, kernel, variant)
    for inst in sorted(INSTANCES):
        print("%-60s %s" % (inst, sorted(REACHED.get(inst, ()))))
    missing = sorted(i for i in INSTANCES if REACHED.get(i, set()) != set(J.DTYPE_NAMES))
    unlisted = sorted(set(REACHED) - INSTANCES)
    assert not missing and not unlisted, (missing, unlisted)
    assert {cs for cs, d in REACHED_CS.items() if d == set(J.DTYPE_NAMES)} == SMALLMAP_CS, REACHED_CS
    assert {c.variant for c in J.CASES} == INSTANCES
