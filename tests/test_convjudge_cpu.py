"""The judge of the inference convolutions (tests/convjudge.py) on the CPU: it must be able to fail.  An fp32 model of the layer -- partial
sums per tap and 32-channel chunk added in index order, the slabs of a split summed separately, the epilogue of the numerical model -- passes
the judge on EVERY row of the table, in both families and both dtypes; each mutation is rejected, and the test says by which family (the
mutation sweep runs on the rows up to convjudge.CPU_MACS: ten mutations x five families x two dtypes per row).  The operand conditions of
the exact family are asserted for every row and variant (they are computed, not measured), the short cuts the truth takes on the
structured variants are held against the plain contraction, and the weights the truth reads from the pack are held against the weights
the case generated.

Which family rejects which mutation (printed by test_every_mutation_is_rejected; the sets below are asserted):
  ONLY the random family  round_partials -- partial sums of mass <= 256 ARE 16-bit values, so by construction the exact family cannot see a
                          rounding of them.
  both                    everything else, at the level of a CASE -- drop_product and slab_twice included, at every K.  drop_product is ONE
                          product (the centre tap of the last input channel) lost in every output of the right border column: less than
                          the whole tap of all Cin channels that a kernel would typically lose there, the smallest fault of the kind.  It
                          touches a whole column, and among thousands of touched elements some carry a large product under a small output;
                          per ELEMENT at K >= 512 the random family sees between a quarter and three quarters of the elements a dropped
                          product or a doubled slab touched (relu hides more), the exact family every one whose product is not zero --
                          test_the_random_family_sees_a_share_of_a_dropped_product.  A kernel that loses the product at ONE pixel passes
                          the random family about every second time."""
import pytest
import torch

import convjudge as J

CPU = [c.name for c in J.cpu_cases()]
RANDOM_ONLY = {"round_partials"}


def test_the_case_table_is_well_formed():
    kernels = {J.GEMM, J.WAVE, J.G256, J.GEMMP, J.PWFLOW, J.HALO, J.SHORT, J.SMALLMAP, J.FIRST, J.DW}
    assert {c.kernel for c in J.CASES} == kernels
    for c in J.CASES:
        assert c.kernel in kernels and isinstance(c.variant, str) and c.variant and " | " not in c.variant, c.name
        assert c.variant.split()[0] == {J.GEMM: "gemm", J.WAVE: "wave", J.G256: "gemm256", J.GEMMP: "gemmp", J.PWFLOW: "pwflow", J.HALO: "halo",
                                        J.SHORT: "short", J.SMALLMAP: "smallmap", J.FIRST: "first", J.DW: "dw"}[c.kernel], c.name
        assert c.act in ("none", "relu", "relu6", "silu", "sigmoid") and c.rmode in J.RES_MODE and c.kind in ("dense", "stem", "dw")
        assert (c.split is None) == (c.act2 is None) and (c.split is None or c.nchw) and not (c.nchw and c.rmode), c.name
        assert c.rmode != "post" or c.act in J.CLAMPS, c.name
        assert ("split" in c.variant.split()) == (c.splits > 1) or c.kernel not in (J.GEMM, J.WAVE, J.HALO), c.name
        assert J.macs(c) <= 11e9, (c.name, J.macs(c))  # the fp64 truth stays cheap (the largest: four 8x8 maps per halo tile, 384 -> 504)
        ho, wo = J.out_hw(c)
        assert c.rmode != "half" or (ho % 2 == 0 and wo % 2 == 0), c.name
        spots, runs = J.onehot_x_spots(c), J.onehot_x_positions(c)
        assert len(set(spots)) == len(spots) and {s[0] for s in spots} >= {c.cin - 1, min(31, c.cin - 1), min(32, c.cin - 1)}
        assert {s[1:] for s in spots} >= {(0, 0), (0, c.w - 1), (c.h - 1, 0), (c.h - 1, c.w - 1)}
        assert sorted(p[1:] for run in runs for p in run) == sorted(spots) and all(run[0][0] == c.n - 1 for run in runs)
        assert all(len({p[0] for p in run}) == len(run) for run in runs)  # one hot element per image
    # every kernel has rows the CPU model runs on or shares its arithmetic with one that does; the model's rows cover every residual
    # mode, both layouts' split heads, a split, every activation and every kind
    cpu = J.cpu_cases()
    assert {c.rmode for c in cpu} == {None, "same", "half", "post"} and any(c.split for c in cpu) and any(c.splits > 1 for c in cpu)
    assert {c.act for c in cpu} == {"none", "relu", "relu6", "silu", "sigmoid"} and {c.kind for c in cpu} == {"dense", "stem", "dw"}
    assert len(J.SPLIT_CASES) >= 8


def test_the_silu_constant_and_the_activation_error():
    v = torch.linspace(-20, 20, 400001, dtype=torch.float64)
    s = torch.sigmoid(v)
    slope = (s * (1 + v * (1 - s))).abs().max()
    assert 1.0998 < float(slope) <= J.SILU_L
    assert float((s * (1 - s)).max()) <= 0.25
    # the model's fp32 sigmoid / silu stay inside A(v) against fp64 (torch's exp2 and division are correctly rounded or 1 ulp)
    v32 = torch.linspace(-30, 30, 200001)
    for act in ("sigmoid", "silu"):
        want = J.act64(v32.double(), act)
        err = (J.act32(v32, act).double() - want).abs()
        assert bool((err <= J.act_error(v32.double(), want, act) + 1e-45).all()), act


@pytest.mark.parametrize("name", ["gemm_bn64", "gemm_split_res", "wave_split", "sm_3x5", "sm_s2_2x2", "first_16_nchw", "dw_8_s2"])
def test_the_structured_truths_are_the_plain_contraction(name):
    """conv64's short cuts for ones / onehot_x / onehot_w against im2col + matmul on the same operands"""
    c = J.BY_NAME[name]
    for variant in ("ones", "onehot_x", "onehot_w"):
        for pos in range(len(J.onehot_x_positions(c)) if variant == "onehot_x" else 1):
            ops = J.exact_operands(c, "bf16", variant, pos)
            x, w = ops.x.double(), J.pack_weight(c, ops.pack)
            assert torch.equal(J.conv64(c, x, w, ops.hint), J.conv64(c, x, w, None)), (variant, pos)
            assert torch.equal(J.conv64(c, x.abs(), w.abs(), ops.hint), J.conv64(c, x.abs(), w.abs(), None)), (variant, pos)


@pytest.mark.parametrize("name", [c.name for c in J.CASES])
def test_the_exact_conditions_hold(name):
    """every case and variant, both dtypes (one dtype for the rows above 1 GMAC: the operands differ by their seed only)"""
    c = J.BY_NAME[name]
    for dtype_name in J.DTYPE_NAMES if J.macs(c) <= 1.0e9 else J.DTYPE_NAMES[J.CASES.index(c) % 2:][:1]:
        for variant in J.VARIANTS:
            for pos in range(len(J.onehot_x_positions(c)) if variant == "onehot_x" else 1):
                tr = J.truth(name, dtype_name, variant, pos)
                bad = J.exact_conditions(c, tr, dtype_name)
                assert not bad, (dtype_name, variant, pos, bad)
                if tr["ops"].pack.scale is not None and variant == "ternary":
                    assert set(tr["ops"].pack.scale.abs().tolist()) == {0.5, 1.0, 2.0}


@pytest.mark.parametrize("name", [c.name for c in J.CASES if c.kind != "stem"])
def test_the_truth_reads_the_weights_the_case_generated(name):
    """the truth is built from the pack's own tensor (what the kernel reads): a wrong permutation inside ConvPack would be mirrored in
    it, so the tensor is held against the generated weights once, for the dense and depthwise rows (the stem's pack holds the product
    of the weights and the folded scale: below)"""
    c = J.BY_NAME[name]
    for ops in (J.operands(c, "bf16"), J.exact_operands(c, "f16", "ternary"), J.exact_operands(c, "bf16", "onehot_w")):
        assert tuple(ops.w.shape) == (c.cout, 1 if c.kind == "dw" else c.cin, c.k, c.k)
        assert torch.equal(J.pack_weight(c, ops.pack), ops.w.double())


def test_the_stem_pack_holds_the_scaled_weights():
    from ssds.modeling.layers import fused_conv as FC

    for c in (r for r in J.CASES if r.kind == "stem"):
        ops = J.exact_operands(c, "bf16", "ternary")
        assert ops.pack.scale is None and torch.equal(J.pack_weight(c, ops.pack), ops.w.double())  # (no BatchNorm: scale 1)
        ops = J.operands(c, "f16")
        if c.bn:  # fp32 w * gamma / sqrt(var + eps), one rounding: recomputed here from the BatchNorm the case drew
            gen = J._gen(c, "f16", 1)
            torch.randn(c.n, c.cin, c.h, c.w, generator=gen), torch.randn(ops.w.shape, generator=gen)
            mean, var = torch.randn(c.cout, generator=gen) * 0.2, torch.rand(c.cout, generator=gen) + 0.5
            gamma = torch.rand(c.cout, generator=gen) + 0.5
            scale = gamma / torch.sqrt(var + 1e-5)
            assert torch.equal(J.pack_weight(c, ops.pack), (ops.w * scale.view(-1, 1, 1, 1)).double())
            assert FC.conv_kind(J._module(c, ops.w, None)) == "stem"


@pytest.mark.parametrize("dtype_name", J.DTYPE_NAMES)
@pytest.mark.parametrize("name", [c.name for c in J.CASES])
def test_the_model_passes_the_judge(name, dtype_name):
    c = J.BY_NAME[name]
    rec = J.check_model(name, dtype_name, "random")
    print("\n".join(rec["lines"]))
    assert not rec["failures"], rec["failures"]
    for variant in J.VARIANTS:
        for pos in range(len(J.onehot_x_positions(c)) if variant == "onehot_x" else 1):
            rec = J.check_model(name, dtype_name, variant, (), pos)
            assert not rec["failures"], (variant, pos, rec["failures"])


def _rejections(mut, dtype_name):
    """-> ({family: [cases that reject]}, [cases where the exact family applies but every variant accepts])"""
    by, blind = {"random": [], "exact": []}, []
    for name in CPU:
        c = J.BY_NAME[name]
        if not J.applies(mut, c):
            continue
        if J.check_model(name, dtype_name, "random", (mut,))["failures"]:
            by["random"].append(name)
        if J.exact_applies(mut, c):
            hit = any(J.check_model(name, dtype_name, v, (mut,), pos)["failures"] for v in J.VARIANTS
                      for pos in range(len(J.onehot_x_positions(c)) if v == "onehot_x" else 1))
            (by["exact"] if hit else blind).append(name)
    return by, blind


@pytest.mark.parametrize("mut", J.MUTATIONS)
def test_every_mutation_is_rejected(mut):
    for dtype_name in J.DTYPE_NAMES:
        by, blind = _rejections(mut, dtype_name)
        print("%s %s: random rejects %s; exact rejects %s" % (mut, dtype_name, by["random"], by["exact"]))
        assert by["random"] or by["exact"], "accepted everywhere"
        # wherever the exact family applies to the mutation it catches it
        assert not blind, (mut, dtype_name, blind)
        if mut in RANDOM_ONLY:
            assert by["random"] and not by["exact"]
        else:
            assert by["random"] and by["exact"]


def test_the_random_family_sees_a_share_of_a_dropped_product():
    """one product lost in every element of the right border column: the share of those elements that leave the random family's bar at
    long K, against the exact family, which differs in every element whose lost product is not zero"""
    import re

    seen = []
    for name in CPU:
        c = J.BY_NAME[name]
        if c.kind != "dense" or J.terms(c) < 512 or c.rmode or c.split or c.act not in J.CLAMPS or c.h * c.w == 1:  # (a 1x1 map: Cin real products)
            continue
        ho, _ = J.out_hw(c)
        for dtype_name in J.DTYPE_NAMES:
            rec = J.check_model(name, dtype_name, "random", ("drop_product",))
            out = int(re.match(r"y: (\d+) elements", rec["failures"][0]).group(1)) if rec["failures"] else 0
            share = out / float(c.n * c.cout * ho)
            print("%s %s K=%d: the random family sees %.3f of the touched elements" % (name, dtype_name, J.terms(c), share))
            assert share < 0.75, (name, dtype_name, share)
            seen.append(share)
            # ternary: got and want differ exactly where the lost product, seen through the activation, is not zero
            tr = J.truth(name, dtype_name, "ternary")
            good, bad = J.model(c, tr["ops"], dtype_name), J.model(c, tr["ops"], dtype_name, ("drop_product",))
            assert torch.equal(good, tr["y"].to(good.dtype)) and int((good != bad).sum()) > 0
            assert int((bad != tr["y"].to(bad.dtype)).sum()) == int((good != bad).sum())
    assert len(seen) >= 6


def test_the_judge_rejects_a_nan_and_a_wrong_dtype():
    name, dtype_name = "gemm_bn32", "f16"
    c = J.BY_NAME[name]
    tr = J.truth(name, dtype_name, "random")
    got = J.model(c, tr["ops"], dtype_name)
    got[0, 0, 0, 0] = float("nan")
    assert J.judge(J.new_rec("nan"), c, got, tr, dtype_name, 1)["failures"]
    assert J.judge(J.new_rec("dtype"), c, got.float(), tr, dtype_name, 1)["failures"]
    assert J.judge_exact(J.new_rec("dtype"), got.float(), J.truth(name, dtype_name, "ternary"), dtype_name)["failures"]


def test_the_variant_text_is_bound():
    """ssdk_last_variant comes through the derived binding (include/ssdk_variant.h) and answers with text; the judge's readers of it"""
    from ssds import _native as N

    assert N.VARIANT_EXPORTS == ("ssdk_last_variant",) and N.lib.ssdk_last_variant.argtypes == []
    assert isinstance(N.last_variant(), str) and "ssdk_last_variant" not in N.EXPORTS
    assert J.instance_of("gemmp remainder | grid=256 tq=1 tr=104") == "gemmp remainder" and J.instance_of("dw stride=2") == "dw stride=2"
    assert J.splits_of("halo first nhwc split | patch=2x10x10 ksplits=9") == 9 and J.splits_of("gemm bn=16 n64=0 resv=0 split | splits=2") == 2
    assert J.splits_of("gemm256 | tiles=128") == 1
