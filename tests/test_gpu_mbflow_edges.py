"""The register-flow block kernel (csrc/ssdk_mbflow.hip) on the cut of the map that csrc/ssdk_flow_plan.h plans: stride-1
strips whose first / last lane stores where it is column 0 / W - 1 (the DPP row shift hands such a lane 0 for its missing
neighbour, which is the zero padding), and row segments whose length comes from the row loop's step.

tests/test_gpu_conv.py compares the register-flow and the LDS-tiled kernel only within a tolerance, so the reference here is
the fp32 block with the intermediate tensors rounded to the model dtype, under that file's bar for these kernels (`_check`,
floor = 1), imported.  Every case runs with x and y between NaN guards (tests/guardband.py): nothing outside y may be written,
and every element of y must be.

Widths (stride 1): 15, 16 one strip (16: both edge lanes store); 17 a second strip that stores one column, in lane 3; 30 a last
strip whose lane 15 IS column W - 1; 31 one column more; 44 three strips (an interior one; 44 = 14 * 2 + 16: lane 15 again);
128 the bench's map, nine strips (the two-strip instance: an odd number, the last wave half empty).  Heights: 5 one short
segment, 18 several, 27 several and a remainder (forced launches cut segments of 4 - 6 rows)."""
import pytest

pytestmark = pytest.mark.gpu

HEIGHTS = (5, 18, 27)


def _run_guarded(x, pk, want, dtype, what):
    import torch
    import guardband as G
    from ssds import _native as N
    from ssds.modeling.layers import fused_conv as FC
    from test_gpu_conv import _check

    gs = G.GuardSet("cuda")
    gx = gs.inp("x", x)
    gy = gs.out("y", tuple(want.shape), dtype, torch.channels_last)
    gs.arm()
    got = FC.mbconv_native(gx, pk, variant=1, y=gy)
    torch.cuda.synchronize()
    name = N.last_kernel()
    assert "mbflow" in name, name
    assert got.data_ptr() == gy.data_ptr()
    assert gs.problems() == [], what
    assert not G.has_nan(got), "%s: an element of y was never written" % what
    _check(got, want, dtype, "%s (%s)" % (what, name), floor=1.0)
    return got


def _block(cin, cout, stride, dtype, seed, residual=None):
    import copy

    import torch
    from ssds.modeling.layers import fused_conv as FC
    from ssds.modeling.layers.planner import groups_of
    from ssds.modeling.nets.mobilenet import InvertedResidual
    from test_gpu_guard import _randomize

    torch.manual_seed(seed)
    blk = InvertedResidual(cin, cout, stride, 6).eval()
    _randomize(blk.modules(), dtype, 2.0)
    mods = list(copy.deepcopy(blk).conv.children())  # the reference stays on the CPU, in fp32
    chain = [mods[0], mods[1], torch.nn.Sequential(mods[2], mods[3])]
    res = blk.use_res_connect if residual is None else residual
    blk = blk.cuda()
    groups = groups_of(blk.conv)
    assert FC.MbPack.supported(groups, res)
    return chain, res, FC.MbPack(groups, res, dtype)


@pytest.mark.parametrize("dtype_name", ["bf16", "f16"])
@pytest.mark.parametrize("w", [15, 16, 17, 30, 31, 44, 128])
@pytest.mark.parametrize("cin", [24, 32])
def test_stride1_edge_strips(cin, w, dtype_name):
    """24 -> 144 -> 24 with the residual (one strip per wave, row pairs) and 32 -> 192 -> 32 without (two strips per wave).

    Why the second block runs without: with the residual the kernel rounds twice, bf16(bf16(block) + x), as torch's tensor add
    does, against a reference that rounds once, bf16(block) + x in fp32.  Where the first rounding falls the other way and the
    second meets a tie, the two differ by 1.5 ulp of the output; floor = 1 grants 2^-7 max|want| + 1e-3, which is fewer ulps
    than that while max|want| sits in the lower 47 % of its binade.  Measured on the residual form of this block at 5 x 17 in
    bf16: got 5.8125, want 5.859375 (a tie of two bf16 values, and the largest element), granted 0.04678, missed by 1e-4 --
    on an interior lane of strip 0, the same arithmetic on any cut of the map."""
    import torch
    from test_gpu_guard import _block_want, _cl

    dtype = torch.bfloat16 if dtype_name == "bf16" else torch.float16
    chain, res, pk = _block(cin, cin, 1, dtype, cin + w, residual=cin == 24)
    for h in HEIGHTS:
        x = torch.randn(2, cin, h, w).to(dtype)
        want = _block_want(chain, x, dtype, res)
        _run_guarded(_cl(x), pk, want, dtype, "%d->%d->%d s1 %dx%d %s" % (cin, 6 * cin, cin, h, w, dtype_name))


@pytest.mark.parametrize("dtype_name", ["bf16", "f16"])
@pytest.mark.parametrize("w", [30, 32])
def test_stride2_segments(w, dtype_name):
    """16 -> 96 -> 24, stride 2: the even / odd strip pairing is as it was, the segment length is new (odd: one surplus row)."""
    import torch
    from test_gpu_guard import _block_want, _cl

    dtype = torch.bfloat16 if dtype_name == "bf16" else torch.float16
    chain, res, pk = _block(16, 24, 2, dtype, 16 + w)
    assert not res
    for h in (18, 34):
        x = torch.randn(2, 16, h, w).to(dtype)
        want = _block_want(chain, x, dtype, res)
        _run_guarded(_cl(x), pk, want, dtype, "16->96->24 s2 %dx%d %s" % (h, w, dtype_name))


@pytest.mark.parametrize("dtype_name", ["bf16", "f16"])
def test_stem_block_segments(dtype_name):
    """3 -> 32 -> 16 from a 64 x 60 image: the stem instances keep their halo strips and their 8-row segments of a forced launch
    (the planned lengths measured no faster on this block), both now read from csrc/ssdk_flow_plan.h."""
    import torch
    from ssds.modeling.layers import fused_conv as FC
    from ssds.modeling.layers.planner import groups_of
    from ssds.modeling.nets.mobilenet import ConvBNReLU6, InvertedResidual
    from test_gpu_guard import _block_want, _randomize

    dtype = torch.bfloat16 if dtype_name == "bf16" else torch.float16
    torch.manual_seed(5)
    stem, blk = ConvBNReLU6(3, 32, stride=2).eval(), InvertedResidual(32, 16, 1, 1).eval()
    _randomize(list(stem.modules()) + list(blk.modules()), dtype, 2.0)
    x = torch.rand(2, 3, 64, 60).to(dtype)
    mods = list(blk.conv.children())
    want = _block_want([stem, mods[0], torch.nn.Sequential(mods[1], mods[2])], x, dtype, False)
    stem, blk = stem.cuda(), blk.cuda()
    sg, bg = groups_of(stem), groups_of(blk.conv)
    assert FC.MbPack.stem_supported(sg, bg)
    pk = FC.MbPack(bg, False, dtype, stem_group=sg[0])
    assert tuple(want.shape) == (2, 16, 32, 30)
    _run_guarded(x.cuda(), pk, want, dtype, "stem block 64x60 " + dtype_name)
