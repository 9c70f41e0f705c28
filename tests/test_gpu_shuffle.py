"""The ShuffleNetV2 unit as one launch (csrc/ssdk_shuffle.hip behind fused_conv.shuffle_unit_native / shuffle_down_native) and the
ShuffleNetV2 plans on the GPU.

Kernels: against the unit's expression in fp32 on the same 16-bit input and the pack's own 16-bit weights,
    m = round16(max(0, conv1x1(x, w1) scale1 + bias1));  d = round16(dw3x3(pad0(m), wd) scale2 + bias2);
    r = round16(max(0, conv1x1(d, w3) scale3 + bias3));  y[2i] = left[i], y[2i + 1] = r[i]
with the three roundings modelled as test_gpu_denselayer._reference models its, and planaudit's bars for a fused op -- (median, p99.9,
max) of |err| / rms: bf16 2e-3 / 0.03 / 0.1, fp16 4e-4 / 6e-3 / 0.03.  The maps come from the kernel's own tile (include/ssdk_shuffle.h
SSDK_SHUFFLE_TILE_H x _W): one pixel, 3 x 2, smaller than a tile both ways, (TH + 3) x (2 TW + 1) -- ragged both ways with more than
one tile each way -- and 13 x 13.  Tensors are [N][H][W][Cp], Cp = pad8(C); the INPUT's padding channels [C, Cp) hold NaN before the
call (a deliberate exception to "padding is zero": a read past C shows as a NaN in y), the OUTPUT's must come back as zeros.

Models: the recorded plan against the reference's fp32 outputs (tests/golden/net_*sfv2*.npz) by the rule of tests/test_gpu_nets.py;
the bare backbone op by op against fp32 on each op's actual input."""
import pytest

import cases_shufflenet
import guardband as G
import nethelp
import planaudit

pytestmark = pytest.mark.gpu

DTYPES = ["bfloat16", "float16"]
CBS = (58, 116, 122, 232, 488)
DOWNS = ((24, 58), (116, 116), (244, 244), (488, 488))
MAPS = range(5)


def _maps():
    from ssds import _native as N

    th, tw = N.SHUFFLE_TILE_H, N.SHUFFLE_TILE_W
    return [(1, 1), (3, 2), (th - 3, tw - 9), (th + 3, 2 * tw + 1), (13, 13)]


def _down_maps():
    from ssds import _native as N

    th, tw = N.SHUFFLE_TILE_H, N.SHUFFLE_TILE_W
    return [(1, 1), (2, 3), (5, 7), (2 * th + 3, 4 * tw + 1), (16, 16)]


def _pad8(c):
    return (c + 7) // 8 * 8


def test_the_parametrisation_covers_the_predicates():
    from ssds import _native as N

    th, tw = N.SHUFFLE_TILE_H, N.SHUFFLE_TILE_W
    small, ragged = _maps()[2], _maps()[3]
    assert 0 < small[0] < th and 0 < small[1] < tw and ragged[0] > th and ragged[0] % th and ragged[1] > tw and ragged[1] % tw
    dh, dw = N.SHUFFLE_DOWN_TILE_H, N.SHUFFLE_DOWN_TILE_W
    big = _down_maps()[3]
    assert ((big[0] - 1) // 2 + 1) % dh and ((big[1] - 1) // 2 + 1) % dw and (big[0] - 1) // 2 + 1 > dh
    for dt in (N.BF16, N.F16):
        assert all(N.lib.ssdk_shuffle_unit_supported(cb, h, w, dt) for cb in CBS for h, w in _maps())
        assert all(N.lib.ssdk_shuffle_down_supported(cin, cb, h, w, dt) for cin, cb in DOWNS for h, w in _down_maps())
    assert any(cb % 8 for cb in CBS) and any(cb % 16 for cb in CBS) and any((2 * cb) % 8 for cb in CBS)


def _gain(h, w, stride=1):
    """test_gpu_dkres._gain: on a small map most taps of the 3x3 fall outside the image and the output shrinks with them;
    sqrt(9 / mean taps inside) scales the depthwise weights so that its output keeps its size on every map."""
    ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
    ty = sum(min(stride * y + 1, h - 1) - max(stride * y - 1, 0) + 1 for y in range(ho))
    tx = sum(min(stride * x + 1, w - 1) - max(stride * x - 1, 0) + 1 for x in range(wo))
    return (9.0 * ho * wo / (ty * tx)) ** 0.5


def _seed_unit(unit, g, gain=1.0):
    """Seeded weights and BatchNorm statistics (cases.seeded_state's distributions); every BatchNorm weight has MIXED SIGNS, as a
    trained BatchNorm's can."""
    import torch

    with torch.no_grad():
        for m in unit.modules():
            if isinstance(m, torch.nn.Conv2d):
                fan_in = (m.in_channels // m.groups) * m.kernel_size[0] * m.kernel_size[1]
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) * (3.0 / fan_in) ** 0.5 * (gain if m.groups > 1 else 1.0))
            elif isinstance(m, torch.nn.BatchNorm2d):
                sign = (torch.randint(0, 2, m.weight.shape, generator=g) * 2 - 1).float()
                m.weight.copy_((torch.rand(m.weight.shape, generator=g) + 0.5) * sign)
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.1)
                m.running_mean.copy_(torch.randn(m.running_mean.shape, generator=g) * 0.1)
                m.running_var.copy_(torch.rand(m.running_var.shape, generator=g) * 0.5 + 0.5)


def _unit(cb, dtype, seed, gain=1.0, cin=None):
    """-> (module on the device, pack) of a seeded stride-1 unit of 2 cb channels, or (``cin``) a stride-2 unit cin -> 2 cb."""
    import torch
    from ssds.modeling.layers import fused_conv as FC
    from ssds.modeling.nets.shufflenet import InvertedResidual

    unit = (InvertedResidual(2 * cb, 2 * cb, 1) if cin is None else InvertedResidual(cin, 2 * cb, 2)).eval()
    _seed_unit(unit, torch.Generator().manual_seed(seed), gain)
    unit = unit.cuda()
    pk = (FC.ShuffleUnitPack if cin is None else FC.ShuffleDownPack)(unit, dtype)
    assert bool((pk.scale1[:cb] < 0).any()) and bool((pk.scale1[:cb] > 0).any())
    return unit, pk


def _input(n, h, w, c, dtype, seed, ld=None):
    """[n][h][w][ld]: channels [0, c) the unit's input (rms 0.7), the padding channels NaN."""
    import torch

    ld = _pad8(c) if ld is None else ld
    g = torch.Generator().manual_seed(seed)
    x = torch.full((n, h, w, ld), float("nan"), dtype=dtype)
    x[..., :c] = (torch.randn(n, h, w, c, generator=g) * 0.7).to(dtype)
    return x.cuda()


def _affine(t, s, b, c):
    return t * s[:c].view(1, -1, 1, 1) + b[:c].view(1, -1, 1, 1)


def _branch2(xf, pk, dtype, stride, kin, wrong_halo=False):
    """fp32 branch2 on NCHW ``xf`` (``kin`` input channels) -> (r [n][cb][ho][wo] rounded, m before the padding)."""
    import torch
    import torch.nn.functional as F

    cb = pk.cb

    def middle(t):
        m = F.conv2d(t, pk.w1[:cb, :kin].float().view(cb, kin, 1, 1))
        return _affine(m, pk.scale1, pk.bias1, cb).clamp(min=0).to(dtype).float()

    m = middle(xf)
    if wrong_halo:  # the WRONG unit whose depthwise sees, outside the image, what the 1x1 makes of an all-zero pixel: relu(bias1)
        n, _, h, w = xf.shape
        outside = middle(torch.zeros(n, kin, h + 2, w + 2, device=xf.device))
        outside[:, :, 1:-1, 1:-1] = m
        mp = outside
    else:
        mp = F.pad(m, (1, 1, 1, 1))
    d = F.conv2d(mp, pk.wd[:, :cb].float().t().reshape(cb, 1, 3, 3), stride=stride, groups=cb)
    d = _affine(d, pk.scale2, pk.bias2, cb).to(dtype).float()
    r = F.conv2d(d, pk.w3[:cb, :cb].float().view(cb, cb, 1, 1))
    return _affine(r, pk.scale3, pk.bias3, cb).clamp(min=0).to(dtype), m


def _interleave(left, right, dtype):
    """NCHW halves -> [n][h][w][pad8(2 cb)]: y[2i] = left[i], y[2i + 1] = right[i], zeros in the padding."""
    import torch

    n, cb, h, w = right.shape
    y = torch.zeros(n, h, w, _pad8(2 * cb), dtype=dtype, device=right.device)
    y[..., 0:2 * cb:2] = left.permute(0, 2, 3, 1)
    y[..., 1:2 * cb:2] = right.permute(0, 2, 3, 1)
    return y


def _reference(x, pk, dtype, wrong_halo=False):
    """The stride-1 unit in fp32 on the 16-bit ``x`` [n][h][w][Cp] and the pack's 16-bit weights -> (y [n][h][w][Cp], m)."""
    import torch

    tf32 = torch.backends.cudnn.allow_tf32
    torch.backends.cudnn.allow_tf32 = False
    try:
        cb = pk.cb
        xc = x.permute(0, 3, 1, 2)
        r, m = _branch2(xc[:, cb:2 * cb].float(), pk, dtype, 1, cb, wrong_halo)
        return _interleave(xc[:, :cb], r, dtype), m
    finally:
        torch.backends.cudnn.allow_tf32 = tf32


def _reference_down(x, pk, dtype, wrong_halo=False):
    """The stride-2 unit in fp32 on channels [0, cin) of ``x`` [n][h][w][ld] -> (y [n][ho][wo][Cp], m)."""
    import torch
    import torch.nn.functional as F

    tf32 = torch.backends.cudnn.allow_tf32
    torch.backends.cudnn.allow_tf32 = False
    try:
        cb, cin = pk.cb, pk.cin
        xf = x[..., :cin].permute(0, 3, 1, 2).float()
        e = F.conv2d(F.pad(xf, (1, 1, 1, 1)), pk.b1_wd[:, :cin].float().t().reshape(cin, 1, 3, 3), stride=2, groups=cin)
        e = _affine(e, pk.b1_scale1, pk.b1_bias1, cin).to(dtype).float()
        left = F.conv2d(e, pk.b1_w2[:cb, :cin].float().view(cb, cin, 1, 1))
        left = _affine(left, pk.b1_scale2, pk.b1_bias2, cb).clamp(min=0).to(dtype)
        r, m = _branch2(xf, pk, dtype, 2, cin, wrong_halo)
        return _interleave(left, r, dtype), m
    finally:
        torch.backends.cudnn.allow_tf32 = tf32


def _within(got, want, dtype, what, kind="fused"):
    med, p999, mx, _ = planaudit.stats(got, want)
    bar = planaudit.BARS[dtype][kind]
    print(what, "median / p99.9 / max = %.5f / %.5f / %.5f of the RMS, bar %s" % (med, p999, mx, bar))
    assert med <= bar[0] and p999 <= bar[1] and mx <= bar[2], (what, med, p999, mx, bar)


def _bits(t):
    import torch

    return t.contiguous().view(torch.int16)


def _rms(t):
    return float(t.float().pow(2).mean().sqrt())


# ---- the stride-1 kernel -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mi", MAPS)
@pytest.mark.parametrize("cb", CBS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_unit_matches_the_fp32_expression(dtype, cb, mi):
    """y against fp32; the input's padding channels are NaN before the call (never read: y is finite); the even output channels are
    x's left half bit for bit; the output's padding channels are zeros; x is unchanged."""
    import torch
    from ssds import _native as N
    from ssds.modeling.layers import fused_conv as FC

    tdt = getattr(torch, dtype)
    h, w = _maps()[mi]
    n, c, cp = 2 + mi % 2, 2 * cb, _pad8(2 * cb)
    _, pk = _unit(cb, tdt, seed=cb + mi, gain=_gain(h, w))
    x = _input(n, h, w, c, tdt, seed=17 * cb + mi)
    before = x.clone()
    want, m = _reference(x, pk, tdt)
    # the comparison decides something: the computed half is of the size of x, the middle map neither dead nor all alive
    assert _rms(want[..., 1:c:2]) >= 0.5 * _rms(x[..., :c]), (_rms(want[..., 1:c:2]), _rms(x[..., :c]))
    assert 0.05 <= float((m == 0).float().mean()) <= 0.95
    y = FC.shuffle_unit_native(x, pk)
    torch.cuda.synchronize()
    assert N.last_kernel() == "shuffle_unit_kernel" and y.shape == x.shape and y.data_ptr() != x.data_ptr()
    assert bool(torch.isfinite(y).all()), "a channel >= C of the input was read"
    _within(y[..., :c], want[..., :c], tdt, "shuffle %d @%dx%d %s" % (cb, h, w, dtype))
    assert torch.equal(_bits(y[..., 0:c:2]), _bits(x[..., :cb])), "the pass-through half is not a bit-exact copy"
    assert cp == c or bool((_bits(y[..., c:]) == 0).all()), "the output's padding channels are not zeros"
    assert G.same_bits(x, before), "the input was written"


# ---- the stride-2 kernel -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mi", MAPS)
@pytest.mark.parametrize("chans", DOWNS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_down_matches_the_fp32_expression(dtype, chans, mi):
    import torch
    from ssds import _native as N
    from ssds.modeling.layers import fused_conv as FC

    tdt = getattr(torch, dtype)
    cin, cb = chans
    h, w = _down_maps()[mi]
    n, c, cp = 2 + mi % 2, 2 * cb, _pad8(2 * cb)
    _, pk = _unit(cb, tdt, seed=cin + cb + mi, gain=_gain(h, w, 2), cin=cin)
    x = _input(n, h, w, cin, tdt, seed=13 * cin + mi)
    before = x.clone()
    want, m = _reference_down(x, pk, tdt)
    assert _rms(want[..., :c]) >= 0.5 * _rms(x[..., :cin]), (_rms(want[..., :c]), _rms(x[..., :cin]))
    assert 0.05 <= float((m == 0).float().mean()) <= 0.95
    y = FC.shuffle_down_native(x, pk)
    torch.cuda.synchronize()
    assert N.last_kernel() == "shuffle_down_kernel" and tuple(y.shape) == (n, (h - 1) // 2 + 1, (w - 1) // 2 + 1, cp)
    assert bool(torch.isfinite(y).all()), "a channel >= Cin of the input was read"
    _within(y[..., 0:c:2], want[..., 0:c:2], tdt, "shuffledown %d>%d @%dx%d %s branch1" % (cin, c, h, w, dtype))
    _within(y[..., 1:c:2], want[..., 1:c:2], tdt, "shuffledown %d>%d @%dx%d %s branch2" % (cin, c, h, w, dtype))
    assert cp == c or bool((_bits(y[..., c:]) == 0).all()), "the output's padding channels are not zeros"
    assert G.same_bits(x, before), "the input was written"


@pytest.mark.parametrize("dtype", DTYPES)
def test_down_reads_a_wider_tensor_and_the_long_input(dtype):
    """The stem's 24 channels in a 32-channel tensor (the plan's conv1 + max-pool), NaN behind them; and Cin = 976 > 512, where the
    kernel runs on half its tile."""
    import torch
    from ssds.modeling.layers import fused_conv as FC

    tdt = getattr(torch, dtype)
    for cin, cb, ld, (h, w) in ((24, 58, 32, (11, 9)), (976, 64, 976, (7, 10))):
        _, pk = _unit(cb, tdt, seed=cin, gain=_gain(h, w, 2), cin=cin)
        x = _input(2, h, w, cin, tdt, seed=cin + 1, ld=ld)
        want, _ = _reference_down(x, pk, tdt)
        y = FC.shuffle_down_native(x, pk)
        assert bool(torch.isfinite(y).all())
        _within(y, want, tdt, "shuffledown %d (ld %d) > %d @%dx%d %s" % (cin, ld, 2 * cb, h, w, dtype))


# ---- the halo ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("down", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
def test_the_halo_outside_the_image_is_zero_not_what_the_biases_give(dtype, down):
    """bias1 = +3 on every middle channel: relu(bias1) = 3 where a kernel that computes its halo from the biases would put it.  Such
    a kernel is wrong by O(1) on every border pixel and right inside."""
    import torch
    from ssds import _native as N
    from ssds.modeling.layers import fused_conv as FC

    tdt = getattr(torch, dtype)
    cb = 116
    h, w = N.SHUFFLE_TILE_H + 3, 2 * N.SHUFFLE_TILE_W + 1
    _, pk = _unit(cb, tdt, seed=5, cin=116 if down else None)
    pk.bias1.fill_(3.0)
    x = _input(2, h, w, 116 if down else 2 * cb, tdt, seed=6)
    ref = _reference_down if down else _reference
    want, _ = ref(x, pk, tdt)
    wrong, _ = ref(x, pk, tdt, wrong_halo=True)
    want, wrong = want[..., 1:2 * cb:2].float(), wrong[..., 1:2 * cb:2].float()  # (the halves branch2 computes)
    ho, wo = want.shape[1:3]
    border = torch.ones(ho, wo, dtype=torch.bool, device="cuda")
    if down:  # stride 2, pad 1: the first row and column always see the padding, the last ones when the size is odd
        border[1:ho - (h % 2 == 1), 1:wo - (w % 2 == 1)] = False
    else:
        border[1:-1, 1:-1] = False
    bar = planaudit.BARS[tdt]["fused"]
    rms = float(want.pow(2).mean().sqrt())
    assert float((wrong - want)[:, border].abs().mean()) > max(0.2, 10 * bar[0]) * rms > 0  # the wrong halo shows, on the border ...
    # ... and only there: inside, the two expressions are the same sums on tensors of two sizes (a rounding of the 16-bit result may
    # flip with the library's summation order), so they agree to the bars the kernel is held to
    _within(wrong[:, ~border], want[:, ~border], tdt, "the wrong expression's interior %s" % dtype)
    y = (FC.shuffle_down_native if down else FC.shuffle_unit_native)(x, pk)[..., 1:2 * cb:2]
    _within(y[:, border], want[:, border], tdt, "border %s" % dtype)
    _within(y[:, ~border], want[:, ~border], tdt, "interior %s" % dtype)
    med, _, _, _ = planaudit.stats(y[:, border], wrong[:, border])
    assert med > 10 * bar[0], "the kernel computes the wrong unit's border"


# ---- guard bands -------------------------------------------------------------------------------------------------------------------
_UNIT_TENSORS = ("w1_img", "scale1", "bias1", "wd", "affine2", "w3_img", "scale3", "bias3")
_DOWN_TENSORS = _UNIT_TENSORS + ("b1_wd", "b1_scale1", "b1_bias1", "b1_w2_img", "b1_scale2", "b1_bias2")


def _guard_pack(pk, names, gs):
    for name in names:
        st, view = G.guarded(getattr(pk, name))
        setattr(pk, name, view)
        gs.adopt(name, st, view)
    pk.scale2, pk.bias2 = pk.affine2[0], pk.affine2[1]


@pytest.mark.parametrize("shape", [(3, 58, 5, 7), (2, 116, 11, 17), (2, 488, 5, 9)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_unit_between_guard_bands(dtype, shape):
    """The guards around x, y, the weight images and every vector intact; the same bits as on ordinary allocations."""
    import torch
    from ssds.modeling.layers import fused_conv as FC

    tdt = getattr(torch, dtype)
    n, cb, h, w = shape
    _, pk = _unit(cb, tdt, seed=cb + h)
    x = _input(n, h, w, 2 * cb, tdt, seed=h * w)
    clean = FC.shuffle_unit_native(x, pk)
    gs = G.GuardSet("cuda")
    xg = gs.inp("x", x)
    yg = gs.out("y", tuple(x.shape), tdt)
    _guard_pack(pk, _UNIT_TENSORS, gs)
    gs.arm()
    FC.shuffle_unit_native(xg, pk, y=yg)
    torch.cuda.synchronize()
    assert gs.problems() == []
    assert G.same_bits(yg, clean) and not G.has_nan(yg)


@pytest.mark.parametrize("shape", [(3, 24, 58, 5, 7), (2, 116, 116, 11, 18), (2, 488, 488, 5, 9)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_down_between_guard_bands(dtype, shape):
    import torch
    from ssds.modeling.layers import fused_conv as FC

    tdt = getattr(torch, dtype)
    n, cin, cb, h, w = shape
    _, pk = _unit(cb, tdt, seed=cb + h, cin=cin)
    x = _input(n, h, w, cin, tdt, seed=h * w)
    clean = FC.shuffle_down_native(x, pk)
    gs = G.GuardSet("cuda")
    xg = gs.inp("x", x)
    yg = gs.out("y", tuple(clean.shape), tdt)
    _guard_pack(pk, _DOWN_TENSORS, gs)
    gs.arm()
    FC.shuffle_down_native(xg, pk, y=yg)
    torch.cuda.synchronize()
    assert gs.problems() == []
    assert G.same_bits(yg, clean) and not G.has_nan(yg)


# ---- capture, replay, determinism ------------------------------------------------------------------------------------------------------
def _capture(fn):
    import torch

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()  # (warm-up outside the capture)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fn()
    return graph


def test_capture_and_replay_through_a_graph_and_two_runs_give_the_same_bits():
    import torch
    from ssds.modeling.layers import fused_conv as FC

    _, pd = _unit(58, torch.float16, seed=11, cin=24)
    _, pu = _unit(58, torch.float16, seed=12)
    x = _input(2, 21, 19, 24, torch.float16, seed=13)

    def run(mid=None, out=None):
        mid = FC.shuffle_down_native(x, pd, y=mid)
        return mid, FC.shuffle_unit_native(mid, pu, y=out)

    mid1, first = run()
    mid2, second = run()
    torch.cuda.synchronize()
    assert G.same_bits(first, second) and G.same_bits(mid1, mid2), "two runs differ"
    mid, out = torch.empty_like(mid1), torch.empty_like(first)
    graph = _capture(lambda: run(mid, out))
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert G.same_bits(out, first)
    x[..., :24] = torch.flip(x[..., :24], dims=[1, 2]).clone()  # new contents in the captured input
    graph.replay()
    torch.cuda.synchronize()
    _, again = run()
    assert G.same_bits(out, again) and not G.same_bits(out, first)


# ---- a stage: a down unit and three stride-1 units ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_stage_of_four_units_against_the_module(dtype):
    """stage2 of ShuffleNetV2 x1 (24 -> 116, four units) on the kernels against the module's stage in fp32 on the same 16-bit weights,
    which rounds NOTHING in between.  Unit j of the kernel chain carries its own three roundings and those of the j - 1 units it
    reads: 3 j independent roundings of the same relative size where the bar of one op allows for one, and independent errors add
    in quadrature -- the bars times sqrt(3 j) (test_gpu_denselayer's chain rule).  A wrong wire, interleave or offset is >= 1."""
    import torch
    from ssds.modeling.layers import fused_conv as FC
    from ssds.modeling.nets.shufflenet import InvertedResidual

    tdt = getattr(torch, dtype)
    g = torch.Generator().manual_seed(31)
    units = [InvertedResidual(24, 116, 2)] + [InvertedResidual(116, 116, 1) for _ in range(3)]
    stage = torch.nn.Sequential(*units).eval()
    for u in units:
        _seed_unit(u, g)
        with torch.no_grad():
            for m in u.modules():
                if isinstance(m, torch.nn.Conv2d):
                    m.weight.copy_(m.weight.to(tdt).float())
    stage = stage.cuda()
    n, h, w = 2, 19, 23
    x = _input(n, h, w, 24, tdt, seed=32)
    with torch.no_grad():
        want = stage(x.permute(0, 3, 1, 2).float())
    cur = FC.shuffle_down_native(x, FC.ShuffleDownPack(units[0], tdt))
    for u in units[1:]:
        cur = FC.shuffle_unit_native(cur, FC.ShuffleUnitPack(u, tdt))
    torch.cuda.synchronize()
    assert tuple(cur.shape) == (n, 10, 12, 120) and bool((_bits(cur[..., 116:]) == 0).all())
    got = cur[..., :116].permute(0, 3, 1, 2)
    assert want.shape == got.shape and bool(torch.isfinite(got).all())
    bar, k = planaudit.BARS[tdt]["fused"], (3.0 * 4) ** 0.5
    med, p999, mx, _ = planaudit.stats(got, want)
    print("stage2 against the module %s: median / p99.9 / max = %.5f / %.5f / %.5f, bar %s x %.2f" % (dtype, med, p999, mx, bar, k))
    assert med <= k * bar[0] and p999 <= k * bar[1] and mx <= k * bar[2], (med, p999, mx, bar, k)


def test_a_tensor_of_the_wrong_width_is_refused():
    import torch
    from ssds import _native as N
    from ssds.modeling.layers import fused_conv as FC

    _, pk = _unit(58, torch.bfloat16, seed=1)
    x = _input(2, 5, 7, 116, torch.bfloat16, seed=2)
    with pytest.raises(N.SsdkError, match="channels per pixel"):
        FC.shuffle_unit_native(x[..., :112].contiguous(), pk)
    with pytest.raises(N.SsdkError, match="overlaps"):
        FC.shuffle_unit_native(x, pk, y=x)


# ---- the plans ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(cases_shufflenet.NET_CASES))
def test_plan_matches_reference_module(name, dtype, monkeypatch):
    import torch
    from ssds.modeling.layers import fused_conv as FC
    from test_shufflenet_cpu import build
    from test_gpu_nets import POOL_DRAWS, SMALL, _check_against_floor, check_small_levels_pooled, floor_runs

    monkeypatch.setenv("SSDK_SHUFFLEUNIT", "1")
    tdt = getattr(torch, dtype)
    model, x, fx = build(name, monkeypatch)
    wl, wc = nethelp.want(fx)
    model = model.cuda().to(tdt)
    xd = x.cuda().to(tdt)
    runs = FC.STATS["plan_runs"]
    with torch.no_grad():
        loc, conf = model(xd)
        loc2, conf2 = model(xd)
    assert FC.STATS["plan_runs"] == runs + 2, "the forward did not run as a recorded plan"
    plans = {k: p for k, p in model.__dict__["_neck_plans"].items() if isinstance(p, FC.ConvPlan)}
    refused = [p for p in model.__dict__["_neck_plans"].values() if isinstance(p, str)]
    assert len(plans) == 1, refused
    (key, plan), = plans.items()
    assert key[0] == "image", "the ShuffleNetV2 backbone was not part of the plan: %s" % refused
    table = plan.layer_table()
    assert len(table) == len(plan.layers)
    assert len([r for r in table if r["name"].startswith("shuffle ")]) == 13
    assert len([r for r in table if r["name"].startswith("shuffledown ")]) == 3
    assert (name != "fpn_sfv2x1") == bool([r for r in table if r["name"].startswith("cat ")])  # (YOLOv3's neck concatenates; no unit does)
    for a, b in zip(loc + conf, loc2 + conf2):
        assert a.is_contiguous() and a.dtype == tdt and torch.equal(a, b), "replay is not deterministic"
    # SSDK_FUSED_CONV=0 gives the module path (floor_runs sets it): no plan, no HIP kernel of this library
    n0, p0 = FC.STATS["native_layers"], FC.STATS["plan_runs"]
    floor = floor_runs(model, xd)
    assert FC.STATS["native_layers"] == n0 and FC.STATS["plan_runs"] == p0
    report = _check_against_floor({"loc": loc, "conf": conf}, floor, {"loc": wl, "conf": wc}, name, dtype)
    print(name, dtype, "; ".join(report))
    # small levels: pooled over POOL_DRAWS more inputs, as tests/test_gpu_nets.py does it
    assert any(t.numel() < SMALL for t in wl + wc)
    cpu_model, _, _ = build(name, monkeypatch)
    cpu = lambda t: t.float().cpu()
    plans_o, floors, wants = [{"loc": [cpu(t) for t in loc], "conf": [cpu(t) for t in conf]}], [
        {"loc": [cpu(t) for t in floor[0]["loc"]], "conf": [cpu(t) for t in floor[0]["conf"]]}], [{"loc": wl, "conf": wc}]
    g = torch.Generator().manual_seed(4711)
    for _ in range(POOL_DRAWS):
        xi = torch.rand(x.shape, generator=g)
        with torch.no_grad():
            cl_, cc_ = cpu_model(xi)
            pl, pc = model(xi.cuda().to(tdt))
        fl = floor_runs(model, xi.cuda().to(tdt), runs=1)[0]
        wants.append({"loc": list(cl_), "conf": list(cc_)})
        plans_o.append({"loc": [cpu(t) for t in pl], "conf": [cpu(t) for t in pc]})
        floors.append({"loc": [cpu(t) for t in fl["loc"]], "conf": [cpu(t) for t in fl["conf"]]})
    assert check_small_levels_pooled(plans_o, floors, wants, name, dtype)


def _bare_plan(tdt):
    """-> (plan, image on the device, output values, fixture): the backbone alone, recorded from the image."""
    import torch
    from ssds.modeling.layers import fused_conv as FC
    from ssds.modeling.layers import planner
    from test_shufflenet_cpu import build_bare

    net, x, fx = build_bare()
    net = net.eval().cuda().to(tdt)
    xd = x.cuda().to(tdt)
    plan = FC.ConvPlan(xd.device, tdt, xd.shape)
    with torch.no_grad():
        outs = planner.record_backbone(plan, plan.input_value(), net)
    return plan.finalize(), xd, outs, fx, net


class _Audit(planaudit.PlanAudit):
    """planaudit.PlanAudit with the reference arithmetic of the two shuffle ops, each in fp32 on the op's ACTUAL input."""

    def nhwc(self, buf, n, h, w, c):
        return self.plan.arena.bufs[buf][0][: n * h * w * c * self.plan.es].view(self.dtype).view(n, h, w, c)

    def _ref_shuffle(self, i, L):
        pk, down = L["pack"], L["kind"] == "shuffledown"
        cp = _pad8(2 * pk.cb)
        xin = self.nhwc(L["x"], L["n"], L["h"], L["w"], L["ld"] if down else cp)[self.sel].clone()

        def run():
            want, _ = (_reference_down if down else _reference)(xin, pk, self.dtype)
            ho, wo = ((L["h"] - 1) // 2 + 1, (L["w"] - 1) // 2 + 1) if down else (L["h"], L["w"])
            return self.nhwc(L["y"], L["n"], ho, wo, cp)[self.sel], want

        return run

    def run(self):
        import torch
        from ssds import _native as N

        plan, rows = self.plan, []
        table = plan.layer_table()
        refs = {None: self._ref_conv, "pool": self._ref_pool, "shuffle": self._ref_shuffle, "shuffledown": self._ref_shuffle}
        tf32 = torch.backends.cudnn.allow_tf32
        torch.backends.cudnn.allow_tf32 = False
        try:
            for i, L in enumerate(plan.layers):
                with torch.no_grad():
                    ref = refs[L.get("kind")](i, L)  # copies the op's inputs BEFORE the launch
                    plan.launch(i, i + 1)
                    torch.cuda.synchronize()
                    kern = N.last_kernel()
                    got, want = ref()
                    med, p999, mx, zeros = planaudit.stats(got, want)
                rows.append(dict(index=i, name=table[i]["name"], kernel=kern.replace("_kernel", ""),
                                 kind="fused" if L.get("kind") in ("shuffle", "shuffledown") else "default", median=med, p999=p999,
                                 max=mx, zeros=zeros))
        finally:
            torch.backends.cudnn.allow_tf32 = tf32
        return rows


@pytest.mark.parametrize("dtype", DTYPES)
def test_bare_backbone_op_by_op(dtype, monkeypatch):
    """Every op of the bare-backbone plan, launched on its own, against fp32 on the op's actual input (planaudit's bars); the maps
    handed back are sliced to their real channels and are as close to the reference's fp32 maps as the same module executed by
    PyTorch-ROCm in the same dtype is (the rule of tests/test_gpu_nets.py: 16 units in 16 bits amplify rounding noise)."""
    import torch
    from test_gpu_nets import _check_against_floor

    monkeypatch.setenv("SSDK_SHUFFLEUNIT", "1")
    tdt = getattr(torch, dtype)
    plan, xd, outs, fx, net = _bare_plan(tdt)
    rows = _Audit(plan, [xd]).run()
    print(planaudit.format_rows([dict(r, plan_kernel="") for r in rows]))
    assert len(rows) == len(plan.layers) == 2 + 16
    assert [r["kernel"] for r in rows if r["name"].startswith("shuffle ")] == ["shuffle_unit"] * 13
    assert [r["kernel"] for r in rows if r["name"].startswith("shuffledown ")] == ["shuffle_down"] * 3
    assert not planaudit.failures(rows, tdt), planaudit.failures(rows, tdt)
    with torch.no_grad():
        plan.run(xd)
        floor = [{"loc": net(xd), "conf": []} for _ in range(3)]
    torch.cuda.synchronize()
    got = [plan.read(o) for o in outs]
    want = [torch.from_numpy(fx["out%d" % i]) for i in range(len(outs))]
    assert [tuple(g.shape) for g in got] == [tuple(w.shape) for w in want] == [(2, 232, 6, 4), (2, 464, 3, 2)]
    report = _check_against_floor({"loc": got, "conf": []}, floor, {"loc": want, "conf": []}, "sfv2x1_bare", dtype)
    print("sfv2x1_bare", dtype, "; ".join(report))


def test_op_profiling_names_the_kernels(monkeypatch):
    import torch

    monkeypatch.setenv("SSDK_SHUFFLEUNIT", "1")
    plan, xd, _, _, _ = _bare_plan(torch.bfloat16)
    with torch.no_grad():
        plan.run(xd)
        plan.ctx.set_op_profiling(True)
        plan.run(xd)
        torch.cuda.synchronize()
        timings = plan.ctx.op_timings()
        plan.ctx.set_op_profiling(False)
    assert len(timings) == len(plan.layers)
    names = [r["name"] for r in plan.layer_table()]
    for (kern, ms), name in zip(timings, names):
        assert (kern == "shuffle_unit_kernel") == name.startswith("shuffle "), (kern, name)
        assert (kern == "shuffle_down_kernel") == name.startswith("shuffledown "), (kern, name)
        assert ms >= 0
    assert sum(n.startswith("shuffle ") for n in names) == 13


# ---- the switch --------------------------------------------------------------------------------------------------------------------
def test_the_switch_puts_the_backbone_back_on_torch(monkeypatch):
    """SSDK_SHUFFLEUNIT=0 (docs/SWITCHES.md; read whenever a plan is recorded): the image plan is refused with the switch's name and
    the detector still runs, on the module path (a 116-channel map is no input for the neck plan either, and the plan says so).  The
    outputs are judged against the reference's fp32 outputs by the rule of tests/test_gpu_nets.py."""
    import torch
    from ssds.modeling.layers import fused_conv as FC
    from test_shufflenet_cpu import build
    from test_gpu_nets import _check_against_floor, floor_runs

    name, dtype = "fpn_sfv2x1", "bfloat16"
    tdt = getattr(torch, dtype)
    for env in ("1", "0"):
        monkeypatch.setenv("SSDK_SHUFFLEUNIT", env)
        model, x, fx = build(name, monkeypatch)
        model = model.cuda().to(tdt)
        xd = x.cuda().to(tdt)
        runs = FC.STATS["plan_runs"]
        with torch.no_grad():
            loc, conf = model(xd)
        torch.cuda.synchronize()
        entries = model.__dict__["_neck_plans"]
        image = [p for k, p in entries.items() if k[0] == "image"]
        assert len(image) == 1
        if env == "1":
            assert isinstance(image[0], FC.ConvPlan) and len(entries) == 1 and FC.STATS["plan_runs"] == runs + 1
            continue
        assert isinstance(image[0], str) and "SSDK_SHUFFLEUNIT=0" in image[0]
        assert FC.STATS["plan_runs"] == runs, "a plan ran although the backbone is on the module path"
        necks = [p for k, p in entries.items() if k[0] != "image"]
        assert len(necks) == 1 and isinstance(necks[0], str) and "116 channels" in necks[0]
        wl, wc = nethelp.want(fx)
        report = _check_against_floor({"loc": loc, "conf": conf}, floor_runs(model, xd), {"loc": wl, "conf": wc}, name, dtype)
        print(name, dtype, "SSDK_SHUFFLEUNIT=0", "; ".join(report))
