"""The DenseNet dense layer as one launch (csrc/ssdk_denselayer.hip behind fused_conv.dense_layer_native), the two small kernels
around it, and the DenseNet121 plans on the GPU.

Kernel: against the layer's expression in fp32 on the same 16-bit input and the pack's folded 16-bit weights,
    xa = round16(max(0, a x + b));  m = round16(max(0, conv1x1(xa, w1) scale1 + bias1));  y = conv3x3(pad0(m), w2)
with both intermediate roundings modelled as test_gpu_dkres._reference models its ``m``, and planaudit's bars for a fused op --
(median, p99.9, max) of |err| / rms: bf16 2e-3 / 0.03 / 0.1, fp16 4e-4 / 6e-3 / 0.03.  The maps come from the kernel's own tile
(include/ssdk_denselayer.h SSDK_DENSE_TILE_H x _W): one pixel, 3 x 2, smaller than a tile both ways, (TH + 3) x (2 TW + 1) -- ragged
both ways with more than one tile each way -- and 13 x 13.  The layer's input sits in channels [0, Cin) of a buffer of pixel stride ld;
every other channel of the buffer holds NaN before the call, so a read past Cin shows in y and a write outside [Cin, Cin + 32) shows
as a changed bit.

Models: the recorded plan against the reference's fp32 outputs (tests/golden/net_*dn121*.npz) by the rule of tests/test_gpu_nets.py;
the bare backbone op by op against fp32 on each op's actual input."""
import pytest

import cases_densenet
import guardband as G
import nethelp
import planaudit

pytestmark = pytest.mark.gpu

DTYPES = ["bfloat16", "float16"]
CINS = (32, 64, 96, 224, 992)
MAPS = range(5)
PADS = (32, 96)  # ld - Cin


def _maps():
    from ssds import _native as N

    th, tw = N.DENSE_TILE_H, N.DENSE_TILE_W
    return [(1, 1), (3, 2), (th - 3, tw - 9), (th + 3, 2 * tw + 1), (13, 13)]


def test_the_parametrisation_covers_the_predicate():
    from ssds import _native as N

    th, tw = N.DENSE_TILE_H, N.DENSE_TILE_W
    small, ragged = _maps()[2], _maps()[3]
    assert 0 < small[0] < th and 0 < small[1] < tw and ragged[0] > th and ragged[0] % th and ragged[1] > tw and ragged[1] % tw
    for c in CINS:
        for dt in (N.BF16, N.F16):
            assert all(N.lib.ssdk_dense_layer_supported(c, h, w, c + p, dt) for h, w in _maps() for p in PADS)


def _gain(h, w):
    """test_gpu_dkres._gain: on a small map most taps of the 3x3 fall outside the image and the output shrinks with them;
    sqrt(9 / mean taps inside) scales w2 so that y keeps the size of x on every map (1 on a large map, 3 on 1 x 1)."""
    taps = sum(min(y + 1, h - 1) - max(y - 1, 0) + 1 for y in range(h)) * sum(min(x + 1, w - 1) - max(x - 1, 0) + 1 for x in range(w))
    return (9.0 * h * w / taps) ** 0.5


def _seed_layer(layer, g, gain2=1.0):
    """Seeded weights and BatchNorm statistics (cases.seeded_state's distributions); norm1's weight has MIXED SIGNS, as a trained
    BatchNorm's can: ``a`` is negative on about half of the channels."""
    import torch

    with torch.no_grad():
        for conv, gain in ((layer.conv1, 1.0), (layer.conv2, gain2)):
            fan_in = conv.in_channels * conv.kernel_size[0] * conv.kernel_size[1]
            conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) * (3.0 / fan_in) ** 0.5 * gain)
        for bn, signed in ((layer.norm1, True), (layer.norm2, False)):
            wgt = torch.rand(bn.weight.shape, generator=g) + 0.5
            if signed:
                wgt = wgt * (torch.randint(0, 2, bn.weight.shape, generator=g) * 2 - 1).float()
            bn.weight.copy_(wgt)
            bn.bias.copy_(torch.randn(bn.bias.shape, generator=g) * 0.1)
            bn.running_mean.copy_(torch.randn(bn.running_mean.shape, generator=g) * 0.1)
            bn.running_var.copy_(torch.rand(bn.running_var.shape, generator=g) * 0.5 + 0.5)


def _layer(cin, dtype, seed, gain2=1.0):
    """-> the pack of a seeded _DenseLayer of ``cin`` input channels."""
    import torch
    from ssds.modeling.layers import fused_conv as FC
    from ssds.modeling.nets.densenet import _DenseLayer

    layer = _DenseLayer(cin, 32, 4, 0).eval()
    _seed_layer(layer, torch.Generator().manual_seed(seed), gain2)
    pk = FC.DenseLayerPack(layer.cuda(), dtype)
    assert bool((pk.a < 0).any()) and bool((pk.a > 0).any())
    return pk


def _buffer(n, h, w, cin, ld, dtype, seed, x=None):
    """[n][h][w][ld]: channels [0, cin) the layer's input (rms 0.7), every other channel NaN."""
    import torch

    g = torch.Generator().manual_seed(seed)
    buf = torch.full((n, h, w, ld), float("nan"), dtype=dtype)
    buf[..., :cin] = (torch.randn(n, h, w, cin, generator=g) * 0.7).to(dtype) if x is None else x
    return buf.cuda()


def _reference(xin, pk, dtype, wrong_halo=False):
    """fp32 on the 16-bit input ``xin`` [n][h][w][cin] and the pack's 16-bit weights -> y [n][h][w][32].  ``wrong_halo``: the WRONG
    layer whose 3x3 sees, outside the image, what the 1x1 makes of an all-zero pixel's relu(b) -- a kernel that computes its halo
    from the biases instead of storing zeros."""
    import torch
    import torch.nn.functional as F

    tf32 = torch.backends.cudnn.allow_tf32
    torch.backends.cudnn.allow_tf32 = False
    try:
        def middle(xf):
            xa = (xf * pk.a.view(1, -1, 1, 1) + pk.b.view(1, -1, 1, 1)).clamp(min=0).to(dtype).float()
            m = F.conv2d(xa, pk.w1.float().view(pk.cmid, pk.cin, 1, 1))
            return (m * pk.scale1.view(1, -1, 1, 1) + pk.bias1.view(1, -1, 1, 1)).clamp(min=0).to(dtype).float()

        xf = xin.float().permute(0, 3, 1, 2)
        m = middle(xf)
        if wrong_halo:
            n, _, h, w = xf.shape
            outside = middle(torch.zeros(n, pk.cin, h + 2, w + 2, device=xf.device))
            outside[:, :, 1:-1, 1:-1] = m
            m = outside
        else:
            m = F.pad(m, (1, 1, 1, 1))
        y = F.conv2d(m, pk.w2.float().permute(0, 3, 1, 2).contiguous())
        return y.permute(0, 2, 3, 1).contiguous(), m
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


# ---- the layer kernel --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("mi", MAPS)
@pytest.mark.parametrize("cin", CINS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_kernel_matches_the_fp32_expression(dtype, cin, mi, pad):
    """y against fp32; channels >= Cin are NaN before the call (never read: y is finite); channels outside [Cin, Cin + 32) keep
    their bits (never written)."""
    import torch
    from ssds import _native as N
    from ssds.modeling.layers import fused_conv as FC

    tdt = getattr(torch, dtype)
    h, w = _maps()[mi]
    n, ld = 2 + mi % 2, cin + pad
    pk = _layer(cin, tdt, seed=cin + mi, gain2=_gain(h, w))
    buf = _buffer(n, h, w, cin, ld, tdt, seed=17 * cin + mi)
    before = buf.clone()
    want, m = _reference(buf[..., :cin], pk, tdt)
    # the comparison decides something: y is of the size of x, the middle map neither dead nor all alive
    rms = lambda t: float(t.float().pow(2).mean().sqrt())
    assert rms(want) >= 0.5 * rms(buf[..., :cin]), (rms(want), rms(buf[..., :cin]))
    inner = m[:, :, 1:-1, 1:-1]
    assert 0.05 <= float((inner == 0).float().mean()) <= 0.95
    out = FC.dense_layer_native(buf, pk)
    torch.cuda.synchronize()
    assert N.last_kernel() == "dense_layer_kernel" and out.data_ptr() == buf.data_ptr()
    y = buf[..., cin:cin + 32]
    assert bool(torch.isfinite(y).all()), "a channel >= Cin was read"
    _within(y, want, tdt, "dense %d ld %d @%dx%d %s" % (cin, ld, h, w, dtype))
    assert torch.equal(_bits(buf[..., :cin]), _bits(before[..., :cin])), "the input channels were written"
    assert torch.equal(_bits(buf[..., cin + 32:]), _bits(before[..., cin + 32:])), "channels behind the layer's 32 were written"


@pytest.mark.parametrize("shape", [(3, 64, 5, 7, 96), (2, 224, 11, 33, 320), (2, 992, 5, 7, 1024)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_guard_bands(dtype, shape):
    """The guards around the buffer, both weights (KRSC and fragment images) and the four vectors intact; inside the buffer only the
    layer's 32 channels change; the same bits as on ordinary allocations."""
    import torch
    from ssds.modeling.layers import fused_conv as FC

    tdt = getattr(torch, dtype)
    n, cin, h, w, ld = shape
    pk = _layer(cin, tdt, seed=cin + h)
    buf = _buffer(n, h, w, cin, ld, tdt, seed=h * w)
    before = buf.clone()
    clean = FC.dense_layer_native(buf.clone(), pk)
    gs = G.GuardSet("cuda")
    storage, bg = G.guarded(buf)
    gs.adopt("buffer", storage, bg, is_input=False)
    for name in ("a", "b", "w1", "scale1", "bias1", "w2", "w1_frag", "w2_frag"):
        st, view = G.guarded(getattr(pk, name))
        setattr(pk, name, view)
        gs.adopt(name, st, view)
    gs.arm()
    FC.dense_layer_native(bg, pk)
    torch.cuda.synchronize()
    assert gs.problems() == []
    assert G.same_bits(bg, clean) and not G.has_nan(bg[..., cin:cin + 32])
    assert torch.equal(_bits(bg[..., :cin]), _bits(before[..., :cin]))
    assert torch.equal(_bits(bg[..., cin + 32:]), _bits(before[..., cin + 32:]))


@pytest.mark.parametrize("cin", (64, 224))
@pytest.mark.parametrize("dtype", DTYPES)
def test_the_halo_outside_the_image_is_zero_not_what_the_biases_give(dtype, cin):
    """x = 0, b = +3, bias1 = +3: relu(b) = 3 on every input channel, so the middle map is the same non-zero vector on every pixel
    of the image.  A kernel that computes its halo outside the image from the biases is wrong by O(1) on every border pixel and right
    inside."""
    import torch
    from ssds import _native as N
    from ssds.modeling.layers import fused_conv as FC

    tdt = getattr(torch, dtype)
    h, w = N.DENSE_TILE_H + 3, 2 * N.DENSE_TILE_W + 1
    pk = _layer(cin, tdt, seed=cin)
    pk.b.fill_(3.0)
    pk.bias1.fill_(3.0)
    buf = _buffer(2, h, w, cin, cin + 32, tdt, seed=1, x=0.0)
    want, _ = _reference(buf[..., :cin], pk, tdt)
    wrong, _ = _reference(buf[..., :cin], pk, tdt, wrong_halo=True)
    border = torch.ones(h, w, dtype=torch.bool, device="cuda")
    border[1:-1, 1:-1] = False
    rms = float(want.pow(2).mean().sqrt())
    assert float((wrong - want)[:, border].abs().mean()) > 0.2 * rms > 0  # the wrong halo shows, on the border ...
    assert float((wrong - want)[:, ~border].abs().max()) <= 1e-5 * rms     # ... and only there
    FC.dense_layer_native(buf, pk)
    y = buf[..., cin:]
    _within(y[:, border], want[:, border], tdt, "border %d %s" % (cin, dtype))
    _within(y[:, ~border], want[:, ~border], tdt, "interior %d %s" % (cin, dtype))
    med, _, _, _ = planaudit.stats(y[:, border], wrong[:, border])
    assert med > 10 * planaudit.BARS[tdt]["fused"][0], "the kernel computes the wrong layer's border"


@pytest.mark.parametrize("frag", [True, False])
def test_both_weight_layouts(frag, monkeypatch):
    """The fragment-major images and the KRSC tensors are two instances of the kernel: the same bits."""
    import torch
    from ssds.modeling.layers import fused_conv as FC

    monkeypatch.setattr(FC, "USE_WFRAG", frag)
    pk = _layer(224, torch.bfloat16, seed=5)
    assert (pk.w1_frag is not None) == frag and (pk.w2_frag is not None) == frag
    buf = _buffer(2, 11, 33, 224, 320, torch.bfloat16, seed=6)
    want, _ = _reference(buf[..., :224], pk, torch.bfloat16)
    other = buf.clone()
    FC.dense_layer_native(buf, pk)
    _within(buf[..., 224:256], want, torch.bfloat16, "dense 224 frag=%s" % frag)
    monkeypatch.setattr(FC, "USE_WFRAG", not frag)
    pk2 = _layer(224, torch.bfloat16, seed=5)
    assert (pk2.w1_frag is not None) != frag
    FC.dense_layer_native(other, pk2)
    assert G.same_bits(buf, other)


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

    pk = _layer(96, torch.float16, seed=11)
    buf = _buffer(2, 11, 33, 96, 128, torch.float16, seed=12)
    first, second = buf.clone(), buf.clone()
    FC.dense_layer_native(first, pk)
    FC.dense_layer_native(second, pk)
    torch.cuda.synchronize()
    assert G.same_bits(first, second), "two runs differ"
    graph = _capture(lambda: FC.dense_layer_native(buf, pk))
    buf[..., 96:] = 0
    graph.replay()
    torch.cuda.synchronize()
    assert G.same_bits(buf, first)
    buf[..., :96] = torch.flip(buf[..., :96], dims=[1, 2]).clone()  # new contents in the captured buffer
    graph.replay()
    torch.cuda.synchronize()
    again = buf.clone()
    FC.dense_layer_native(again, pk)
    assert G.same_bits(buf, again) and not G.same_bits(buf[..., 96:], first[..., 96:])


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_chain_of_three_layers_in_one_buffer(dtype):
    """place + three layers, each reading the channels the one before it wrote.

    (a) Against the layer's expression applied three times, every layer on the 16-bit channels the expression itself produced before
    it: the bars of one fused op, since the kernel's input differs from the expression's only where an accumulation order flipped a
    rounding of y.
    (b) Against the module's _DenseBlock in fp32 on the same 16-bit weights, which rounds NOTHING in between.  Layer j of the kernel
    chain carries its own three roundings (xa, m, y) and those of the j - 1 layers it reads: 3 j independent roundings of the same
    relative size where the bar of one op allows for one, and independent errors add in quadrature -- the bars times sqrt(3 j), and
    times sqrt(9) for the buffer as a whole.  (A wrong wire, channel offset or stride is >= 1.)"""
    import torch
    from ssds.modeling.layers import fused_conv as FC
    from ssds.modeling.nets.densenet import _DenseBlock

    tdt = getattr(torch, dtype)
    n, c0, h, w = 2, 64, 11, 19
    block = _DenseBlock(3, c0, 4, 32, 0).eval()
    g = torch.Generator().manual_seed(21)
    for layer in block.values():
        _seed_layer(layer, g)
        with torch.no_grad():
            for conv in (layer.conv1, layer.conv2):
                conv.weight.copy_(conv.weight.to(tdt).float())
    block = block.cuda()
    x = (torch.randn(n, c0, h, w, generator=g) * 0.7).to(tdt).cuda().contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        want = block(x.float())
    assert want.shape == (n, c0 + 96, h, w)
    packs = [FC.DenseLayerPack(layer, tdt) for layer in block.values()]
    buf = torch.full((n, h, w, c0 + 96), float("nan"), dtype=tdt, device="cuda")
    FC.dense_place_native(x, buf)
    for pk in packs:
        FC.dense_layer_native(buf, pk)
    torch.cuda.synchronize()
    got = buf.permute(0, 3, 1, 2)
    assert bool(torch.isfinite(got).all()) and torch.equal(got[:, :c0], x)
    # (a) the expression, layer by layer on its own 16-bit outputs
    cur = x.permute(0, 2, 3, 1).contiguous()
    for j, pk in enumerate(packs):
        lo = c0 + 32 * j
        y, _ = _reference(cur, pk, tdt)
        _within(buf[..., lo:lo + 32], y, tdt, "chain layer %d against the expression %s" % (j + 1, dtype))
        cur = torch.cat([cur, y.to(tdt)], -1)
    # (b) the module, which rounds nothing
    bar = planaudit.BARS[tdt]["fused"]
    for j in range(3):
        lo = c0 + 32 * j
        med, p999, mx, _ = planaudit.stats(got[:, lo:lo + 32], want[:, lo:lo + 32])
        k = (3.0 * (j + 1)) ** 0.5
        print("chain layer %d against _DenseBlock %s: median / p99.9 / max = %.5f / %.5f / %.5f, bar %s x %.2f" % (j + 1, dtype, med, p999, mx, bar, k))
        assert med <= k * bar[0] and p999 <= k * bar[1] and mx <= k * bar[2], (j, med, p999, mx, bar, k)
    med, p999, mx, _ = planaudit.stats(got, want)
    print("chain, the whole buffer against _DenseBlock %s: median / p99.9 / max = %.5f / %.5f / %.5f" % (dtype, med, p999, mx))
    assert med <= 3 * bar[0] and p999 <= 3 * bar[1] and mx <= 3 * bar[2], (med, p999, mx, bar)


# ---- the pool and the place ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(2, 2), (5, 7), (13, 16)])
@pytest.mark.parametrize("c", (64, 256))
@pytest.mark.parametrize("dtype", DTYPES)
def test_pool_matches_the_fp32_expression(dtype, c, hw):
    import torch
    import torch.nn.functional as F
    from ssds import _native as N
    from ssds.modeling.layers import fused_conv as FC

    tdt = getattr(torch, dtype)
    h, w = hw
    g = torch.Generator().manual_seed(c + h)
    a = ((torch.rand(c, generator=g) + 0.5) * (torch.randint(0, 2, (c,), generator=g) * 2 - 1).float()).cuda()
    b = (torch.randn(c, generator=g) * 0.3).cuda()
    buf = _buffer(3, h, w, c, c + 32, tdt, seed=c * h + w)  # strided input, NaN behind the c channels
    before = buf.clone()
    want = F.avg_pool2d((buf[..., :c].float().permute(0, 3, 1, 2) * a.view(1, -1, 1, 1) + b.view(1, -1, 1, 1)).clamp(min=0), 2, 2)
    gs = G.GuardSet("cuda")
    yg = gs.out("y", (3, c, h // 2, w // 2), tdt, torch.channels_last)
    storage, bg = G.guarded(buf)
    gs.adopt("buffer", storage, bg)
    gs.arm()
    y = FC.dense_pool_native(bg, c, a, b, y=yg)
    torch.cuda.synchronize()
    assert N.last_kernel() == "dense_pool_kernel" and y.shape == want.shape and gs.problems() == []
    assert not G.has_nan(y) and G.same_bits(bg, before)
    _within(y, want, tdt, "densepool %d @%dx%d %s" % (c, h, w, dtype), kind="default")


@pytest.mark.parametrize("shape", [(2, 64, 5, 7, 256), (3, 128, 1, 1, 160), (2, 256, 13, 16, 256)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_place_is_bit_exact_between_guard_bands(dtype, shape):
    import torch
    from ssds import _native as N
    from ssds.modeling.layers import fused_conv as FC

    tdt = getattr(torch, dtype)
    n, c, h, w, ld = shape
    g = torch.Generator().manual_seed(c + ld)
    x = torch.randn(n, c, h, w, generator=g).to(tdt).cuda().contiguous(memory_format=torch.channels_last)
    buf = torch.full((n, h, w, ld), float("nan"), dtype=tdt, device="cuda")
    before = buf.clone()
    gs = G.GuardSet("cuda")
    xg = gs.inp("x", x)
    storage, bg = G.guarded(buf)
    gs.adopt("buffer", storage, bg, is_input=False)
    gs.arm()
    FC.dense_place_native(xg, bg)
    torch.cuda.synchronize()
    assert N.last_kernel() == "dense_place_kernel" and gs.problems() == []
    assert torch.equal(_bits(bg[..., :c]), _bits(x.permute(0, 2, 3, 1)))
    assert torch.equal(_bits(bg[..., c:]), _bits(before[..., c:]))


def test_a_buffer_too_narrow_for_the_layer_is_refused():
    import torch
    from ssds import _native as N
    from ssds.modeling.layers import fused_conv as FC

    pk = _layer(64, torch.bfloat16, seed=1)
    buf = _buffer(2, 5, 7, 64, 64 + 32, torch.bfloat16, seed=2)
    keep = buf.clone()
    narrow = buf.view(2, 5, 7 * 3, 32)  # pixel stride 32 < Cin + 32
    with pytest.raises(N.SsdkError, match="unsupported"):
        FC.dense_layer_native(narrow, pk)
    torch.cuda.synchronize()
    assert G.same_bits(buf, keep)


# ---- the plans ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(cases_densenet.NET_CASES))
def test_plan_matches_reference_module(name, dtype, monkeypatch):
    import torch
    from ssds.modeling.layers import fused_conv as FC
    from test_densenet_cpu import build
    from test_gpu_nets import POOL_DRAWS, SMALL, _check_against_floor, check_small_levels_pooled, floor_runs

    monkeypatch.delenv("SSDK_DENSELAYER", raising=False)
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
    assert key[0] == "image", "the DenseNet121 backbone was not part of the plan: %s" % refused
    table = plan.layer_table()
    assert len(table) == len(plan.layers)
    assert len([r for r in table if r["name"].startswith("dense ")]) == 58
    assert len([r for r in table if r["name"].startswith("densepool ")]) == 3
    assert len([r for r in table if r["name"].startswith("denseplace ")]) == 4
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
    """-> (plan, image on the device, output values): the backbone alone, recorded from the image."""
    import torch
    from ssds.modeling.layers import fused_conv as FC
    from ssds.modeling.layers import planner
    from test_densenet_cpu import build_bare

    net, x, fx = build_bare()
    net = net.eval().cuda().to(tdt)
    xd = x.cuda().to(tdt)
    plan = FC.ConvPlan(xd.device, tdt, xd.shape)
    with torch.no_grad():
        outs = planner.record_backbone(plan, plan.input_value(), net)
    return plan.finalize(), xd, outs, fx


class _Audit(planaudit.PlanAudit):
    """planaudit.PlanAudit with the reference arithmetic of the three dense ops, each in fp32 on the op's ACTUAL input."""

    def block(self, buf, n, h, w, ld):
        """[n][h][w][ld] view of a block's buffer"""
        return self.plan.arena.bufs[buf][0][: n * h * w * ld * self.plan.es].view(self.dtype).view(n, h, w, ld)

    def _ref_dense(self, i, L):
        pk, cin = L["pack"], L["cin"]
        xin = self.block(L["x"], L["n"], L["h"], L["w"], L["ld"])[self.sel][..., :cin].clone()

        def run():
            want, _ = _reference(xin, pk, self.dtype)
            return self.block(L["y"], L["n"], L["h"], L["w"], L["ld"])[self.sel][..., cin:cin + 32], want

        return run

    def _ref_densepool(self, i, L):
        import torch.nn.functional as F

        xin = self.block(L["x"], L["n"], L["h"], L["w"], L["ld"])[self.sel][..., :L["ch"]].float().permute(0, 3, 1, 2).clone()

        def run():
            want = F.avg_pool2d((xin * L["a"].view(1, -1, 1, 1) + L["b"].view(1, -1, 1, 1)).clamp(min=0), 2, 2)
            return self.view(L["y"], L["n"], L["ch"], L["h"] // 2, L["w"] // 2)[self.sel], want

        return run

    def _ref_denseplace(self, i, L):
        xin = self.take(L["x"], L["n"], L["ch"], L["h"], L["w"])

        def run():
            return self.block(L["y"], L["n"], L["h"], L["w"], L["ld"])[self.sel][..., :L["ch"]].permute(0, 3, 1, 2), xin

        return run

    def run(self):
        import torch
        from ssds import _native as N

        plan, rows = self.plan, []
        table = plan.layer_table()
        refs = {None: self._ref_conv, "stem7": self._ref_stem7, "pool": self._ref_pool, "dense": self._ref_dense,
                "densepool": self._ref_densepool, "denseplace": self._ref_denseplace}
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
                                 kind="fused" if L.get("kind") == "dense" else "default", median=med, p999=p999, max=mx, zeros=zeros))
        finally:
            torch.backends.cudnn.allow_tf32 = tf32
        return rows


@pytest.mark.parametrize("dtype", DTYPES)
def test_bare_backbone_op_by_op(dtype, monkeypatch):
    """Every op of the bare-backbone plan, launched on its own, against fp32 on the op's actual input (planaudit's bars); the place
    is exact."""
    import torch

    monkeypatch.delenv("SSDK_DENSELAYER", raising=False)
    tdt = getattr(torch, dtype)
    plan, xd, outs, _ = _bare_plan(tdt)
    rows = _Audit(plan, [xd]).run()
    print(planaudit.format_rows([dict(r, plan_kernel="") for r in rows]))
    assert len(rows) == len(plan.layers) == 2 + 58 + 3 + 4 + 3
    assert [r["kernel"] for r in rows if r["name"].startswith("dense ")] == ["dense_layer"] * 58
    assert [r["kernel"] for r in rows if r["name"].startswith("densepool ")] == ["dense_pool"] * 3
    assert [r["kernel"] for r in rows if r["name"].startswith("denseplace ")] == ["dense_place"] * 4
    assert all(r["max"] == 0 for r in rows if r["name"].startswith("denseplace "))
    assert not planaudit.failures(rows, tdt), planaudit.failures(rows, tdt)


def test_op_profiling_names_the_kernels(monkeypatch):
    import torch

    monkeypatch.delenv("SSDK_DENSELAYER", raising=False)
    plan, xd, _, _ = _bare_plan(torch.bfloat16)
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
        assert (kern == "dense_layer_kernel") == name.startswith("dense "), (kern, name)
        assert (kern == "dense_pool_kernel") == name.startswith("densepool "), (kern, name)
        assert (kern == "dense_place_kernel") == name.startswith("denseplace "), (kern, name)
        assert ms >= 0
    assert sum(n.startswith("dense ") for n in names) == 58


# ---- the switch --------------------------------------------------------------------------------------------------------------------
def test_the_switch_puts_the_backbone_back_on_torch(monkeypatch):
    """SSDK_DENSELAYER=0 (docs/SWITCHES.md; read whenever a plan is recorded): the image plan is refused with the switch's name, the
    backbone runs module by module on PyTorch-ROCm and the neck plan takes its maps.  The outputs are judged against the reference's
    fp32 outputs by the rule of tests/test_gpu_nets.py, as the default plan's are in test_plan_matches_reference_module."""
    import torch
    from ssds.modeling.layers import fused_conv as FC
    from test_densenet_cpu import build
    from test_gpu_nets import _check_against_floor, floor_runs

    name, dtype = "yolov3_dn121", "bfloat16"
    tdt = getattr(torch, dtype)
    for env in ("1", "0"):
        monkeypatch.setenv("SSDK_DENSELAYER", env)
        model, x, fx = build(name, monkeypatch)
        model = model.cuda().to(tdt)
        xd = x.cuda().to(tdt)
        with torch.no_grad():
            loc, conf = model(xd)
        torch.cuda.synchronize()
        entries = model.__dict__["_neck_plans"]
        image = [p for k, p in entries.items() if k[0] == "image"]
        assert len(image) == 1
        if env == "1":
            assert isinstance(image[0], FC.ConvPlan) and len(entries) == 1
            continue
        assert isinstance(image[0], str) and "SSDK_DENSELAYER=0" in image[0]
        necks = [p for k, p in entries.items() if k[0] != "image"]
        assert len(necks) == 1 and isinstance(necks[0], FC.ConvPlan)
        assert not [r for r in necks[0].layer_table() if r["name"].startswith("dense")]
        wl, wc = nethelp.want(fx)
        report = _check_against_floor({"loc": loc, "conf": conf}, floor_runs(model, xd), {"loc": wl, "conf": wc}, name, dtype)
        print(name, dtype, "SSDK_DENSELAYER=0", "; ".join(report))
