"""The DarkNet residual block as one launch (csrc/ssdk_dkres.hip behind fused_conv.dkres_native) and the DarkNet53 plans on the GPU.

Kernel: against the block's expression in fp32 on the same 16-bit input and the pack's folded 16-bit weights, the intermediate map
rounded to the tensor dtype as the two-launch path stores it (what planaudit's ``xpair`` row does), with planaudit's bars for a fused
op -- (median, p99.9, max) of |err| / rms: bf16 2e-3 / 0.03 / 0.1, fp16 4e-4 / 6e-3 / 0.03.  The maps come from the kernel's own tile
(include/ssdk_dkres.h SSDK_DKRES_TILE_H x _W): one pixel, 3 x 2, smaller than a tile both ways, (TH + 3) x (2 TW + 1) -- ragged both
ways with more than one tile each way -- and 13 x 13.

Models: the recorded plan against the reference's fp32 outputs (tests/golden/net_*dk53*.npz) by the rule of tests/test_gpu_nets.py --
the floor of PyTorch-ROCm running the same module in the same dtype; the bare backbone op by op against fp32 on each op's input."""
import pytest

import cases_darknet
import guardband as G
import nethelp
import planaudit

pytestmark = pytest.mark.gpu

DTYPES = ["bfloat16", "float16"]


def _widths():
    """Every C the predicate accepts (multiples of 8 up to 2048; H, W and the dtype are the predicate's other arguments)."""
    from ssds import _native as N

    return [c for c in range(8, 2049, 8) if N.lib.ssdk_dkres_supported(c, 13, 13, N.BF16)]


def _maps():
    from ssds import _native as N

    th, tw = N.DKRES_TILE_H, N.DKRES_TILE_W
    return [(1, 1), (3, 2), (th - 3, tw - 9), (th + 3, 2 * tw + 1), (13, 13)]


WIDTHS = (64, 128, 256)  # parametrisation only: test_the_parametrisation_covers_the_predicate holds it against the predicate
MAPS = range(5)


def test_the_parametrisation_covers_the_predicate():
    from ssds import _native as N

    assert tuple(_widths()) == WIDTHS and len(_maps()) == len(MAPS)
    th, tw = N.DKRES_TILE_H, N.DKRES_TILE_W
    small, ragged = _maps()[2], _maps()[3]
    assert 0 < small[0] < th and 0 < small[1] < tw and ragged[0] > th and ragged[0] % th and ragged[1] > tw and ragged[1] % tw
    for c in WIDTHS:
        for dt in (N.BF16, N.F16):
            assert all(N.lib.ssdk_dkres_supported(c, h, w, dt) for h, w in _maps())


def _gain(h, w):
    """On a small map most taps of the 3x3 fall outside the image and the branch shrinks with them: sqrt(9 / mean taps inside), which
    the second BatchNorm's weight is scaled by so that the branch keeps the size of x on every map (1 on a large map, 3 on 1 x 1)."""
    taps = sum(min(y + 1, h - 1) - max(y - 1, 0) + 1 for y in range(h)) * sum(min(x + 1, w - 1) - max(x - 1, 0) + 1 for x in range(w))
    return (9.0 * h * w / taps) ** 0.5


def _block(c, dtype, seed, bias1=None, gain2=1.0):
    """(p1, p2): packs of a Residual of width c with seeded weights and BatchNorm statistics (cases.seeded_state's distributions;
    ``gain2`` scales the second BatchNorm's weight)."""
    import torch
    from ssds.modeling.layers import fused_conv as FC
    from ssds.modeling.nets.darknet import Residual

    g = torch.Generator().manual_seed(seed)
    blk = Residual(c).eval()
    with torch.no_grad():
        for seq in (blk.conv1x1, blk.conv3x3):
            conv, bn = seq[0], seq[1]
            fan_in = conv.in_channels * conv.kernel_size[0] * conv.kernel_size[1]
            conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) * (1.5 / fan_in) ** 0.5)
            conv.bias.copy_(torch.randn(conv.bias.shape, generator=g) * 0.1)
            bn.weight.copy_((torch.rand(bn.weight.shape, generator=g) + 0.5) * (gain2 if seq is blk.conv3x3 else 1.0))
            bn.bias.copy_(torch.randn(bn.bias.shape, generator=g) * 0.1)
            bn.running_mean.copy_(torch.randn(bn.running_mean.shape, generator=g) * 0.1)
            bn.running_var.copy_(torch.rand(bn.running_var.shape, generator=g) * 0.5 + 0.5)
    blk = blk.cuda()
    p1 = FC.ConvPack(blk.conv1x1[0], blk.conv1x1[1], "relu6", dtype)
    p2 = FC.ConvPack(blk.conv3x3[0], blk.conv3x3[1], "relu6", dtype)
    if bias1 is not None:
        p1.bias.fill_(bias1)
    return p1, p2


def _input(n, c, h, w, dtype, seed):
    import torch

    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(n, c, h, w, generator=g) * 0.7).to(dtype).cuda()  # rms 0.7: the level of the backbone's own block inputs
    return x.contiguous(memory_format=torch.channels_last)


def _reference(x, p1, p2, pad_value=0.0):
    """fp32 on the 16-bit input and the packs' 16-bit weights -> (y, branch).  ``pad_value``: what the 3x3 sees outside the image
    (0: the block; anything else: the WRONG block that a kernel computing its halo from the bias alone would produce)."""
    import torch
    import torch.nn.functional as F

    tf32 = torch.backends.cudnn.allow_tf32
    torch.backends.cudnn.allow_tf32 = False
    try:
        xf = x.float()
        m = F.conv2d(xf, p1.w.float().permute(0, 3, 1, 2).contiguous())
        m = planaudit.act_fn(m * p1.scale.view(1, -1, 1, 1) + p1.bias.view(1, -1, 1, 1), p1.act).to(x.dtype).float()
        m = F.pad(m, (1, 1, 1, 1), value=pad_value)
        br = F.conv2d(m, p2.w.float().permute(0, 3, 1, 2).contiguous())
        br = planaudit.act_fn(br * p2.scale.view(1, -1, 1, 1) + p2.bias.view(1, -1, 1, 1), p2.act)
        return br + xf, br
    finally:
        torch.backends.cudnn.allow_tf32 = tf32


def _within(got, want, dtype, what):
    med, p999, mx, _ = planaudit.stats(got, want)
    bar = planaudit.BARS[dtype]["fused"]
    print(what, "median / p99.9 / max = %.5f / %.5f / %.5f of the RMS, bar %s" % (med, p999, mx, bar))
    assert med <= bar[0] and p999 <= bar[1] and mx <= bar[2], (what, med, p999, mx, bar)


# ---- the kernel --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mi", MAPS)
@pytest.mark.parametrize("c", WIDTHS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_kernel_matches_the_fp32_expression(dtype, c, mi):
    import torch
    from ssds import _native as N
    from ssds.modeling.layers import fused_conv as FC

    tdt = getattr(torch, dtype)
    h, w = _maps()[mi]
    p1, p2 = _block(c, tdt, seed=c + mi, gain2=_gain(h, w))
    x = _input(2, c, h, w, tdt, seed=17 * c + mi)
    want, br = _reference(x, p1, p2)
    # the comparison decides something: the branch is of the size of x, neither dead nor saturated
    rms = lambda t: float(t.float().pow(2).mean().sqrt())
    assert rms(br) >= 0.5 * rms(x), (rms(br), rms(x))
    assert 0.05 <= float((br == 0).float().mean()) <= 0.95 and float((br == 6).float().mean()) < 0.5
    y = FC.dkres_native(x, p1, p2)
    torch.cuda.synchronize()
    assert N.last_kernel() == "dkres_kernel" and y.shape == x.shape and y.dtype == tdt
    assert y.is_contiguous(memory_format=torch.channels_last)
    _within(y, want, tdt, "dkres %d @%dx%d %s" % (c, h, w, dtype))


@pytest.mark.parametrize("frag", [True, False])
def test_both_weight_layouts(frag, monkeypatch):
    """The fragment-major images and the KRSC tensors are two instances of the kernel: the same bits."""
    import torch
    from ssds.modeling.layers import fused_conv as FC

    p1, p2 = _block(128, torch.bfloat16, seed=5)
    x = _input(2, 128, 11, 33, torch.bfloat16, seed=6)
    want, _ = _reference(x, p1, p2)
    monkeypatch.setattr(FC, "USE_WFRAG", frag)
    assert (p1.frag() is not None) == frag and (p2.frag() is not None) == frag
    y = FC.dkres_native(x, p1, p2)
    _within(y, want, torch.bfloat16, "dkres 128 frag=%s" % frag)
    monkeypatch.setattr(FC, "USE_WFRAG", not frag)
    p1._frag = p2._frag = None
    assert torch.equal(y, FC.dkres_native(x, p1, p2))


@pytest.mark.parametrize("c", WIDTHS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_the_halo_outside_the_image_is_zero_not_the_bias(dtype, c):
    """bias1 = +3 on every channel and x = 0: the intermediate map is 3 everywhere inside the image.  A kernel that fills the halo
    outside the image with act1(bias1) is wrong by O(1) on every border pixel and right inside."""
    import torch
    from ssds import _native as N
    from ssds.modeling.layers import fused_conv as FC

    tdt = getattr(torch, dtype)
    h, w = N.DKRES_TILE_H + 3, 2 * N.DKRES_TILE_W + 1
    p1, p2 = _block(c, tdt, seed=c, bias1=3.0)
    x = torch.zeros(2, c, h, w, dtype=tdt, device="cuda").contiguous(memory_format=torch.channels_last)
    want, _ = _reference(x, p1, p2)
    wrong, _ = _reference(x, p1, p2, pad_value=3.0)
    border = torch.ones(h, w, dtype=torch.bool, device="cuda")
    border[1:-1, 1:-1] = False
    rms = float(want.pow(2).mean().sqrt())
    assert float((wrong - want)[:, :, border].abs().mean()) > 0.2 * rms > 0  # the wrong halo shows, on the border ...
    assert float((wrong - want)[:, :, ~border].abs().max()) <= 1e-5 * rms     # ... and only there
    y = FC.dkres_native(x, p1, p2)
    _within(y[:, :, border], want[:, :, border], tdt, "border %d %s" % (c, dtype))
    _within(y[:, :, ~border], want[:, :, ~border], tdt, "interior %d %s" % (c, dtype))


@pytest.mark.parametrize("shape", [(3, 64, 5, 7), (2, 256, 11, 33), (2, 128, 5, 7)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_guard_bands(dtype, shape):
    """y fully written; the guards around y, x, both weights (KRSC and fragment images) and the four vectors intact; no NaN of a
    guard reaches y; the same bits as on ordinary allocations."""
    import torch
    from ssds.modeling.layers import fused_conv as FC

    tdt = getattr(torch, dtype)
    n, c, h, w = shape
    p1, p2 = _block(c, tdt, seed=c + h)
    x = _input(n, c, h, w, tdt, seed=h * w)
    clean = FC.dkres_native(x, p1, p2)
    gs = G.GuardSet("cuda")
    xg = gs.inp("x", x)
    for tag, pk in (("p1.", p1), ("p2.", p2)):
        moved = G.guard_pack(pk)
        assert {"w", "scale", "bias", "w_frag"} <= {name for name, _, _ in moved}
        for name, storage, view in moved:
            gs.adopt(tag + name, storage, view)
    yg = gs.out("y", (n, c, h, w), tdt, torch.channels_last)
    gs.arm()
    y = FC.dkres_native(xg, p1, p2, y=yg)
    torch.cuda.synchronize()
    assert y.data_ptr() == yg.data_ptr()
    assert gs.problems() == []
    assert not G.has_nan(yg) and G.same_bits(yg, clean)


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


def test_capture_and_replay_through_a_graph():
    import torch
    from ssds.modeling.layers import fused_conv as FC

    p1, p2 = _block(128, torch.float16, seed=11)
    x = _input(2, 128, 11, 33, torch.float16, seed=12)
    eager = FC.dkres_native(x, p1, p2)
    y = torch.zeros_like(eager)
    graph = _capture(lambda: FC.dkres_native(x, p1, p2, y=y))
    y.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(y, eager)
    x.copy_(torch.flip(x, dims=[2, 3]).clone())  # new contents in the captured buffer
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(y, FC.dkres_native(x, p1, p2)) and not torch.equal(y, eager)


@pytest.mark.parametrize("c", WIDTHS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_fused_against_two_launches(dtype, c):
    """On the same packs the one launch and the two ssdk_conv launches differ by rounding only (the two launches round the branch
    before the add, and their accumulation order differs): the same bars, no bit equality."""
    import torch
    from ssds.modeling.layers import fused_conv as FC

    tdt = getattr(torch, dtype)
    p1, p2 = _block(c, tdt, seed=3 * c)
    x = _input(2, c, 13, 13, tdt, seed=c + 1)
    fused = FC.dkres_native(x, p1, p2)
    mid = FC.conv_native(x, p1)
    two = FC.conv_native(mid, p2, residual=x, res_mode=0)
    assert two.shape == fused.shape
    _within(fused, two, tdt, "fused vs two launches %d %s" % (c, dtype))
    want, _ = _reference(x, p1, p2)
    _within(two, want, tdt, "two launches vs fp32 %d %s" % (c, dtype))


def test_in_place_is_refused():
    import torch
    from ssds import _native as N
    from ssds.modeling.layers import fused_conv as FC

    p1, p2 = _block(64, torch.bfloat16, seed=1)
    x = _input(2, 64, 5, 7, torch.bfloat16, seed=2)
    keep = x.clone()
    with pytest.raises(N.SsdkError, match="overlaps"):
        FC.dkres_native(x, p1, p2, y=x)
    torch.cuda.synchronize()
    assert torch.equal(x, keep)


# ---- the plans ---------------------------------------------------------------------------------------------------------------------
def _build(name, monkeypatch):
    monkeypatch.setattr(nethelp, "cases", cases_darknet)
    return nethelp.build(name)


def _routed(h, w, dtype_code):
    """(C, H, W) of the residual blocks of DarkNet53 on an h x w image that the plan routes to the fused kernel."""
    from ssds import _native as N
    from ssds.modeling.layers import fused_conv as FC
    from test_darknet_cpu import _residuals

    return [r for r in _residuals(h, w) if N.lib.ssdk_dkres_supported(r[0], r[1], r[2], dtype_code) and r[0] in FC.DKRES_DEFAULT_WIDTHS]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(cases_darknet.NET_CASES))
def test_plan_matches_reference_module(name, dtype, monkeypatch):
    import torch
    from ssds import _native as N
    from ssds.modeling.layers import fused_conv as FC
    from test_gpu_nets import POOL_DRAWS, SMALL, _check_against_floor, check_small_levels_pooled, floor_runs

    monkeypatch.delenv("SSDK_DKRES", raising=False)
    tdt = getattr(torch, dtype)
    model, x, fx = _build(name, monkeypatch)
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
    assert key[0] == "image", "the DarkNet53 backbone was not part of the plan: %s" % refused
    table = plan.layer_table()
    assert len(table) == len(plan.layers)
    want_rows = _routed(x.shape[2], x.shape[3], N._DTYPES[tdt])
    assert len([r for r in table if r["name"].startswith("dkres ")]) == len(want_rows)
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
    cpu_model, _, _ = _build(name, monkeypatch)
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


def _bare_plan(tdt, net=None, x=None):
    """-> (plan, image on the device, output values): the backbone alone, recorded from the image."""
    import torch
    from ssds.modeling.layers import fused_conv as FC
    from ssds.modeling.layers import planner
    from test_darknet_cpu import build_bare

    if net is None:
        net, x, _ = build_bare()
    net = net.eval().cuda().to(tdt)
    xd = x.cuda().to(tdt)
    plan = FC.ConvPlan(xd.device, tdt, xd.shape)
    with torch.no_grad():
        outs = planner.record_backbone(plan, plan.input_value(), net)
    return plan.finalize(), xd, outs


class _Audit(planaudit.PlanAudit):
    """planaudit.PlanAudit with the reference arithmetic of the dkres op: the block in fp32 on the op's ACTUAL input."""

    def _ref_dkres(self, i, L):
        p1, p2 = L["pack"], L["pack2"]
        xin = self.view(L["x"], L["n"], p1.cin, L["h"], L["w"])[self.sel].clone()

        def run():
            want, _ = _reference(xin, p1, p2)
            return self.view(L["y"], L["n"], p2.cout, L["h"], L["w"])[self.sel], want

        return run

    def run(self):
        import torch
        from ssds import _native as N

        plan, rows = self.plan, []
        table = plan.layer_table()
        refs = {None: self._ref_conv, "dkres": self._ref_dkres}
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
                                 kind="fused" if L.get("kind") == "dkres" else "default", median=med, p999=p999, max=mx, zeros=zeros))
        finally:
            torch.backends.cudnn.allow_tf32 = tf32
        return rows


@pytest.mark.parametrize("dtype", DTYPES)
def test_bare_backbone_op_by_op(dtype, monkeypatch):
    """Every op of the bare-backbone plan, launched on its own, against fp32 on the op's actual input (planaudit's bars)."""
    import torch

    monkeypatch.setenv("SSDK_DKRES", "1")  # every width the predicate takes, whatever the default routing
    tdt = getattr(torch, dtype)
    plan, xd, outs = _bare_plan(tdt)
    rows = _Audit(plan, [xd]).run()
    print(planaudit.format_rows([dict(r, plan_kernel="") for r in rows]))
    assert len(rows) == len(plan.layers) == 1 + 5 + 11 + 2 * 12
    assert [r["kernel"] for r in rows if r["name"].startswith("dkres ")] == ["dkres"] * 11
    assert not planaudit.failures(rows, tdt), planaudit.failures(rows, tdt)


def test_op_profiling_names_the_kernel(monkeypatch):
    import torch

    monkeypatch.setenv("SSDK_DKRES", "1")
    plan, xd, _ = _bare_plan(torch.bfloat16)
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
        assert (kern == "dkres_kernel") == name.startswith("dkres "), (kern, name)
        assert ms >= 0
    assert sum(n.startswith("dkres ") for n in names) == 11


# ---- the switch --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_ssdk_dkres_switch(dtype, monkeypatch):
    """SSDK_DKRES=0 (docs/SWITCHES.md; read at every recording): no dkres row, two convs per block in its place.  The outputs are
    compared where ONE block separates the two plans (level 1 of the backbone): the bars are those of one op, and behind several
    blocks the two roundings of every block would have compounded."""
    import torch
    from ssds.modeling.nets.darknet import DarkNet

    tdt = getattr(torch, dtype)
    x = torch.rand(2, 3, 40, 56, generator=torch.Generator().manual_seed(5))
    outs = {}
    for env in ("1", "0"):
        monkeypatch.setenv("SSDK_DKRES", env)
        net = DarkNet(layers=[1, 1, 1, 1, 1], outputs=[1])
        spec = [(k, tuple(v.shape)) for k, v in net.state_dict().items()]
        net.load_state_dict({k: torch.from_numpy(v) for k, v in cases_darknet.seeded_state(spec, 7).items()})
        plan, xd, vals = _bare_plan(tdt, net, x)
        names = [r["name"] for r in plan.layer_table()]
        assert sum(n.startswith("dkres ") for n in names) == (1 if env == "1" else 0)
        assert len(names) == (3 if env == "1" else 4)
        with torch.no_grad():
            plan.run(xd)
        torch.cuda.synchronize()
        (buf, n, c, h, w), = vals
        assert (n, c, h, w) == (2, 64, 20, 28)
        outs[env] = planaudit.PlanAudit.view(_View(plan, tdt), buf, n, c, h, w).float().clone()
    assert float(outs["1"].std()) > 0.1 and float((outs["1"] == 0).float().mean()) < 0.5
    _within(outs["0"], outs["1"], tdt, "SSDK_DKRES=0 against =1, %s" % dtype)
    # the whole backbone: not one dkres op is left
    monkeypatch.setenv("SSDK_DKRES", "0")
    plan, _, _ = _bare_plan(tdt)
    assert not [r for r in plan.layer_table() if r["name"].startswith("dkres ")] and len(plan.layers) == 1 + 5 + 46


class _View(object):
    """What planaudit.PlanAudit.view reads of its ``self``: the plan and its dtype."""

    def __init__(self, plan, dtype):
        self.plan, self.dtype = plan, dtype
