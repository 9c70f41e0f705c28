"""The DenseNet dense-block training step on the GPU (csrc/ssdk_densetrain.hip, ssds/modeling/layers/densetrain.py): the five entry
points against fp64 per element on EXACT operands (tests/densejudge.py), guard bands around every buffer, whole blocks in train
mode under bf16 autocast against the fp64 CPU block, graph capture, and the Solver's switch.

Bars.  16-bit results (tests/dwjudge.py): |err| <= eps |want| + 4 eps rms(want), eps 2^-8 (bf16) | 2^-10 (fp16), per element.  fp32
sums: |err| <= D u M, u = 2^-24, M the fp64 mass of the sum's terms and D the depth function of densetrain.py, derived next to it
from the kernels' summation structure.  The statistics of pw_forward: the form of tests/test_gpu_shuffle_train.py, |sum err| <=
Ds u S|y| + Dy u S(My), |sumsq err| <= Ds u S(y^2) + 2 Dy u S(|y| My).  bn1_reduce, second sum: a term g xhat carries, besides the
rounding of the product (counted in D), the two roundings of xhat = fl(fl(x - mean) invstd) -- x and mean are fp32 values, so
fl(x - mean) is the exact difference times (1 + d1), the product with invstd adds (1 + d2), |d| <= u: the term is off by at most
2 u |g xhat| (first order), hence |err| <= (D + 2) u sum |g xhat|."""
import copy
import os
import subprocess
import sys

import pytest

import densejudge as DJ
import guardband as G

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = DJ.U
CASES, DTYPE_NAMES, cid = DJ.CASES, DJ.DTYPE_NAMES, DJ.cid


def _setup(case, name):
    import torch
    from ssds import _native as N

    r = DJ.exact_case(case, name)
    dev = torch.device("cuda")
    F = r["F"].cuda()
    return r, dev, F, N.dtype_code(F)


# ---- single kernels ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", DTYPE_NAMES)
@pytest.mark.parametrize("case", CASES, ids=cid)
def test_pw_forward_and_its_statistics(case, name):
    import torch
    from ssds.modeling.layers import densetrain as DT
    from ssds.modeling.layers import shuffletrain as ST

    b, ctot, k, m, h, w = case
    r, dev, F, code = _setup(case, name)
    hw = h * w
    coef = r["coef"].cuda()
    w16, _ = ST.prepare_weights(r["w"].cuda(), F.dtype)
    runs = []
    for want_sums in (False, True, True):
        y = torch.full((b, m, h, w), float("nan"), device=dev, dtype=F.dtype)
        sums = DT.pw_forward(F.data_ptr(), ctot * hw, coef, w16, y, b, k, m, hw, code, dev, want_sums)
        runs.append((y, sums))
    torch.cuda.synchronize()
    DJ.judge16("m %s %s" % (cid(case), name), runs[0][0], r["y"], name)
    assert torch.equal(DJ.bits(runs[0][0]), DJ.bits(runs[1][0])), "the outputs with and without statistics differ"
    assert torch.equal(runs[1][1], runs[2][1]), "the statistics of two runs differ"
    assert b * ((hw + 127) // 128) <= 6  # one group per wave: pw_stats_sum_depth(1)
    ds, dy = DT.pw_stats_sum_depth(1), DT.pw_gemm_sum_depth(k)
    sums = runs[1][1]
    assert tuple(sums.shape) == (m, 2)
    DJ.judge_abs("sum", sums[:, 0], r["sums"][:, 0], ds * U * r["S_abs"] + dy * U * r["S_My"])
    DJ.judge_abs("sumsq", sums[:, 1], r["sums"][:, 1], ds * U * r["S_sq"] + 2 * dy * U * r["S_yMy"])


@pytest.mark.parametrize("name", DTYPE_NAMES)
@pytest.mark.parametrize("case", CASES, ids=cid)
def test_pw_wgrad(case, name):
    import torch
    from ssds.modeling.layers import densetrain as DT

    b, ctot, k, m, h, w = case
    r, dev, F, code = _setup(case, name)
    hw = h * w
    coef, dm = r["coef"].cuda(), r["dm"].cuda()
    runs = [DT.pw_wgrad(dm, F.data_ptr(), ctot * hw, coef, b, m, k, hw, code, dev) for _ in range(2)]
    torch.cuda.synchronize()
    assert tuple(runs[0].shape) == (m, k, 1, 1) and runs[0].dtype == torch.float32
    assert torch.equal(runs[0].view(torch.int32), runs[1].view(torch.int32)), "two calls differ"
    DJ.judge_abs("dW1 %s %s" % (cid(case), name), runs[0].view(m, k), r["dw"], DT.pw_wgrad_sum_depth(b, m, k, hw) * U * r["Mw"])


@pytest.mark.parametrize("name", DTYPE_NAMES)
@pytest.mark.parametrize("case", CASES, ids=cid)
def test_bn1_reduce_and_apply(case, name):
    import torch
    from ssds.modeling.layers import densetrain as DT

    b, ctot, k, m, h, w = case
    r, dev, F, code = _setup(case, name)
    hw = h * w
    coef, s, mean, invstd, gamma = (r[key].cuda() for key in ("coef", "s", "mean", "invstd", "gamma"))
    reds = [DT.bn1_reduce(s.data_ptr(), F.data_ptr(), ctot * hw, coef, mean, invstd, b, k, hw, code, dev) for _ in range(2)]
    torch.cuda.synchronize()
    assert tuple(reds[0].shape) == (k, 2) and torch.equal(reds[0].view(torch.int32), reds[1].view(torch.int32)), "two calls differ"
    d = DT.bn1_sum_depth(b, k, hw)
    DJ.judge_abs("sum g", reds[0][:, 0], r["red"][:, 0], d * U * r["R_g"])
    DJ.judge_abs("sum g xhat", reds[0][:, 1], r["red"][:, 1], (d + 2) * U * r["R_gx"])
    g = r["gold"].cuda()
    DT.bn1_apply(s.data_ptr(), F.data_ptr(), ctot * hw, coef, mean, invstd, gamma, r["red32"].cuda(), g.data_ptr(), ctot * hw, b, k, hw,
                 code, dev)
    torch.cuda.synchronize()
    DJ.judge16("G %s %s" % (cid(case), name), g[:, :k], r["gnew"], name)
    assert torch.equal(DJ.bits(g[:, k:].cpu()), DJ.bits(r["gold"][:, k:])), "channels >= K of G were written"


@pytest.mark.parametrize("name", DTYPE_NAMES)
@pytest.mark.parametrize("case", CASES, ids=cid)
def test_place(case, name):
    """The block's input (K channels at the front) and a layer's 32 new channels (behind them), into a buffer of 0xFFFF words: the
    slice carries the input's bits (signed zeros included), every other element keeps its 0xFFFF, and the sums are those of the
    stored values."""
    import torch
    from ssds.modeling.layers import densetrain as DT

    b, ctot, k, m, h, w = case
    r, dev, _, code = _setup(case, name)
    hw = h * w
    for off, c in ((0, k), (k, 32)):
        if off + c > ctot:
            continue
        t = DJ.SJ.tensor((b, c, h, w), DJ.DTYPES[name], 29 * k + off)
        t.view(-1)[0], t.view(-1)[-1] = -0.0, 0.0
        F = torch.full((b, ctot, h, w), -1, dtype=torch.int16, device=dev).view(DJ.DTYPES[name])
        sums = torch.full((ctot, 2), float("nan"), device=dev)
        DT.place(t.cuda(), F.data_ptr() + 2 * off * hw, ctot * hw, sums.data_ptr() + 8 * off, b, c, hw, code, dev)
        torch.cuda.synchronize()
        Fc = F.cpu()
        assert torch.equal(DJ.bits(Fc[:, off:off + c]), DJ.bits(t)), "the slice does not carry the input's bits"
        rest = torch.cat((Fc[:, :off], Fc[:, off + c:]), 1)
        assert bool((DJ.bits(rest) == -1).all()), "place wrote outside the slice"
        got = sums[off:off + c]
        assert bool(torch.isnan(torch.cat((sums[:off], sums[off + c:]))).all()), "sums of other channels were written"
        t64 = t.double()
        d = DT.place_sum_depth(b, c, hw)
        DJ.judge_abs("sum", got[:, 0], t64.sum((0, 2, 3)), d * U * t64.abs().sum((0, 2, 3)))
        DJ.judge_abs("sumsq", got[:, 1], t64.pow(2).sum((0, 2, 3)), d * U * t64.pow(2).sum((0, 2, 3)))


@pytest.mark.parametrize("name", DTYPE_NAMES)
@pytest.mark.parametrize("case", CASES[:2], ids=cid)
def test_guard_bands_of_the_five_entries(case, name):
    """Every buffer between guards; the channels >= K of F and G hold 0xFFFF (NaN): none reaches a result, none is written, and
    place writes its slice of F only."""
    import torch
    from ssds import _native as N
    from ssds.modeling.layers import shuffletrain as ST

    b, ctot, k, m, h, w = case
    r = DJ.exact_case(case, name)
    hw, dev, dt = h * w, torch.device("cuda"), DJ.DTYPES[name]
    gs = G.GuardSet(dev)
    Fh = r["F"].clone()
    Fh.view(torch.int16)[:, k:] = -1
    F = gs.inp("F", Fh)
    coef = gs.inp("coef", torch.nan_to_num(r["coef"], nan=0.0))  # (guards are compared as bytes: no NaN payload games inside)
    s, dm = gs.inp("s", r["s"]), gs.inp("dm", r["dm"])
    mean, invstd, gamma, red32 = (gs.inp(key, r[key]) for key in ("mean", "invstd", "gamma", "red32"))
    w16 = gs.inp("w16", ST.prepare_weights(r["w"].cuda(), dt)[0])
    t = gs.inp("t", r["s"][:, :32].contiguous())
    y = gs.out("m", (b, m, h, w), dt)
    sums = gs.out("sums", (m, 2), torch.float32)
    dw = gs.out("dw", (m, k), torch.float32)
    red = gs.out("red", (k, 2), torch.float32)
    psums = gs.out("place sums", (32, 2), torch.float32)
    Gh = r["gold"].clone()
    Gh.view(torch.int16)[:, k:] = -1
    gstore, gview = G.guarded(Gh.to(dev))
    gs.adopt("G", gstore, gview, is_input=False)
    F2 = gs.out("F of place", (b, ctot, h, w), dt)
    L = N.lib
    need = dict(stats=int(L.ssdk_pws_stats_workspace_bytes(b, k, m, hw)), wgrad=int(L.ssdk_pws_wgrad_workspace_bytes(b, m, k, hw)),
                bn1=int(L.ssdk_dense_train_bn1_workspace_bytes(b, k, hw)), place=int(L.ssdk_dense_train_place_workspace_bytes(b, 32, hw)))
    ws = {key: gs.out(key + " workspace", (v,), torch.uint8) for key, v in need.items()}
    gs.arm()
    code, sp, fs = N.dtype_code(F), N.stream_ptr(dev), ctot * hw
    N.check(L.ssdk_dense_train_pw_forward(F.data_ptr(), fs, coef.data_ptr(), w16.data_ptr(), int(w16.shape[1]), y.data_ptr(), sums.data_ptr(),
                                          ws["stats"].data_ptr(), need["stats"], b, k, m, hw, code, sp), "pw_forward")
    N.check(L.ssdk_dense_train_pw_wgrad(dm.data_ptr(), F.data_ptr(), fs, coef.data_ptr(), dw.data_ptr(), ws["wgrad"].data_ptr(), need["wgrad"],
                                        b, m, k, hw, code, sp), "pw_wgrad")
    N.check(L.ssdk_dense_train_bn1_reduce(s.data_ptr(), F.data_ptr(), fs, coef.data_ptr(), mean.data_ptr(), invstd.data_ptr(), red.data_ptr(),
                                          ws["bn1"].data_ptr(), need["bn1"], b, k, hw, code, sp), "bn1_reduce")
    N.check(L.ssdk_dense_train_bn1_apply(s.data_ptr(), F.data_ptr(), fs, coef.data_ptr(), mean.data_ptr(), invstd.data_ptr(), gamma.data_ptr(),
                                         red32.data_ptr(), gview.data_ptr(), fs, b, k, hw, code, sp), "bn1_apply")
    N.check(L.ssdk_dense_train_place(t.data_ptr(), F2.data_ptr() + 2 * k * hw, fs, psums.data_ptr(), ws["place"].data_ptr(), need["place"],
                                     b, 32, hw, code, sp), "place")
    torch.cuda.synchronize()
    assert gs.problems() == []
    for out in (y, sums, dw, red, psums, gview[:, :k]):
        assert not G.has_nan(out)
    assert bool((DJ.bits(gview[:, k:]) == -1).all()), "channels >= K of G were written"
    assert torch.equal(DJ.bits(F2[:, k:k + 32].cpu()), DJ.bits(r["s"][:, :32]))
    assert bool((DJ.bits(torch.cat((F2[:, :k], F2[:, k + 32:]), 1)) == -1).all()), "place wrote outside its slice of F"
    DJ.judge16("m", y, r["y"], name)
    DJ.judge16("G", gview[:, :k], r["gnew"], name)


# ---- blocks ------------------------------------------------------------------------------------------------------------------------
BLOCKS = [((3, 64, 4, 32, 0), (2, 64, 9, 7)), ((2, 128, 4, 32, 0), (2, 128, 5, 5))]


def _rel(a, b):
    return float((a.double().cpu() - b.double()).norm() / b.double().norm().clamp(min=1e-12))


def _make_block(cfg, seed):
    """A train-mode ``_DenseBlock`` with random (not dyadic) parameters and running statistics."""
    import torch
    import torch.nn as nn
    from ssds.modeling.nets.densenet import _DenseBlock

    torch.manual_seed(seed)
    block = _DenseBlock(*cfg).train()
    for mod in block.modules():
        if isinstance(mod, nn.BatchNorm2d):
            nn.init.uniform_(mod.weight, 0.5, 1.5)
            nn.init.normal_(mod.bias, 0.0, 0.3)
            nn.init.normal_(mod.running_mean, 0.0, 0.3)
            nn.init.uniform_(mod.running_var, 0.5, 1.5)
    return block


def _swapped(block, native):
    """The Solver's swaps on a copy of ``block`` on the GPU, in its order; ``native``: with use_native_dense_block."""
    from ssds.modeling.layers import densetrain as DT
    from ssds.modeling.layers.batchnorm import fuse_bn_activations, use_fast_batchnorm
    from ssds.modeling.layers.denseconv import use_native_dense3x3
    from ssds.modeling.layers.pointwise import fuse_conv_bn_statistics, use_pointwise_gemm

    m = copy.deepcopy(block).float().cuda()
    use_fast_batchnorm(m)
    fuse_bn_activations(m)
    if native:
        assert DT.use_native_dense_block(m) == 1 and type(m) is DT.TrainDenseBlock
    use_pointwise_gemm(m)
    fuse_conv_bn_statistics(m)
    use_native_dense3x3(m)
    return m


def _block_run(m, x, device, requires_grad=True):
    import torch

    x = x.to(device).to(torch.float32 if device == "cuda" else torch.float64).requires_grad_(requires_grad)
    ctx = torch.autocast("cuda", dtype=torch.bfloat16) if device == "cuda" else torch.autocast("cpu", enabled=False)
    with ctx:
        y = m(x * 1.0)  # (the block's input is not a leaf: a leaf's gradient is accumulated by a copy)
    (y.float() if device == "cuda" else y).pow(2).mean().backward()
    if device == "cuda":
        torch.cuda.synchronize()
    res = {"output": y.detach()}
    if requires_grad:
        res["input.grad"] = x.grad
    res.update({k + ".grad": p.grad for k, p in m.named_parameters() if p.requires_grad})
    res.update({k: v for k, v in m.named_buffers()})
    return res


def _check(got, want, floor, what):
    assert set(got) == set(want) == set(floor), what
    bad = []
    for k in sorted(want):
        if k.endswith("num_batches_tracked"):
            assert int(got[k]) == int(want[k]) == int(floor[k]), (what, k)
            continue
        rn, rf = _rel(got[k], want[k]), _rel(floor[k], want[k])
        print("%s %-44s rel native %.5f floor %.5f" % (what, k, rn, rf))
        if not rn <= 2.0 * rf + 0.02:
            bad.append((k, rn, rf))
    assert not bad, (what, bad)


@pytest.mark.parametrize("cfg,shape", BLOCKS, ids=lambda v: "-".join(str(i) for i in v))
def test_block_in_train_mode(cfg, shape):
    """A switched block with the Solver's swaps, train mode, bf16 autocast, against the fp64 CPU block: per tensor (output, input
    gradient, every parameter gradient, every running statistic) rel(native) <= 2 rel(floor) + 0.02, the floor being the same
    autocast block without use_native_dense_block (the rule of tests/test_gpu_shuffle_train.py::test_unit_in_train_mode)."""
    import torch
    from ssds.modeling.layers import densetrain as DT

    block = _make_block(cfg, 21)
    image = torch.randn(*shape, generator=torch.Generator().manual_seed(22))
    want = _block_run(copy.deepcopy(block).double(), image, "cpu")
    calls = dict(DT.STATS)
    got = _block_run(_swapped(block, True), image, "cuda")
    delta = {k: DT.STATS[k] - calls[k] for k in calls}
    assert delta == dict(swapped=1, native_forward=1, forward_layers=cfg[0], backward_layers=cfg[0], fallback=0), "the native path did not run"
    assert tuple(got["output"].shape) == (shape[0], cfg[1] + 32 * cfg[0], shape[2], shape[3]) and got["output"].dtype == torch.bfloat16
    calls = dict(DT.STATS)
    floor = _block_run(_swapped(block, False), image, "cuda")
    assert dict(DT.STATS) == calls, "the floor ran the native path"
    _check(got, want, floor, str(cfg))


def test_block_variants():
    """An input that needs no gradient, a frozen conv1.weight, two forward passes before the two backward passes (under the rule
    above), and eval mode: the fallback gives the module's bits."""
    import torch
    from ssds.modeling.layers import densetrain as DT

    cfg, shape = BLOCKS[0]
    block = _make_block(cfg, 23)
    image = torch.randn(*shape, generator=torch.Generator().manual_seed(24))
    # the input needs no gradient
    got = _block_run(_swapped(block, True), image, "cuda", requires_grad=False)
    assert "input.grad" not in got
    _check(got, _block_run(copy.deepcopy(block).double(), image, "cpu", False), _block_run(_swapped(block, False), image, "cuda", False),
           "no input grad")
    # the second layer's conv1 weight frozen
    frozen = copy.deepcopy(block)
    frozen.denselayer2.conv1.weight.requires_grad_(False)
    got = _block_run(_swapped(frozen, True), image, "cuda")
    assert "denselayer2.conv1.weight.grad" not in got and "input.grad" in got
    _check(got, _block_run(copy.deepcopy(frozen).double(), image, "cpu"), _block_run(_swapped(frozen, False), image, "cuda"), "frozen weight")

    # two forward passes, then two backward passes
    def twice(m, device):
        dt = torch.float32 if device == "cuda" else torch.float64
        xs = [(image * s).to(device).to(dt).requires_grad_(True) for s in (1.0, 0.5)]
        ctx = torch.autocast("cuda", dtype=torch.bfloat16) if device == "cuda" else torch.autocast("cpu", enabled=False)
        with ctx:
            ys = [m(x * 1.0) for x in xs]
        for y in ys:
            y.double().pow(2).mean().backward()
        res = {"input%d.grad" % i: x.grad for i, x in enumerate(xs)}
        res.update({"output%d" % i: y.detach() for i, y in enumerate(ys)})
        res.update({k + ".grad": p.grad for k, p in m.named_parameters()})
        res.update({k: v for k, v in m.named_buffers()})
        return res

    calls = dict(DT.STATS)
    got = twice(_swapped(block, True), "cuda")
    assert (DT.STATS["forward_layers"] - calls["forward_layers"], DT.STATS["backward_layers"] - calls["backward_layers"]) == (6, 6)
    _check(got, twice(copy.deepcopy(block).double(), "cpu"), twice(_swapped(block, False), "cuda"), "two forwards")
    # eval mode
    native, plain = _swapped(block, True).eval(), _swapped(block, False).eval()
    x = image.cuda()
    calls, reasons = dict(DT.STATS), DT.FALLBACK_REASONS["eval mode"]
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        a, b = native(x), plain(x)
    torch.cuda.synchronize()
    assert a.dtype == b.dtype and torch.equal(a, b)
    assert DT.STATS["fallback"] == calls["fallback"] + 1 and DT.FALLBACK_REASONS["eval mode"] == reasons + 1
    assert DT.STATS["native_forward"] == calls["native_forward"]


def test_graph_capture_replays_a_block():
    """Forward + backward of the switched 3-layer block captured in a torch.cuda.graph (one stream, no parallel branches) and
    replayed with two inputs: outputs and gradients equal the eager runs bit for bit."""
    import torch

    cfg, shape = BLOCKS[0]
    m = _swapped(_make_block(cfg, 25), True)
    for mod in m.modules():
        if hasattr(mod, "momentum") and hasattr(mod, "running_mean"):
            mod.momentum = 0.0  # (the running statistics are not part of what is compared; they stay put across the runs)
    params = [p for p in m.parameters()]
    inputs = [torch.randn(*shape, generator=torch.Generator().manual_seed(s)).bfloat16() for s in (1, 2)]
    x = inputs[0].clone().cuda().requires_grad_(True)

    def step():
        with torch.autocast("cuda", dtype=torch.bfloat16):
            y = m(x)
        grads = torch.autograd.grad(y.float().pow(2).mean(), [x] + params)
        return (y,) + tuple(grads)

    eager = []
    for inp in inputs:
        with torch.no_grad():
            x.copy_(inp)
        eager.append([t.detach().clone() for t in step()])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up on a side stream, as torch.cuda.graph asks
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step()
    for i in (1, 0):
        with torch.no_grad():
            x.copy_(inputs[i])
        graph.replay()
        torch.cuda.synchronize()
        for j, (got, want) in enumerate(zip(outs, eager[i])):
            same = torch.equal(got.view(torch.int16 if got.element_size() == 2 else torch.int32),
                               want.view(torch.int16 if want.element_size() == 2 else torch.int32))
            assert same, (i, j)


# ---- the switch ----------------------------------------------------------------------------------------------------------------------
_SWITCH = r"""
import sys, math, torch
sys.path[:0] = [%(root)r, %(pkg)r]
from ssds.core import config
from ssds.utils import train_ddp
from ssds.modeling.layers import densetrain as DT
from ssds.modeling.nets.densenet import _DenseBlock
cfg = config.cfg_from_file(%(cfg)r)
s = train_ddp.Solver(cfg, 0, torch.device("cuda", 0))
net = s.model
net.train()
x = torch.randn(2, 3, %(size)d, %(size)d, device="cuda")
with torch.autocast("cuda", dtype=torch.bfloat16):
    loc, conf = net(x)
loss = sum(o.float().pow(2).mean() for o in tuple(loc) + tuple(conf))
s.optimizer.zero_grad()
loss.backward()
s.optimizer.step()
torch.cuda.synchronize()
grads = [p.grad for p in net.parameters() if p.grad is not None]
finite = math.isfinite(float(loss)) and all(bool(torch.isfinite(g).all()) for g in grads)
blocks = [m for m in net.modules() if isinstance(m, _DenseBlock)]
print("RESULT", len(blocks), sum(type(m) is DT.TrainDenseBlock for m in blocks), DT.STATS["swapped"], DT.STATS["native_forward"],
      DT.STATS["forward_layers"], DT.STATS["backward_layers"], DT.STATS["fallback"], int(finite), len(grads))
"""


@pytest.mark.parametrize("cfg_name", ["fpn_densenet121_640.yml", "yolov3_densenet121_416.yml", "ssd_mobilenetv2_512.yml"])
@pytest.mark.parametrize("switch", ["0", "1"])
def test_the_switch(cfg_name, switch):
    """The Solver-built model of each shipped DenseNet config takes one training step (forward, backward, optimizer) at batch 2 and
    image size 128 (256 for the other backbone), in a subprocess: with SSDK_DENSE_TRAIN=1 the four blocks are TrainDenseBlock and run natively (58 layers forward
    and backward) with a finite loss and finite gradients; with 0 every counter is zero.  A model on another backbone is untouched by
    either value."""
    env = dict(os.environ, SSDK_DENSE_TRAIN=switch)
    code = _SWITCH % dict(root=ROOT, pkg=os.path.join(ROOT, "ssds.pytorch_amd"), cfg=os.path.join(ROOT, "experiments", "cfgs", cfg_name),
                        size=128 if "densenet" in cfg_name else 256)
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    res = [int(v) for v in [l for l in out.stdout.splitlines() if l.startswith("RESULT")][-1].split()[1:]]
    nblocks, nswapped, swapped, nf, fl, bl, fb, finite, ngrads = res
    assert finite == 1 and ngrads > 0
    if "densenet" not in cfg_name:
        assert res[:7] == [0] * 7
    elif switch == "0":
        assert nblocks == 4 and res[1:7] == [0] * 6
    else:
        assert (nblocks, nswapped, swapped, nf, fl, bl, fb) == (4, 4, 4, 4, 58, 58, 0)
