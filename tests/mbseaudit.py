"""Judge of the EfficientNet MBConv tail (``ssdk_mbse``, csrc/ssdk_mbse.hip), shared by tests/test_effnet_cpu.py and
tests/test_gpu_mbse.py, and the per-op audit of ``mbse`` ops in a recorded plan (what tests/planaudit.py is for the other ops).

Truth is fp64 on the CPU from the operands AS STORED, stage by stage: stage 2 is judged on the judged side's own ``t``, stage 3
on its own ``t`` and ``gate``, so the rounding of an earlier stage does not count twice.  u = 2^-24, eps = 2^-8 (bf16) | 2^-10
(fp16):

  t, y   per element      |err| <= eps |want| + 4 eps rms(want)                  (the 16-bit bar of tests/test_gpu_dense3_train.py;
                          for y it covers the re-rounded ``t * gate`` operand: about 0.1 eps rms(want) rms of extra error)
  pool   per (image, c)   |sum_T partial / (Ho Wo) - mean64(t)| <= D_pool u mean|t|,   D_pool = fused_conv.MBSE_POOL_DEPTH(T)
  gate   per (image, c)   absolute.  With m = the fp64 mean, dm = the pool bar, D1 / D2 = fused_conv.MBSE_FC1_DEPTH / FC2_DEPTH:
                            dz1 = |W1| dm + D1 u (|W1| |m| + |b1|)                    FC1 on an inexact mean, summed D1 deep
                            ds  = 1.1 dz1 + 9 u |z1|                                  SiLU: slope <= 1.1; fast exp + reciprocal (4 u
                                                                                      each) and the product's rounding, on |z1| >= |s|
                            dz2 = |W2| ds + D2 u (|W2| |s| + |b2|)
                            dg  = dz2 / 4 + 9 u                                       sigmoid: slope <= 1/4; exp, reciprocal, rounding
                          and dg must not exceed 2^-13 for the operands of a test (an eighth of fp16's rounding step below 1: the
                          gate then never shows at operand precision) -- ``judge`` reports a larger bar as a failure of its own.
"""
import torch
import torch.nn.functional as F

from ssds.modeling.layers import fused_conv as FC

U = 2.0 ** -24
EPS = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -10}
GATE_CAP = 2.0 ** -13


def out_hw(h, w, k, stride):
    return (h + 2 * (k // 2) - k) // stride + 1, (w + 2 * (k // 2) - k) // stride + 1


def operands(pk, dtype=torch.float64):
    """The pack's tensors on the CPU in ``dtype`` (values exactly as stored), in torch's layouts."""
    c = lambda v: v.detach().cpu().to(dtype)  # noqa: E731
    return dict(w_dw=c(pk.w_dw).permute(2, 0, 1).unsqueeze(1).contiguous(), scale_dw=c(pk.scale_dw), bias_dw=c(pk.bias_dw),
                w1=c(pk.w_se1), b1=c(pk.b_se1), w2=c(pk.w_se2), b2=c(pk.b_se2), w_proj=c(pk.w_proj), scale_proj=c(pk.scale_proj),
                bias_proj=c(pk.bias_proj))


def silu(v):
    return v * torch.sigmoid(v)


def stage_dw(pk, o, x):
    """x [N,C,H,W] -> t [N,C,Ho,Wo] in the dtype of ``o``'s tensors."""
    t = F.conv2d(x, o["w_dw"], None, pk.stride, pk.k // 2, 1, pk.cin)
    return silu(t * o["scale_dw"].view(1, -1, 1, 1) + o["bias_dw"].view(1, -1, 1, 1))


def stage_gate(o, mean):
    """mean [N,C] -> gate [N,C] (and the hidden layer, for the error masses)."""
    z1 = mean @ o["w1"].t() + o["b1"]
    s = silu(z1)
    return torch.sigmoid(s @ o["w2"].t() + o["b2"]), z1, s


def stage_proj(o, t, gate, residual=None, round_to=None):
    """t [N,C,Ho,Wo], gate [N,C] -> y [N,Cout,Ho,Wo]; ``round_to``: the dtype the product t * gate is rounded to first."""
    g = t * gate.view(gate.shape[0], -1, 1, 1)
    if round_to is not None:
        g = g.to(round_to).to(t.dtype)
    y = torch.einsum("nchw,oc->nohw", g, o["w_proj"])
    y = y * o["scale_proj"].view(1, -1, 1, 1) + o["bias_proj"].view(1, -1, 1, 1)
    return y if residual is None else y + residual


def reference(pk, x, residual=None, dtype=torch.float64):
    """The three stages chained in ``dtype`` without any intermediate rounding -> dict(t, mean, gate, y)."""
    o = operands(pk, dtype)
    t = stage_dw(pk, o, x.to(dtype))
    mean = t.mean((2, 3))
    gate = stage_gate(o, mean)[0]
    return dict(t=t, mean=mean, gate=gate, y=stage_proj(o, t, gate, None if residual is None else residual.to(dtype)))


def cpu_model(pk, x, residual, dtype, reround=True, mutate=None):
    """An fp32 model of the three kernels on the CPU: fp32 arithmetic on the 16-bit operands, t rounded once, the pool over t as
    stored, the product t * gate re-rounded (or not) on its way into the projection, y rounded once.  ``mutate`` plants one
    defect: 'pool' (the pool over the unrounded values with one pixel dropped), 'gate' (image 0's gate used for image 1),
    'ktail' (the last 8 channels of K skipped), 'shift' (the depthwise window shifted by one column).
    -> dict(t, pool_partial [N][1][C], gate, y) shaped like the device buffers (t, y as [N,C,H,W])."""
    o = operands(pk, torch.float32)
    x32 = x.float()
    if mutate == "shift":
        x32 = torch.roll(x32, 1, 3)
    t32 = stage_dw(pk, o, x32)
    t = t32.to(dtype)
    hw = t.shape[2] * t.shape[3]
    part = t.float().sum((2, 3))
    if mutate == "pool":
        part = t32.sum((2, 3)) - t32[:, :, 0, 0]
    gate = stage_gate(o, part / hw)[0]
    g = gate.clone()
    if mutate == "gate":
        g[1] = g[0]
    if mutate == "ktail":
        g[:, -8:] = 0
    y = stage_proj(o, t.float(), g, None if residual is None else residual.float(), round_to=dtype if reround else None)
    return dict(t=t, pool_partial=part.unsqueeze(1), gate=gate, y=y.to(dtype))


def _elem(name, got, want, eps, lines):
    want = want.double()
    err = (got.double() - want).abs()
    rms = float(want.pow(2).mean().sqrt())
    bar = eps * want.abs() + 4 * eps * rms
    worst = float((err / bar).max())
    lines.append("%s: worst |err| / bar = %.3f (rms(want) %.4g)" % (name, worst, rms))
    return [] if worst <= 1.0 else ["%s misses eps |want| + 4 eps rms(want) by a factor %.3g" % (name, worst)]


def judge(pk, x, residual, out, dtype, stages=7, lines=None):
    """``out``: dict(t [N,C,Ho,Wo], pool_partial [N][T][C], gate [N][C], y [N,Cout,Ho,Wo]) as the judged side produced them
    from x (and residual).  -> list of failures (empty: every stage is at its rounding level).  ``lines`` collects one figure
    per check."""
    lines = [] if lines is None else lines
    eps = EPS[dtype]
    o = operands(pk)
    bad = []
    t_dev = out["t"].detach().cpu().double()
    hw = t_dev.shape[2] * t_dev.shape[3]
    mean64 = t_dev.mean((2, 3))
    if stages & 1:
        bad += _elem("t", out["t"].detach().cpu(), stage_dw(pk, o, x.detach().cpu().double()), eps, lines)
        part = out["pool_partial"].detach().cpu().double()
        tiles = part.shape[1]
        got_mean = part.sum(1) / hw
        pbar = FC.MBSE_POOL_DEPTH(tiles) * U * t_dev.abs().mean((2, 3))
        perr = (got_mean - mean64).abs()
        worst = float((perr / pbar.clamp_min(1e-300)).max()) if float(pbar.max()) > 0 else float(perr.max() > 0)
        lines.append("pool: worst |err| / bar = %.3f (D_pool %d)" % (worst, FC.MBSE_POOL_DEPTH(tiles)))
        if worst > 1.0:
            bad.append("pool misses D_pool u mean|t| by a factor %.3g" % worst)
    if stages & 2:
        tiles = out["pool_partial"].shape[1]
        want, z1, s = stage_gate(o, mean64)
        dm = FC.MBSE_POOL_DEPTH(tiles) * U * t_dev.abs().mean((2, 3))
        d1, d2 = FC.MBSE_FC1_DEPTH(pk.cin), FC.MBSE_FC2_DEPTH(pk.r)
        dz1 = dm @ o["w1"].abs().t() + d1 * U * (mean64.abs() @ o["w1"].abs().t() + o["b1"].abs())
        ds = 1.1 * dz1 + 9 * U * z1.abs()
        dz2 = ds @ o["w2"].abs().t() + d2 * U * (s.abs() @ o["w2"].abs().t() + o["b2"].abs())
        gbar = dz2 / 4 + 9 * U
        gerr = (out["gate"].detach().cpu().double() - want).abs()
        worst = float((gerr / gbar).max())
        lines.append("gate: worst |err| / bar = %.3f, largest bar %.3g (cap %.3g)" % (worst, float(gbar.max()), GATE_CAP))
        if float(gbar.max()) > GATE_CAP:
            bad.append("the derived gate bar %.3g exceeds 2^-13: the summation is too deep or the operands too large" % float(gbar.max()))
        if worst > 1.0:
            bad.append("gate misses its derived bar by a factor %.3g" % worst)
    if stages & 4:
        want = stage_proj(o, t_dev, out["gate"].detach().cpu().double(), None if residual is None else residual.detach().cpu().double())
        bad += _elem("y", out["y"].detach().cpu(), want, eps, lines)
    return bad


# ---- the op inside a recorded plan ---------------------------------------------------------------------------------------------
def audit_plan(plan, inputs):
    """Every ``mbse`` op of a finalized plan launched ALONE on the plan's actual input and compared with fp32 torch arithmetic on
    the pack's folded weights (planaudit.stats; the caller holds the rows against planaudit.BARS[dtype]['fused']).  The other ops
    are launched in order so that every mbse op sees the activation the plan gives it.  -> rows like planaudit's."""
    import planaudit
    from ssds import _native as N

    plan.prepare(*inputs)
    held = list(plan._held)
    table = plan.layer_table()
    rows = []

    def view(buf, n, c, h, w):
        if isinstance(buf, FC.ExtBuf):
            return held[buf.index]
        return plan.arena.bufs[buf][0][: n * c * h * w * plan.es].view(plan.dtype).view(n, h, w, c).permute(0, 3, 1, 2)

    with torch.no_grad():
        for i, L in enumerate(plan.layers):
            if L.get("kind") != "mbse":
                plan.launch(i, i + 1)
                continue
            pk, n, h, w = L["pack"], L["n"], L["h"], L["w"]
            ho, wo = out_hw(h, w, pk.k, pk.stride)
            xin = view(L["x"], n, pk.cin, h, w).float().clone()  # copied BEFORE the launch: the arena may recycle the buffer
            res = view(L["res"], n, pk.cout, ho, wo).float().clone() if L["res"] is not None else None
            plan.launch(i, i + 1)
            torch.cuda.synchronize()
            kern = N.last_kernel()
            o = {k: v.to(xin.device) for k, v in operands(pk, torch.float32).items()}
            t = stage_dw(pk, o, xin)
            want = stage_proj(o, t, stage_gate(o, t.mean((2, 3)))[0], res)
            med, p999, mx, zeros = planaudit.stats(view(L["y"], n, pk.cout, ho, wo), want)
            rows.append(dict(index=i, name=table[i]["name"], kernel=kern.replace("_kernel", ""), kind="fused", median=med, p999=p999,
                             max=mx, zeros=zeros))
        torch.cuda.synchronize()
    return rows


# ---- the detector cases of tests/golden/cases_effnet.py ------------------------------------------------------------------------
def build_case(name):
    """nethelp.build for a case of cases_effnet.NET_CASES: this repository's detector on the CPU in fp32 with the case's seeded
    weights and the fixture's BatchNorm statistics, its ``state_dict`` schema checked against the reference's
    -> (model.eval(), image, fixture)."""
    import numpy as np

    import cases_effnet
    import nethelp
    from ssds.modeling import nets, ssds

    fx = nethelp.load_fixture(name)
    seed, head, net, fl, A, C, _ = cases_effnet.NET_CASES[name]
    cls = getattr(ssds, head)
    nets_outputs, extras, hd = cls.add_extras(feature_layer=[list(f) if isinstance(f, list) else f for f in fl],
                                              mbox=[A] * len(fl[0]), num_classes=C)
    model = cls(backbone=getattr(nets, net)(outputs=nets_outputs), extras=extras, head=hd, num_classes=C)
    ref_spec = [(str(k), tuple(int(v) for v in str(sh).split(",")) if str(sh) else ()) for k, sh in zip(fx["keys"], fx["shapes"])]
    ref = dict(ref_spec)
    mine = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    missing = [k for k in ref if k not in mine and not k.startswith(nethelp.UNUSED_TAILS)]
    assert not missing, "reference parameters this model lacks: %s" % missing[:8]
    assert not [k for k in mine if k not in ref], "parameters the reference does not have: %s" % [k for k in mine if k not in ref][:8]
    assert any(k.startswith(nethelp.UNUSED_TAILS) for k in ref), "the reference has a classifier tail: the fixture lists it"
    bad = [(k, mine[k], ref[k]) for k in mine if mine[k] != ref[k]]
    assert not bad, "shape mismatch: %s" % bad[:4]
    assert [k for k, _ in ref_spec if k in mine] == list(mine), "state_dict key order differs from the reference"
    state = cases_effnet.seeded_state(ref_spec, seed)
    for k in list(state):
        if "bn/" + k in fx:
            state[k] = fx["bn/" + k]
    model.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in state.items() if k in mine})
    return model.eval(), torch.from_numpy(cases_effnet.net_image(name)), fx


def make_block(cin, cout, expand, k, stride, seed, se_std=0.5):
    """A seeded ``MBConvBlock`` in eval mode with O(1) activations: conv weights ~ N(0, 1.5 / fan_in), squeeze-excite weights
    ~ N(0, se_std / fan_in) and biases ~ N(0, 0.1^2) (small enough for the derived gate bar to stay under its cap at C = 1152),
    non-trivial BatchNorm statistics."""
    from ssds.modeling.nets.efficientnet import MBConvBlock, PlainConv2d

    g = torch.Generator().manual_seed(seed)
    blk = MBConvBlock(cin, cout, expand, k, stride).eval()
    for m in blk.modules():
        if isinstance(m, torch.nn.Conv2d):
            fan = m.weight[0].numel()
            std = (se_std / fan) ** 0.5 if (isinstance(m, PlainConv2d) and m.bias is not None) else (1.5 / fan) ** 0.5
            m.weight.data = torch.randn(m.weight.shape, generator=g) * std
            if m.bias is not None:
                m.bias.data = torch.randn(m.bias.shape, generator=g) * 0.1
        elif isinstance(m, torch.nn.BatchNorm2d):
            m.weight.data = torch.rand(m.weight.shape, generator=g) + 0.5
            m.bias.data = torch.randn(m.bias.shape, generator=g) * 0.2
            m.running_mean.data = torch.randn(m.running_mean.shape, generator=g) * 0.2
            m.running_var.data = torch.rand(m.running_var.shape, generator=g) + 0.5
    return blk
