"""The judge of the EfficientNet training kernels (csrc/ssdk_mbconvtrain.hip behind ssds/modeling/layers/mbconvtrain.py): operands, the
fp64 truth with its absolute-value masses, the bars, the case lists, an fp32 CPU model of every pass with planted defects
(tests/test_mbconv_train_cpu.py) and the runners of tests/test_gpu_mbconv_train.py.  Not a conftest.

Operands: x, u, dy, dz ~ N(0, 1) in the dtype; w5 ~ N(0, 1) / 5 rounded, kept as an fp32 master; W1 ~ N(0, 1 / C), W2 ~ N(0, 1 / Cr),
biases ~ N(0, 1 / 4), fp32.  Truth: fp64 on the CPU from the operands as stored; the same expressions on absolute values for the masses.

Bars (u = 2^-24, eps = 2^-8 bf16 | 2^-10 fp16):
  y, dx, z, du   per element   |err| <= eps |want| + 4 eps rms(want)            (z, du against the whole fp64 function)
  dW5            per (c, tap)  |err| <= DW5_SUM_DEPTH u Mw
  pooled         per (n, c)    |err| <= (SE_POOL_DEPTH(HW) + 8) u mean|silu(u)|  (8 u: the fast exp and reciprocal, 4 u each)
  gate           per (n, c)    the derived absolute bar of mbseaudit.judge (FC depths, slopes 1.1 / 1/4), under its cap 2^-13
  dgate_raw      per (n, c)    |err| <= (SE_RED_DEPTH(HW) + 9) u sum|dz silu(u)|
  dpool, dW1, db1, dW2, db2 of ssdk_se_gate_bwd, on the stage's own inputs: D u mass with D, mass of mbconvtrain.SE_GATE_BWD_DEPTHS.
Every depth is derived next to the wrappers in ssds/modeling/layers/mbconvtrain.py and is at most dwjudge.DEPTH_CAP."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "ssds.pytorch_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

U = 2.0 ** -24
EPS = {"bf16": 2.0 ** -8, "f16": 2.0 ** -10}
DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16}
CODES = {"bf16": 1, "f16": 2}
DEPTH_CAP = 256  # dwjudge.DEPTH_CAP
GATE_CAP = 2.0 ** -13  # mbseaudit.GATE_CAP
STRIDES = (1, 2)
ONE_HOT = -1.3125

# (N, C, H, W)
DW_CASES = [(2, 3, 1, 1),                     # only the centre tap inside
            (1, 2, 2, 3),                     # map smaller than the window
            (1, 2, 5, 5),
            (2, 3, 8, 16), (2, 3, 8, 17),     # whole 16-byte rows, and one over
            (1, 2, 16, 16),
            (3, 5, 19, 19),                   # odd, several planes per workgroup
            (17, 2, 7, 7),                    # ragged last group
            (1, 2, 33, 65),                   # more than one band
            (1, 2, 64, 64),
            (1, 1, 5, 600)]                   # wide row: several column tiles
DW_ONES = [(3, 5, 19, 19), (1, 2, 33, 65)]
DW_ONEHOT = [(2, 3, 8, 17), (3, 5, 19, 19), (17, 2, 7, 7), (1, 2, 33, 65), (1, 1, 5, 600)]
DW_ALIGN = [(2, 3, 8, 17), (3, 5, 19, 19), (1, 2, 33, 65)]
# (N, C, Cr, H, W)
SE_CASES = [(1, 8, 2, 1, 1), (2, 16, 4, 7, 7), (2, 40, 10, 16, 16),
            (3, 144, 6, 9, 5),                # odd plane, C no multiple of 64
            (2, 32, 8, 33, 65),               # a workgroup per plane: several partials per plane
            (2, 1152, 48, 4, 4),
            (1, 24, 1, 3, 3),                 # Cr = 1
            (33, 8, 2, 2, 2)]
SE_ALIGN = [(2, 16, 4, 7, 7), (3, 144, 6, 9, 5), (2, 32, 8, 33, 65)]
OFFSETS = {"a": 1, "b": 3, "c": 4}  # elements into the allocation: base pointers 2-, 6- and 8-byte aligned


def sid(shape):
    return "x".join(str(v) for v in shape)


def out_hw(h, w, stride):
    return (h - 1) // stride + 1, (w - 1) // stride + 1


def M():
    from ssds.modeling.layers import mbconvtrain

    return mbconvtrain


def new_rec(what):
    return {"what": what, "ratios": {}, "lines": [], "failures": []}


def _say(rec, what, err, bar):
    worst = float((err / bar.clamp(min=1e-300)).max()) if err.numel() else 0.0
    rec["ratios"][what] = worst
    rec["lines"].append("%s %s: worst |err| / bar = %.3f" % (what, rec["what"], worst))
    bad = int((~(err <= bar)).sum())  # (a NaN is outside every bar)
    if bad:
        rec["failures"].append("%s: %d elements outside the bar, worst %.3g of it" % (what, bad, worst))


def _elem(rec, what, got, want, dt):
    want = want.double()
    err = (got.double().cpu() - want).abs()
    _say(rec, what, err, EPS[dt] * want.abs() + 4 * EPS[dt] * float(want.pow(2).mean().sqrt()))


def equal(rec, what, got, want):
    if tuple(got.shape) != tuple(want.shape) or not torch.equal(got.cpu(), want.cpu()):
        diff = int((got.cpu() != want.cpu()).sum()) if tuple(got.shape) == tuple(want.shape) else -1
        rec["failures"].append("%s: not equal (%d elements differ)" % (what, diff))


def silu(v):
    return v * torch.sigmoid(v)


def dsilu(v):
    s = torch.sigmoid(v)
    return s * (1 + v * (1 - s))


# ---- depthwise 5x5 -----------------------------------------------------------------------------------------------------------------
def dw_operands(shape, stride, dt):
    n, c, h, w = shape
    g = torch.Generator().manual_seed(500000 * stride + 1000 * n + 100 * c + 7 * h + 3 * w + CODES[dt])
    x = torch.randn(n, c, h, w, generator=g).to(DTYPES[dt])
    wt = (torch.randn(c, 1, 5, 5, generator=g) / 5).to(DTYPES[dt]).float()
    ho, wo = out_hw(h, w, stride)
    dy = torch.randn(n, c, ho, wo, generator=g).to(DTYPES[dt])
    return x, wt, dy


def _conv(x, wt, dy, stride, dtype):
    xx = x.detach().to(dtype).requires_grad_(True)
    ww = wt.detach().to(dtype).requires_grad_(True)
    y = F.conv2d(xx, ww, None, stride, 2, 1, x.shape[1])
    y.backward(dy.to(dtype))
    return y.detach(), xx.grad, ww.grad


def dw_truth(x, wt, dy, stride):
    y, dx, dw = _conv(x, wt, dy, stride, torch.float64)
    _, _, mw = _conv(x.abs(), wt.abs(), dy.abs(), stride, torch.float64)
    return {"y": y, "dx": dx, "dw": dw, "Mw": mw}


def dw_model(x, wt, dy, stride, dt, mutate=None):
    """fp32 arithmetic on the stored operands, y and dx rounded once.  ``mutate``: 'shift' (the window one column off), 'oddtaps' (the
    stride-2 input gradient without the taps of odd index), 'lastimage' (the dW sum without the last image)."""
    xs = torch.roll(x, 1, 3) if mutate == "shift" else x
    y, dx, dw = _conv(xs, wt, dy, stride, torch.float32)
    if mutate == "oddtaps" and stride == 2:
        we = wt.clone()
        we[:, :, 1::2, :] = 0
        we[:, :, :, 1::2] = 0
        dx = _conv(x, we, dy, stride, torch.float32)[1]
    if mutate == "lastimage":
        dw = _conv(x[:-1], wt, dy[:-1], stride, torch.float32)[2] if x.shape[0] > 1 else torch.zeros_like(dw)
    return {"y": y.to(DTYPES[dt]), "dx": dx.to(DTYPES[dt]), "dw": dw}


def dw_depth(shape, stride):
    return M().DW5_SUM_DEPTH(shape[0], shape[1], shape[2], shape[3], stride)


def dw_judge(rec, got, tr, dt, depth):
    for k in ("y", "dx"):
        if got.get(k) is not None:
            _elem(rec, k, got[k], tr[k], dt)
    if got.get("dw") is not None:
        _say(rec, "dW5", (got["dw"].double().cpu() - tr["dw"]).abs(), depth * U * tr["Mw"])
    return rec


def dw_one_hot_truth(x, wt, pos, stride, dt):
    """dy one-hot at ``pos``: dW[c, t] = the fp32 product dy x[window tap] (exact for 16-bit operands), dx = the product dy w[tap]
    rounded to the dtype where the window reaches, zero elsewhere -- written out by the definition."""
    n, c, oy, ox = pos
    h, w = x.shape[2:]
    val = torch.tensor(ONE_HOT, dtype=torch.float32)
    xp = F.pad(x.float(), (2, 2, 2, 2))
    dw = torch.zeros(x.shape[1], 1, 5, 5)
    dx = torch.zeros(x.shape, dtype=DTYPES[dt])
    for ky in range(5):
        for kx in range(5):
            dw[c, 0, ky, kx] = val * xp[n, c, oy * stride + ky, ox * stride + kx]
            iy, ix = oy * stride + ky - 2, ox * stride + kx - 2
            if 0 <= iy < h and 0 <= ix < w:
                dx[n, c, iy, ix] = (val * wt[c, 0, ky, kx].float()).to(DTYPES[dt])
    return dx, dw


def dw_positions(shape, stride):
    """positions of dy: the corners and centres, both sides of every multiple of 4 rows (every band seam of either plan is one),
    of every 128 / 256 columns (column tiles), and the first / last image of every group of up to 8 planes"""
    n, c, h, w = shape
    ho, wo = out_hw(h, w, stride)
    pos = {(0, 0, 0, 0), (n - 1, c - 1, ho - 1, wo - 1), (0, 0, ho - 1, 0), (0, c - 1, 0, wo - 1), (n - 1, 0, ho - 1, wo // 2),
           (n - 1, c // 2, ho // 2, wo - 1), (0, c // 2, ho // 2, wo // 2)}
    rows = sorted({v for r in range(4, ho, 4) for v in (r - 1, r)})
    if len(rows) > 8:
        rows = rows[:4] + rows[-4:]
    cols = sorted({v for q in range(64, wo, 64) for v in (q - 1, q)})
    if len(cols) > 8:
        cols = cols[:4] + cols[-4:]
    pos.update((n - 1, c - 1, r, wo // 2) for r in rows)
    pos.update((0, 0, ho // 2, q) for q in cols)
    pos.update((i, c - 1, ho // 2, wo // 2) for i in range(n) if i % 2 == 1 or i == n - 1)
    return sorted(pos)


# ---- SiLU + squeeze-excite ---------------------------------------------------------------------------------------------------------
def se_operands(case, dt):
    n, c, cr, h, w = case
    g = torch.Generator().manual_seed(7000 * n + 100 * c + 31 * cr + 7 * h + 3 * w + CODES[dt])
    u = torch.randn(n, c, h, w, generator=g).to(DTYPES[dt])
    dz = torch.randn(n, c, h, w, generator=g).to(DTYPES[dt])
    w1 = torch.randn(cr, c, generator=g) / c ** 0.5
    w2 = torch.randn(c, cr, generator=g) / cr ** 0.5
    b1 = torch.randn(cr, generator=g) * 0.5
    b2 = torch.randn(c, generator=g) * 0.5
    return {"u": u, "dz": dz, "w1": w1, "b1": b1, "w2": w2, "b2": b2}


def se_function(u, w1, b1, w2, b2):
    t = silu(u)
    pooled = t.mean((2, 3))
    hp = pooled @ w1.t() + b1
    gate = torch.sigmoid(silu(hp) @ w2.t() + b2)
    return t * gate[:, :, None, None], pooled, hp, gate


def se_truth(o):
    """fp64: every intermediate, the gradients of the whole function by autograd, and the masses."""
    d = {k: v.detach().double() for k, v in o.items()}
    leaves = {k: d[k].clone().requires_grad_(True) for k in ("u", "w1", "b1", "w2", "b2")}
    z, pooled, hp, gate = se_function(*(leaves[k] for k in ("u", "w1", "b1", "w2", "b2")))
    grads = torch.autograd.grad(z, [leaves[k] for k in ("u", "w1", "b1", "w2", "b2")], d["dz"])
    t = silu(d["u"])
    return {"z": z.detach(), "pooled": pooled.detach(), "hp": hp.detach(), "gate": gate.detach(), "du": grads[0], "dw1": grads[1],
            "db1": grads[2], "dw2": grads[3], "db2": grads[4], "draw": (d["dz"] * t).sum((2, 3)), "M_pool": t.abs().mean((2, 3)),
            "M_draw": (d["dz"] * t).abs().sum((2, 3))}


def gate_bar(pooled, dm, w1, b1, w2, b2, c, cr):
    """the derivation of mbseaudit.judge on fp64 operands: -> (bar of hidden_pre, bar of gate)"""
    d1, d2 = M().SE_FC1_DEPTH(c), M().SE_FC2_DEPTH(cr)
    z1 = pooled @ w1.t() + b1
    s = silu(z1)
    dz1 = dm @ w1.abs().t() + d1 * U * (pooled.abs() @ w1.abs().t() + b1.abs())
    ds = 1.1 * dz1 + 9 * U * z1.abs()
    dz2 = ds @ w2.abs().t() + d2 * U * (s.abs() @ w2.abs().t() + b2.abs())
    return dz1 + U * z1.abs(), dz2 / 4 + 9 * U


def gate_bwd_truth(draw, gate, pooled, hp, w1, w2):
    """fp64 outputs of ssdk_se_gate_bwd from its own inputs, and the masses of mbconvtrain.SE_GATE_BWD_DEPTHS"""
    draw, gate, pooled, hp, w1, w2 = (t.detach().double().cpu() for t in (draw, gate, pooled, hp, w1, w2))
    dv2 = draw * gate * (1 - gate)
    s = silu(hp)
    dh = (dv2 @ w2) * dsilu(hp)
    a = draw.abs() * gate * (1 - gate)
    mh = (a @ w2.abs()) * (1 + hp.abs())
    return {"dpool": dh @ w1, "dw1": dh.t() @ pooled, "db1": dh.sum(0), "dw2": dv2.t() @ s, "db2": dv2.sum(0),
            "M_dpool": mh @ w1.abs(), "M_dw1": mh.t() @ pooled.abs(), "M_db1": mh.sum(0), "M_dw2": a.t() @ hp.abs(), "M_db2": a.sum(0)}


def gate_bwd_judge(rec, got, tr, n, c, cr):
    depths = M().SE_GATE_BWD_DEPTHS(n, c, cr)
    for k in ("dpool", "dw1", "db1", "dw2", "db2"):
        g = got[k].double().cpu().reshape(tr[k].shape)
        _say(rec, k, (g - tr[k]).abs(), depths[k] * U * tr["M_" + k])
    return rec


def se_depths(case):
    n, c, cr, h, w = case
    m = M()
    d = {"pool": m.SE_POOL_DEPTH(h * w) + 8, "red": m.SE_RED_DEPTH(h * w) + 9, "fc1": m.SE_FC1_DEPTH(c), "fc2": m.SE_FC2_DEPTH(cr)}
    d.update(m.SE_GATE_BWD_DEPTHS(n, c, cr))
    return d


def se_judge(rec, got, tr, o, case, dt):
    """got: any of z, du, pooled, hp, gate, draw (whole function, against fp64)."""
    n, c, cr, h, w = case
    m = M()
    d = {k: v.detach().double() for k, v in o.items()}
    for k in ("z", "du"):
        if got.get(k) is not None:
            _elem(rec, k, got[k], tr[k], dt)
    dm = (m.SE_POOL_DEPTH(h * w) + 8) * U * tr["M_pool"]
    if got.get("pooled") is not None:
        _say(rec, "pooled", (got["pooled"].double().cpu() - tr["pooled"]).abs(), dm)
    hbar, gbar = gate_bar(tr["pooled"], dm, d["w1"], d["b1"], d["w2"], d["b2"], c, cr)
    if float(gbar.max()) > GATE_CAP:
        rec["failures"].append("the derived gate bar %.3g exceeds 2^-13" % float(gbar.max()))
    if got.get("hp") is not None:
        _say(rec, "hidden_pre", (got["hp"].double().cpu() - tr["hp"]).abs(), hbar)
    if got.get("gate") is not None:
        _say(rec, "gate", (got["gate"].double().cpu() - tr["gate"]).abs(), gbar)
    if got.get("draw") is not None:
        _say(rec, "dgate_raw", (got["draw"].double().cpu() - tr["draw"]).abs(), (m.SE_RED_DEPTH(h * w) + 9) * U * tr["M_draw"])
    return rec


def se_model(o, dt, mutate=None):
    """fp32 arithmetic on the stored operands in the kernels' stages, z and du rounded once.  ``mutate``: 'pool' (the pool less one
    pixel), 'gate' (image 0's gate used for image 1), 'nodpool' (du without the dpool / HW term), 'sigma' (silu' replaced by sigmoid),
    'dw2last' (dW2 without the last image), 'fc1tail' (the last 8 channels left out of FC1)."""
    u, dz = o["u"].float(), o["dz"].float()
    w1, b1, w2, b2 = (o[k].float() for k in ("w1", "b1", "w2", "b2"))
    n, c, h, w = u.shape
    hw = h * w
    t = silu(u)
    pooled = t.sum((2, 3)) / hw
    if mutate == "pool":
        pooled = (t.sum((2, 3)) - t[:, :, -1, -1]) / hw
    w1f = w1.clone()
    if mutate == "fc1tail":
        w1f[:, -8:] = 0
    hp = pooled @ w1f.t() + b1
    s = silu(hp)
    gate = torch.sigmoid(s @ w2.t() + b2)
    g = gate.clone()
    if mutate == "gate" and n > 1:
        g[1] = g[0]
    z = t * g[:, :, None, None]
    draw = (dz * t).sum((2, 3))
    dv2 = draw * gate * (1 - gate)
    dh = (dv2 @ w2) * dsilu(hp)
    dpool = dh @ w1
    dw2 = dv2.t() @ s
    if mutate == "dw2last":
        dw2 = dv2[:-1].t() @ s[:-1]
    back = torch.sigmoid(u) if mutate == "sigma" else dsilu(u)
    inner = dz * gate[:, :, None, None]
    if mutate != "nodpool":
        inner = inner + (dpool / hw)[:, :, None, None]
    return {"z": z.to(DTYPES[dt]), "pooled": pooled, "hp": hp, "gate": gate, "draw": draw, "dpool": dpool, "dw1": dh.t() @ pooled,
            "db1": dh.sum(0), "dw2": dw2, "db2": dv2.sum(0), "du": (inner * back).to(DTYPES[dt])}


def se_judge_all(rec, got, tr, o, case, dt):
    """the whole-function bars, and ssdk_se_gate_bwd's outputs on the judged side's OWN stage inputs (draw, gate, pooled, hp)"""
    n, c, cr, h, w = case
    se_judge(rec, got, tr, o, case, dt)
    gtr = gate_bwd_truth(got["draw"], got["gate"], got["pooled"], got["hp"], o["w1"], o["w2"])
    return gate_bwd_judge(rec, got, gtr, n, c, cr)


# ---- the block shapes of B0 ... B5 (depth conditions) ------------------------------------------------------------------------------
def backbone_blocks(name, size=512):
    """[(hidden width, Cr, k, stride, input H = W of the depthwise convolution)] of every MBConv block of a backbone at size x size"""
    from ssds.modeling import nets

    net = getattr(nets, name)(outputs=[7])
    hw = (size - 1) // 2 + 1
    rows = []
    for j in range(7):
        for blk in getattr(net, "stage%d" % (j + 1)):
            _, dw, se, _, _ = blk.parts()
            conv = dw[0]
            rows.append((conv.in_channels, se.se[1].out_channels, conv.kernel_size[0], conv.stride[0], hw))
            hw = (hw - 1) // conv.stride[0] + 1
    return rows


# ---- running the kernels -----------------------------------------------------------------------------------------------------------
def dw_native(x, wt, dy, stride):
    m = M()
    xd = x.detach().requires_grad_(True)
    wd = wt.detach().requires_grad_(True)
    y = m.dwconv5x5(xd, wd, stride)
    y.backward(dy)
    torch.cuda.synchronize()
    return {"y": y.detach(), "dx": xd.grad, "dw": wd.grad}


def dw_direct(x, w16, dy, stride, y=None, dx=None, dw=None):
    """the entry points on the calling thread -> outputs, kernel names"""
    from ssds import _native as N

    n, c, h, wd = (int(v) for v in x.shape)
    ho, wo = out_hw(h, wd, stride)
    y = torch.empty((n, c, ho, wo), device=x.device, dtype=x.dtype) if y is None else y
    dx = torch.empty_like(x) if dx is None else dx
    dw = torch.empty((c, 1, 5, 5), device=x.device, dtype=torch.float32) if dw is None else dw
    need = int(N.lib.ssdk_dwconv5_bwd_weight_workspace_bytes(n, c, h, wd, stride))
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device=x.device)
    code, sp = N.dtype_code(x), N.stream_ptr(x.device)
    names = []
    N.check(N.lib.ssdk_dwconv5_fwd(x.data_ptr(), w16.data_ptr(), y.data_ptr(), n, c, h, wd, stride, code, sp), "dwconv5_fwd")
    names.append(N.last_kernel())
    N.check(N.lib.ssdk_dwconv5_bwd_data(dy.data_ptr(), w16.data_ptr(), dx.data_ptr(), n, c, h, wd, stride, code, sp), "dwconv5_bwd_data")
    names.append(N.last_kernel())
    N.check(N.lib.ssdk_dwconv5_bwd_weight(x.data_ptr(), dy.data_ptr(), dw.data_ptr(), ws.data_ptr(), need, n, c, h, wd, stride, code, sp),
            "dwconv5_bwd_weight")
    names.append(N.last_kernel())
    torch.cuda.synchronize()
    return {"y": y, "dx": dx, "dw": dw}, names


def se_native(o):
    """through the wrapper, tensors on the device -> z, du and the parameter gradients"""
    m = M()
    leaves = {k: o[k].detach().requires_grad_(True) for k in ("u", "w1", "b1", "w2", "b2")}
    cr, c = o["w1"].shape[0], o["w1"].shape[1]
    z = m.silu_squeeze_excite(leaves["u"], leaves["w1"].view(cr, c, 1, 1), leaves["b1"], leaves["w2"].view(c, cr, 1, 1), leaves["b2"])
    z.backward(o["dz"])
    torch.cuda.synchronize()
    return {"z": z.detach(), "du": leaves["u"].grad, "dw1": leaves["w1"].grad, "db1": leaves["b1"].grad, "dw2": leaves["w2"].grad,
            "db2": leaves["b2"].grad}


def se_direct(o, z=None, du=None):
    """the six entry points in the wrapper's order on device tensors -> every stage's outputs"""
    from ssds import _native as N

    u, dz = o["u"], o["dz"]
    n, c, h, w = (int(v) for v in u.shape)
    cr, dev = int(o["w1"].shape[0]), u.device
    f32 = dict(device=dev, dtype=torch.float32)
    pooled, hp, gate = torch.empty((n, c), **f32), torch.empty((n, cr), **f32), torch.empty((n, c), **f32)
    draw, dpool = torch.empty((n, c), **f32), torch.empty((n, c), **f32)
    dw1, db1, dw2, db2 = torch.empty((cr, c), **f32), torch.empty((cr,), **f32), torch.empty((c, cr), **f32), torch.empty((c,), **f32)
    z = torch.empty_like(u) if z is None else z
    du = torch.empty_like(u) if du is None else du
    need = int(N.lib.ssdk_se_gate_bwd_workspace_bytes(n, c, cr))
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
    code, sp = N.dtype_code(u), N.stream_ptr(dev)
    w1, b1, w2, b2 = (o[k].contiguous() for k in ("w1", "b1", "w2", "b2"))
    N.check(N.lib.ssdk_se_pool_fwd(u.data_ptr(), pooled.data_ptr(), n, c, h, w, code, sp), "se_pool_fwd")
    N.check(N.lib.ssdk_se_gate_fwd(pooled.data_ptr(), w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), hp.data_ptr(),
                                   gate.data_ptr(), n, c, cr, sp), "se_gate_fwd")
    N.check(N.lib.ssdk_se_scale_fwd(u.data_ptr(), gate.data_ptr(), z.data_ptr(), n, c, h, w, code, sp), "se_scale_fwd")
    N.check(N.lib.ssdk_se_bwd_reduce(u.data_ptr(), dz.data_ptr(), draw.data_ptr(), n, c, h, w, code, sp), "se_bwd_reduce")
    N.check(N.lib.ssdk_se_gate_bwd(draw.data_ptr(), gate.data_ptr(), pooled.data_ptr(), hp.data_ptr(), w1.data_ptr(), w2.data_ptr(),
                                   dpool.data_ptr(), dw1.data_ptr(), db1.data_ptr(), dw2.data_ptr(), db2.data_ptr(), ws.data_ptr(), need,
                                   n, c, cr, sp), "se_gate_bwd")
    N.check(N.lib.ssdk_se_bwd_apply(u.data_ptr(), dz.data_ptr(), gate.data_ptr(), dpool.data_ptr(), du.data_ptr(), n, c, h, w, code, sp),
            "se_bwd_apply")
    torch.cuda.synchronize()
    return {"z": z, "pooled": pooled, "hp": hp, "gate": gate, "draw": draw, "dpool": dpool, "dw1": dw1, "db1": db1, "dw2": dw2,
            "db2": db2, "du": du}


def guarded(t, offset):
    """``t`` as a contiguous view ``offset`` elements past a 16-byte boundary inside one larger NaN-filled device allocation
    -> view, allocation, index of the view's first element"""
    per = t.numel()
    guard = (4096 + per + 7) // 8 * 8
    big = torch.full((guard + offset + per + guard,), float("nan"), dtype=t.dtype, device="cuda")
    assert big.data_ptr() % 16 == 0
    big[guard + offset:guard + offset + per] = t.reshape(-1).cuda()
    v = big[guard + offset:guard + offset + per].view(t.shape)
    assert v.is_contiguous() and v.data_ptr() == big.data_ptr() + (guard + offset) * big.element_size()
    return v, big, guard + offset


def guards_intact(big, start, per):
    return bool(torch.isnan(big[:start]).all()) and bool(torch.isnan(big[start + per:]).all())
