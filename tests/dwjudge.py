"""The judge of the depthwise 3x3 training kernels (csrc/ssdk_dwplane.hip: whole rows; csrc/ssdk_dwtrain.hip: 32 x 64 tiles) behind
ssds/modeling/layers/dwconv.py: operands, the fp64 truth with its absolute-value masses, the bars, the case lists and the checks
that tests/test_gpu_dwtrain.py runs in process and -- for the tiled kernels that SSDK_DW_PLANE=0 selects, a switch the library reads
once per process -- in ONE child process (``python tests/dwjudge.py --family tiled`` prints one ``RESULT`` JSON line).
tests/test_dwjudge_cpu.py turns the judge on an fp32 CPU model of the passes and on mutations of it.  Not a conftest.

Operands: x, dy ~ N(0, 1) in the dtype; w [C,1,3,3] ~ N(0, 1) / 3 rounded to the dtype, kept as the fp32 master tensor holding the
rounded values (``_DwConv3x3`` then returns an fp32 dW); nothing is rounded in the fp32 cases.  Truth: ``F.conv2d(groups=C)`` under
autograd in fp64 on the CPU on those operands, and the same convolution on |x|, |w|, |dy| for the masses My, Mdx, Mw.

Bars (u = 2^-24):
  y, dx 16 bit   per element   |err| <= eps |want| + 4 eps rms(want), eps = 2^-8 bf16, 2^-10 fp16 (tests/test_gpu_dense3_train.py)
  y, dx fp32     per element   |err| <= 16 u M, M the element's mass (nine fp32 products added in any order)
  dW             per (c, tap)  |err| <= DW_SUM_DEPTH u Mw[c,t]
  sums[:,0]      per channel   |err| <= DW_STATS_DEPTH u sum|y| + 16 u sum My           (against the fp64 sums of the unrounded y)
  sums[:,1]      per channel   |err| <= DW_STATS_DEPTH u sum y^2 + 2 * 16 u sum |y| My
The two depths are derived next to ``_DwConv3x3`` in ssds/modeling/layers/dwconv.py.  No other tolerance exists here; the exact
checks (all ones, one-hot gradients, bit equality under misalignment) have none."""
import ctypes
import json
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
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
CODES = {"f32": 0, "bf16": 1, "f16": 2}  # include/ssdk.h SSDK_F32 | SSDK_BF16 | SSDK_F16
DEPTH_CAP = 256
STRIDES = (1, 2)
PLAN_NAMES = ("G", "T", "TR", "seg", "LD", "SR", "CH", "UP", "nwg", "groups", "lds", "Ht")
WHOLE_NAMES = ["dwp_fwd_kernel", "dwp_dgrad_kernel", "dwp_wgrad_kernel"]
TILED_NAMES = ["dw_fwd_kernel", "dw_dgrad_kernel", "dw_wgrad_reduce_kernel"]
ONE_HOT = -1.3125

# (N, C, H, W)
WHOLE_ROW = [(3, 5, 1, 1), (2, 3, 2, 3), (2, 4, 7, 9),      # smallest planes
             (2, 3, 8, 16), (2, 3, 8, 17),                   # exactly two eight-pixel segments, and one pixel over
             (27, 4, 19, 19), (70, 2, 10, 10),               # several images per workgroup, ragged last group
             (2, 4, 150, 150), (1, 2, 151, 149),             # row bands; ragged last band, odd sizes under the stride-2 row pairing
             (1, 2, 5, 1000),                                # widest row
             (2, 2, 3, 3000)]                                # 16 bit stays on this family; fp32 does not fit the LDS budget
WIDE = (2, 2, 3, 3000)
TILED_SWITCH = [(1, 2, 1, 1),                                # smallest plane
                (2, 3, 31, 63), (2, 3, 32, 64), (2, 3, 33, 65),  # one under, at and over the tile
                (1, 2, 70, 130),                             # 3 x 3 tiles, element-by-element staging
                (2, 2, 64, 128),                             # several tiles, the aligned 16-byte staging and store paths
                (1, 3, 15, 16),                              # stride 2 gives Wo = 8: dy aligned
                (1, 2, 40, 72)]                              # x aligned; dy not aligned at stride 2
TILED_DISPATCH = [(1, 2, 35, 5601), (1, 2, 34, 5608)]       # rows too wide for the whole-row kernels' LDS budget
ONES = {"whole": [(27, 4, 19, 19), (2, 4, 150, 150)], "tiled": [(1, 2, 70, 130), (2, 2, 64, 128)]}
ONEHOT = {"whole": [(2, 3, 8, 17), (27, 4, 19, 19), (2, 4, 150, 150), (1, 2, 151, 149)],
          "tiled": [(2, 3, 33, 65), (1, 2, 70, 130), (2, 2, 64, 128)], "dispatch": [(1, 2, 34, 5608)]}
AFFINE = [(27, 4, 19, 19), (2, 4, 150, 150), (1, 2, 151, 149), (2, 3, 8, 17)]
ACTS = (0, 1, 2)  # csrc/ssdk_dwplane.hip DwpParams.act: 0 none | 1 ReLU6 | 2 ReLU
ALIGN = [(2, 3, 8, 17), (27, 4, 19, 19), (1, 2, 151, 149)]
OFFSETS = {"x": 1, "dy": 3, "w": 4}  # elements into the allocation: base pointers 2-, 6- and 8-byte aligned


def sid(shape):
    return "x".join(str(v) for v in shape)


def depths():
    from ssds.modeling.layers import dwconv as D

    return D.DW_SUM_DEPTH, D.DW_STATS_DEPTH


def out_hw(h, w, stride):
    return (h - 1) // stride + 1, (w - 1) // stride + 1


# ---- operands and truth ------------------------------------------------------------------------------------------------------------
def operands(shape, stride, dtype_name, seed=None):
    n, c, h, w = shape
    dtype = DTYPES[dtype_name]
    g = torch.Generator().manual_seed(100000 * stride + 1000 * n + 100 * c + 7 * h + 3 * w + CODES[dtype_name] if seed is None else seed)
    x = torch.randn(n, c, h, w, generator=g).to(dtype)
    wt = (torch.randn(c, 1, 3, 3, generator=g) / 3).to(dtype).float()
    ho, wo = out_hw(h, w, stride)
    dy = torch.randn(n, c, ho, wo, generator=g).to(dtype)
    return x, wt, dy


def _conv64(x, wt, dy, stride):
    x64 = x.detach().double().requires_grad_(True)  # (detach: .double() of an fp64 tensor is the tensor itself)
    w64 = wt.detach().double().requires_grad_(True)
    y = F.conv2d(x64, w64, None, stride, 1, 1, x.shape[1])
    y.backward(dy.double())
    return y.detach(), x64.grad, w64.grad


def truth(x, wt, dy, stride):
    """fp64 y, dx, dW, their masses, and the per-channel statistics of the unrounded y with the sums their bars need."""
    y, dx, dw = _conv64(x, wt, dy, stride)
    my, mdx, mw = _conv64(x.abs(), wt.abs(), dy.abs(), stride)
    dims = (0, 2, 3)
    return {"y": y, "dx": dx, "dw": dw, "My": my, "Mdx": mdx, "Mw": mw,
            "sums": torch.stack([y.sum(dims), y.pow(2).sum(dims)], 1),
            "S_abs": y.abs().sum(dims), "S_sq": y.pow(2).sum(dims), "S_My": my.sum(dims), "S_yMy": (y.abs() * my).sum(dims)}


def affine_operands(shape, stride, dtype_name, act):
    """x = k / 8 (|k| <= 32), a in {0.5, 1, 2}, b a multiple of 1/8 in [-1, 3] (positive on some channels, negative on others):
    act(a x + b) is exact in bf16 and fp16.  -> x, coef [C,4] = (a, b, 0, 0), the staged tensor, w, dy."""
    n, c, h, w = shape
    dtype = DTYPES[dtype_name]
    g = torch.Generator().manual_seed(31 * n + 17 * c + 5 * h + 3 * w + stride + 1000 * act)
    x = (torch.randint(-32, 33, (n, c, h, w), generator=g).float() / 8).to(dtype)
    a = torch.tensor([0.5, 1.0, 2.0])[torch.arange(c) % 3]
    b = torch.randint(-8, 25, (c,), generator=g).float() / 8
    b[0], b[-1] = 1.5, -0.5
    coef = torch.zeros(c, 4)
    coef[:, 0], coef[:, 1] = a, b
    staged = apply_act(x.double() * a.double().view(1, -1, 1, 1) + b.double().view(1, -1, 1, 1), act)
    _, wt, dy = operands(shape, stride, dtype_name)
    return x, coef, staged, wt, dy


def apply_act(v, act):
    if act:
        v = v.clamp(min=0)
    if act == 1:
        v = v.clamp(max=6)
    return v


def affine_value_set():
    """every value a x + b can take in affine_operands, fp64"""
    k = torch.arange(-32, 33).double() / 8
    a = torch.tensor([0.5, 1.0, 2.0]).double()
    b = torch.arange(-8, 25).double() / 8
    return (k.view(-1, 1, 1) * a.view(1, -1, 1) + b.view(1, 1, -1)).reshape(-1)


# ---- the bars ----------------------------------------------------------------------------------------------------------------------
def _ratio(err, bar):
    return float((err / bar.clamp(min=1e-300)).max()) if err.numel() else 0.0


def _say(rec, what, err, bar):
    worst = _ratio(err, bar)
    rec["ratios"][what] = worst
    rec["lines"].append("%s %s: worst |err| / bar = %.3f" % (what, rec["what"], worst))
    bad = int((~(err <= bar)).sum())  # (a NaN is outside every bar)
    if bad:
        rec["failures"].append("%s: %d elements outside the bar, worst %.3g of it" % (what, bad, worst))


def judge(rec, got, tr, dtype_name):
    """got: {"y", "dx", "dw", "sums"} (any subset) on any device -> rec gets a ratio and a line per tensor, a failure per miss."""
    sum_depth, stats_depth = depths()
    for k in ("y", "dx"):
        if got.get(k) is None:
            continue
        want, mass = tr[k], tr["My" if k == "y" else "Mdx"]
        err = (got[k].double().cpu() - want).abs()
        if dtype_name == "f32":
            bar = 16 * U * mass
        else:
            bar = EPS[dtype_name] * want.abs() + 4 * EPS[dtype_name] * float(want.pow(2).mean().sqrt())
        _say(rec, k, err, bar)
    if got.get("dw") is not None:
        _say(rec, "dW", (got["dw"].double().cpu() - tr["dw"]).abs(), sum_depth * U * tr["Mw"])
    if got.get("sums") is not None:
        err = (got["sums"].double().cpu() - tr["sums"]).abs()
        _say(rec, "sum", err[:, 0], stats_depth * U * tr["S_abs"] + 16 * U * tr["S_My"])
        _say(rec, "sumsq", err[:, 1], stats_depth * U * tr["S_sq"] + 2 * 16 * U * tr["S_yMy"])
    return rec


def new_rec(what):
    return {"what": what, "ratios": {}, "lines": [], "failures": [], "names": None}


def _equal(rec, what, got, want):
    if tuple(got.shape) != tuple(want.shape) or not torch.equal(got.cpu(), want.cpu()):
        diff = int((got.cpu() != want.cpu()).sum()) if tuple(got.shape) == tuple(want.shape) else -1
        rec["failures"].append("%s: not equal (%d elements differ)" % (what, diff))


# ---- an fp32 CPU model of the three passes, rounded once ---------------------------------------------------------------------------
def model(x, wt, dy, stride, dtype_name):
    dtype = DTYPES[dtype_name]
    x32 = x.float().detach().requires_grad_(True)
    w32 = wt.float().detach().requires_grad_(True)
    y = F.conv2d(x32, w32, None, stride, 1, 1, x.shape[1])
    y.backward(dy.float())
    y = y.detach()
    return {"y": y.to(dtype), "dx": x32.grad.to(dtype), "dw": w32.grad.clone(),
            "sums": torch.stack([y.sum((0, 2, 3)), y.pow(2).sum((0, 2, 3))], 1)}


# ---- the library's plan ------------------------------------------------------------------------------------------------------------
def plan(kind, shape, stride, dtype_name):
    """ssdk_dwconv_plan: the whole-row cut of pass ``kind`` (0 forward, 1 input gradient, 2 weight gradient) or None (tiled kernels)."""
    from ssds import _native as N

    out = (ctypes.c_int32 * 12)()
    rc = N.lib.ssdk_dwconv_plan(kind, shape[0], shape[1], shape[2], shape[3], stride, CODES[dtype_name], out)
    assert rc in (0, 1), rc
    return dict(zip(PLAN_NAMES, out)) if rc == 0 else None


def expected_names(shape, stride, dtype_name, family):
    """the kernel the library's own plan sends each pass to (``tiled``: the switch overrides the plan)"""
    if family == "tiled":
        return list(TILED_NAMES)
    return [WHOLE_NAMES[k] if plan(k, shape, stride, dtype_name) else TILED_NAMES[k] for k in range(3)]


def positions(shape):
    """as _positions of tests/test_gpu_necktrain.py"""
    n, c, h, w = shape
    pos = [(0, 0, 0, 0), (n - 1, c - 1, h - 1, w - 1), (0, 0, h - 1, 0), (0, c - 1, 0, w - 1), (n - 1, 0, h - 1, w // 2),
           (n - 1, c // 2, h // 2, w - 1), (0, c // 2, h // 2, w // 2), (n - 1, c - 1, max(h - 2, 0), max(w - 2, 0))]
    return sorted(set(pos))


def seam_positions(shape, stride, dtype_name, family):
    """positions of dy: the eight of ``positions`` and both sides of every band and group seam of the case's three plans (whole-row
    kernels) or of every 32-row / 64-column tile seam of y and of dx (tiled kernels)."""
    n, c, h, w = shape
    ho, wo = out_hw(h, w, stride)
    rows, cols, imgs = set(), set(), set()
    tiled_passes = [k for k in range(3) if family != "whole" or plan(k, shape, stride, dtype_name) is None]
    for k in range(3):
        per = stride if k == 1 else 1  # the input gradient's thread space is dx: a seam at row r lies at dy row r / stride
        if k in tiled_passes:
            rows.update(v for r in range(32, h if k == 1 else ho, 32) for v in (r // per - 1, r // per))
            cols.update(v for q in range(64, w if k == 1 else wo, 64) for v in (q // per - 1, q // per))
        else:
            p = plan(k, shape, stride, dtype_name)
            rows.update(v for b in range(1, p["T"]) for v in (b * p["TR"] // per - 1, b * p["TR"] // per))
            if 1 < p["G"] < n:
                last = (n - 1) // p["G"] * p["G"]
                imgs.update((p["G"] - 1, p["G"], last - 1, last))
    rows = sorted(r for r in rows if 0 <= r < ho)
    cols = sorted(q for q in cols if 0 <= q < wo)
    if len(cols) > 8:  # (rows of thousands of pixels: the first two and the last two seams)
        cols = cols[:4] + cols[-4:]
    pos = set(positions((n, c, ho, wo)))
    pos.update((n - 1, c - 1, r, wo // 2) for r in rows)
    pos.update((0, 0, ho // 2, q) for q in cols)
    pos.update((i, c // 2, ho // 2, wo // 2) for i in imgs if 0 <= i < n)
    pos.update((n - 1, 0, r, q) for r in rows[:2] for q in cols[:2])
    return sorted(pos)


def one_hot_truth(x, wt, pos, stride, dtype_name):
    """dy one-hot at ``pos`` = ONE_HOT: dW[c,t] = the fp32 product dy x[window tap] (exact for 16-bit operands), dx = the fp32 product
    dy w[tap] rounded to the dtype at the positions the window reaches, zero elsewhere -- written out by the definition."""
    dtype = DTYPES[dtype_name]
    n, c, oy, ox = pos
    h, w = x.shape[2:]
    val = torch.tensor(ONE_HOT, dtype=torch.float32)
    xp = F.pad(x.float(), (1, 1, 1, 1))
    dw = torch.zeros(x.shape[1], 1, 3, 3)
    dx = torch.zeros(x.shape, dtype=dtype)
    for ky in range(3):
        for kx in range(3):
            dw[c, 0, ky, kx] = val * xp[n, c, oy * stride + ky, ox * stride + kx]
            iy, ix = oy * stride + ky - 1, ox * stride + kx - 1
            if 0 <= iy < h and 0 <= ix < w:
                dx[n, c, iy, ix] = (val * wt[c, 0, ky, kx].float()).to(dtype)
    return dx, dw


# ---- running the kernels -----------------------------------------------------------------------------------------------------------
def native(x, wt, dy, stride, want_sums=False, pending=None, need_dx=True):
    """through the autograd wrapper, tensors already on the device -> {"y", "dx", "dw", "sums"}"""
    from ssds.modeling.layers.dwconv import dwconv3x3

    xd = x.detach().requires_grad_(need_dx)
    wd = wt.detach().requires_grad_(True)
    y = dwconv3x3(xd, wd, stride, want_sums=want_sums, pending=pending)
    sums = getattr(y, "_ssdk_bn_sums", None)
    y.backward(dy)
    torch.cuda.synchronize()
    return {"y": y.detach(), "dx": xd.grad, "dw": wd.grad, "sums": sums}


def direct(x, w, dy, stride, y=None, dx=None, dw=None):
    """the three entry points on the calling thread (ssdk_last_kernel is per thread, autograd's backward runs on another one);
    x, w, dy of one dtype on the device -> {"y", "dx", "dw"}, [kernel name per pass]"""
    from ssds import _native as N

    n, c, h, wd = (int(v) for v in x.shape)
    ho, wo = out_hw(h, wd, stride)
    y = torch.empty((n, c, ho, wo), device=x.device, dtype=x.dtype) if y is None else y
    dx = torch.empty_like(x) if dx is None else dx
    dw = torch.empty((c, 1, 3, 3), device=x.device, dtype=torch.float32) if dw is None else dw
    need = int(N.lib.ssdk_dwconv_bwd_weight_workspace_bytes(n, c, h, wd, stride))
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device=x.device)
    code, sp = N.dtype_code(x), N.stream_ptr(x.device)
    names = []
    N.check(N.lib.ssdk_dwconv_fwd(x.data_ptr(), w.data_ptr(), y.data_ptr(), n, c, h, wd, stride, code, sp), "dwconv_fwd")
    names.append(N.last_kernel())
    N.check(N.lib.ssdk_dwconv_bwd_data(dy.data_ptr(), w.data_ptr(), dx.data_ptr(), n, c, h, wd, stride, code, sp), "dwconv_bwd_data")
    names.append(N.last_kernel())
    N.check(N.lib.ssdk_dwconv_bwd_weight(x.data_ptr(), dy.data_ptr(), dw.data_ptr(), ws.data_ptr(), need, n, c, h, wd, stride, code, sp),
            "dwconv_bwd_weight")
    names.append(N.last_kernel())
    torch.cuda.synchronize()
    return {"y": y, "dx": dx, "dw": dw}, names


def _names(rec, names, shape, stride, dtype_name, family):
    rec["names"] = names
    want = expected_names(shape, stride, dtype_name, family)
    if names != want:
        rec["failures"].append("kernels %s, expected %s" % (names, want))


def check_random(shape, stride, dtype_name, family):
    """random operands: kernel names through the entry points, numbers through the wrapper against fp64"""
    rec = new_rec("%s s%d %s %s" % (sid(shape), stride, dtype_name, family))
    x, wt, dy = operands(shape, stride, dtype_name)
    tr = truth(x, wt, dy, stride)
    xd, wd, dyd = x.cuda(), wt.cuda(), dy.cuda()
    raw, names = direct(xd, wd.to(xd.dtype), dyd, stride)
    _names(rec, names, shape, stride, dtype_name, family)
    got = native(xd, wd, dyd, stride)
    for k in ("y", "dx", "dw"):
        if got[k].dtype != (torch.float32 if k == "dw" else DTYPES[dtype_name]) or not got[k].is_contiguous():
            rec["failures"].append("%s: dtype %s / layout" % (k, got[k].dtype))
        _equal(rec, k + " (entry point against wrapper)", raw[k], got[k])
    return judge(rec, got, tr, dtype_name)


def check_ones(shape, stride, dtype_name, family):
    """x = w = dy = 1: y, dx, dW (and sums on the whole-row kernels) are counts -- exact in every dtype"""
    rec = new_rec("ones %s s%d %s %s" % (sid(shape), stride, dtype_name, family))
    dtype = DTYPES[dtype_name]
    n, c, h, w = shape
    ho, wo = out_hw(h, w, stride)
    x, wt, dy = torch.ones(shape, dtype=dtype), torch.ones(c, 1, 3, 3), torch.ones(n, c, ho, wo, dtype=dtype)
    tr = truth(x, wt, dy, stride)
    assert float(tr["sums"].max()) < 2 ** 24 and float(tr["dw"].max()) < 2 ** 24
    stats = family == "whole"  # (fp32 too: ssdk_dwconv_fwd_stats takes SSDK_F32, and counts below 2^24 are exact in its accumulators)
    got = native(x.cuda(), wt.cuda(), dy.cuda(), stride, want_sums=stats)
    for k in ("y", "dx", "dw") + (("sums",) if stats else ()):
        if got[k] is None:
            rec["failures"].append(k + ": missing")
        else:
            _equal(rec, k, got[k].double(), tr[k])
    return rec


def check_onehot(shape, stride, dtype_name, family):
    rec = new_rec("onehot %s s%d %s %s" % (sid(shape), stride, dtype_name, family))
    from ssds.modeling.layers.dwconv import dwconv3x3

    dtype = DTYPES[dtype_name]
    x, wt, dy = operands(shape, stride, dtype_name)
    xd, wd = x.cuda().requires_grad_(True), wt.cuda().requires_grad_(True)
    y = dwconv3x3(xd, wd, stride)
    gy = torch.zeros(dy.shape, dtype=dtype, device="cuda")
    pos_all = seam_positions(shape, stride, dtype_name, "whole" if family == "dispatch" else family)
    for pos in pos_all:
        gy.zero_()
        gy[pos] = ONE_HOT
        gx, gw = torch.autograd.grad(y, (xd, wd), gy, retain_graph=True)
        want_dx, want_dw = one_hot_truth(x, wt, pos, stride, dtype_name)
        _equal(rec, "dW at %s" % (pos,), gw, want_dw)
        _equal(rec, "dx at %s" % (pos,), gx, want_dx)
    rec["lines"].append("%s: %d positions" % (rec["what"], len(pos_all)))
    return rec


def check_stats(shape, stride, dtype_name):
    """whole-row kernels, 16 bit: sums within the statistics bar of the fp64 sums of the unrounded y, y bit-equal to the plain
    forward, two runs bit-equal"""
    from ssds.modeling.layers.dwconv import dwconv3x3

    rec = new_rec("stats %s s%d %s" % (sid(shape), stride, dtype_name))
    x, wt, dy = operands(shape, stride, dtype_name)
    tr = truth(x, wt, dy, stride)
    xd, wd = x.cuda(), wt.cuda()
    plain = dwconv3x3(xd, wd, stride)
    runs = [dwconv3x3(xd, wd, stride, want_sums=True) for _ in range(2)]
    torch.cuda.synchronize()
    for y in runs:
        if getattr(y, "_ssdk_bn_sums", None) is None:
            rec["failures"].append("no sums attached")
            return rec
        _equal(rec, "y with statistics against the plain forward", y, plain)
    _equal(rec, "sums of two runs", runs[0]._ssdk_bn_sums, runs[1]._ssdk_bn_sums)
    return judge(rec, {"sums": runs[0]._ssdk_bn_sums}, tr, dtype_name)


def check_no_stats(shape, stride, dtype_name):
    """tiled kernels: no statistics workspace, no sums attached"""
    from ssds import _native as N
    from ssds.modeling.layers.dwconv import dwconv3x3

    rec = new_rec("nostats %s s%d %s" % (sid(shape), stride, dtype_name))
    n, c, h, w = shape
    if int(N.lib.ssdk_dwconv_fwd_stats_workspace_bytes(n, c, h, w, stride, CODES[dtype_name])) != 0:
        rec["failures"].append("ssdk_dwconv_fwd_stats_workspace_bytes != 0")
    x, wt, _ = operands(shape, stride, dtype_name)
    y = dwconv3x3(x.cuda(), wt.cuda(), stride, want_sums=True)
    torch.cuda.synchronize()
    if hasattr(y, "_ssdk_bn_sums"):
        rec["failures"].append("_ssdk_bn_sums attached")
    _equal(rec, "y against the plain forward", y, dwconv3x3(x.cuda(), wt.cuda(), stride))
    return rec


def check_affine(shape, stride, dtype_name, act):
    """the deferred-BatchNorm variants directly: y, sums and (through backward) dW against the fp64 convolution of act(a x + b)"""
    from ssds import _native as N

    rec = new_rec("affine %s s%d %s act%d" % (sid(shape), stride, dtype_name, act))
    n, c, h, w = shape
    if not N.lib.ssdk_dwconv_affine_supported(n, c, h, w, stride, CODES[dtype_name]):
        rec["failures"].append("ssdk_dwconv_affine_supported == 0")
        return rec
    x, coef, staged, wt, dy = affine_operands(shape, stride, dtype_name, act)
    if not torch.equal(staged.to(DTYPES[dtype_name]).double(), staged):
        rec["failures"].append("the staged tensor is not exact in the dtype")
    tr = truth(staged, wt, dy, stride)
    xd, wd, dyd, cd = x.cuda(), wt.cuda(), dy.cuda(), coef.cuda()
    got = native(xd, wd, dyd, stride, want_sums=True, pending=(cd, act), need_dx=False)
    if got["sums"] is None:
        rec["failures"].append("no sums attached")
    bare = native(xd, wd, dyd, stride, want_sums=False, pending=(cd, act), need_dx=False)
    _equal(rec, "y without statistics", bare["y"], got["y"])
    _equal(rec, "dW without statistics", bare["dw"], got["dw"])
    # the same convolution on the staged tensor, written out: bit for bit the two-step path
    two = native(staged.to(DTYPES[dtype_name]).cuda(), wd, dyd, stride)
    _equal(rec, "y against the two-step path", got["y"], two["y"])
    _equal(rec, "dW against the two-step path", got["dw"], two["dw"])
    got["dx"] = None
    return judge(rec, got, tr, dtype_name)


def guarded(t, offset, dt=None):
    """``t`` as a contiguous view ``offset`` elements past a 16-byte boundary inside one larger NaN-filled device allocation
    -> view, allocation, index of the view's first element"""
    dt = dt or t.dtype
    per = t.numel()
    guard = (4096 + per + 7) // 8 * 8
    big = torch.full((guard + offset + per + guard,), float("nan"), dtype=dt, device="cuda")
    assert big.data_ptr() % 16 == 0
    big[guard + offset:guard + offset + per] = t.reshape(-1).to(dt).cuda()
    v = big[guard + offset:guard + offset + per].view(t.shape)
    assert v.is_contiguous() and v.data_ptr() == big.data_ptr() + (guard + offset) * big.element_size()
    return v, big, guard + offset


def check_alignment(shape, stride, dtype_name, family):
    """x, dy, w (wrapper) and y, dx, dW (entry points) as 2-, 6- and 8-byte aligned views inside NaN-filled allocations: finite,
    bit-equal to the results on clean aligned copies, every guard element untouched"""
    rec = new_rec("align %s s%d %s %s" % (sid(shape), stride, dtype_name, family))
    dtype = DTYPES[dtype_name]
    n, c, h, w = shape
    ho, wo = out_hw(h, w, stride)
    x, wt, dy = operands(shape, stride, dtype_name)
    w16 = wt.to(dtype)
    clean = native(x.cuda(), w16.cuda(), dy.cuda(), stride)
    xv, keep_x, _ = guarded(x, OFFSETS["x"])
    dv, keep_d, _ = guarded(dy, OFFSETS["dy"])
    wv, keep_w, _ = guarded(w16, OFFSETS["w"])
    for t, mod in ((xv, 2), (dv, 6), (wv, 8)):
        assert t.data_ptr() % 16 == mod, (t.data_ptr() % 16, mod)
    # the wrapper must hand these very pointers on: its .contiguous() and .to(same dtype) are no-ops on contiguous views (asserted
    # here); the entry-point calls further down pass the misaligned pointers by construction and are the guarantee
    for t in (xv, dv, wv):
        assert t.detach().to(dtype).contiguous().data_ptr() == t.data_ptr()
    view = native(xv, wv, dv, stride)
    for k in ("y", "dx", "dw"):
        if not bool(torch.isfinite(view[k].float()).all()):
            rec["failures"].append(k + ": not finite (read outside the tensor)")
        _equal(rec, k + " of the misaligned views", view[k], clean[k])
    yv, keep_y, sy = guarded(torch.zeros(n, c, ho, wo, dtype=dtype), OFFSETS["x"])
    dxv, keep_dx, sx = guarded(torch.zeros(shape, dtype=dtype), OFFSETS["dy"])
    dwv, keep_dw, sw = guarded(torch.zeros(c, 1, 3, 3), 1)  # fp32: 4-byte aligned
    clean_raw, _ = direct(x.cuda(), w16.cuda(), dy.cuda(), stride)
    raw, names = direct(xv, wv, dv, stride, y=yv, dx=dxv, dw=dwv)
    _names(rec, names, shape, stride, dtype_name, family)
    for k, big, start in (("y", keep_y, sy), ("dx", keep_dx, sx), ("dw", keep_dw, sw)):
        _equal(rec, k + " into a misaligned view", raw[k], clean_raw[k])
        if k != "dw":  # (the wrapper rounds dW to the 16-bit weight's dtype)
            _equal(rec, k + " of the entry point against the wrapper", clean_raw[k], clean[k])
        per = raw[k].numel()
        if not (bool(torch.isnan(big[:start]).all()) and bool(torch.isnan(big[start + per:]).all())):
            rec["failures"].append(k + ": written outside the tensor")
    for k, big, t, off in (("x", keep_x, x, OFFSETS["x"]), ("dy", keep_d, dy, OFFSETS["dy"]), ("w", keep_w, w16, OFFSETS["w"])):
        if int(torch.isnan(big).sum()) != big.numel() - t.numel():
            rec["failures"].append(k + ": an input allocation was written")
    return rec


# ---- the case lists of the tiled family's child process (ids are known to the parent without running it) ----------------------------
def tiled_cases():
    cases = []
    for dt in ("f32", "bf16", "f16"):
        for s in STRIDES:
            cases += [("random", sh, s, dt) for sh in TILED_SWITCH]
            cases += [("ones", sh, s, dt) for sh in ONES["tiled"]]
            cases += [("onehot", sh, s, dt) for sh in ONEHOT["tiled"]]
            if dt != "f32":
                cases += [("nostats", sh, s, dt) for sh in ONES["tiled"]]
                cases += [("align", sh, s, dt) for sh in ALIGN]
    return cases


def case_id(case):
    return "%s-%s-s%d-%s" % (case[0], sid(case[1]), case[2], case[3])


def _run_case(case):
    kind, shape, stride, dt = case
    if kind == "random":
        return check_random(shape, stride, dt, "tiled")
    if kind == "ones":
        return check_ones(shape, stride, dt, "tiled")
    if kind == "onehot":
        return check_onehot(shape, stride, dt, "tiled")
    if kind == "nostats":
        return check_no_stats(shape, stride, dt)
    return check_alignment(shape, stride, dt, "tiled")


def main(argv):
    if argv != ["--family", "tiled"]:
        print("usage: dwjudge.py --family tiled   (with SSDK_DW_PLANE=0 in the environment)")
        return 2
    if os.environ.get("SSDK_DW_PLANE") != "0":
        print("SSDK_DW_PLANE=0 is not set: this process would run the whole-row kernels")
        return 2
    out = {}
    for case in tiled_cases():
        rec = _run_case(case)
        for line in rec["lines"]:
            print(line)
        out[case_id(case)] = rec
    print("RESULT " + json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
