"""The judge of the 1x1 training kernels (csrc/ssdk_pwtrain.hip with ssdk_pwtrain_kernels.h) and of their direct users: the 1x1 layers
(pointwise.PointwiseConv2d), the 3x3 layers that run as im2col / col2im around them (pointwise.NativeConv3x3) and the backward of an
SSD level's loc | conf pair (headconv.head_pair).  Operands, the fp64 truth with its absolute-value masses, the bars, the case lists,
an fp32 CPU model of every pass with its mutations, and the checks tests/test_gpu_pwtrain.py runs.  tests/test_pwjudge_cpu.py turns
the judge on the model and on the mutations.  Plain torch, importable on the CPU.  Not a conftest.

Random family.  x, dy ~ N(0, 1) rounded to the dtype; w ~ N(0, 1) / sqrt(K) rounded to the dtype and kept as the fp32 master tensor
holding the rounded values, so the layers run the product path (ssdk_pw_prepare, fp32 dW without a cast); bias fp32.  Truth:
``F.conv2d`` under autograd in fp64 on the CPU on those operands; the same operation on |x|, |w|, |dy|, |bias| gives the masses.

Bars (u = 2^-24; eps = 2^-8 bf16, 2^-10 fp16).  No other tolerance exists here.
  y, dx          per element   |err| <= f (eps |want| + 4 eps rms(want)): one 16-bit store, f = 1; f = 3 for the dx of NativeConv3x3,
                               a sum of up to 9 terms of a 16-bit dcol (tests/test_gpu_train.py::test_native_conv3x3_matches_torch)
  dW (fp32)      per element   |err| <= D u Mw, D = 128 cps_ub + 20 passes: products of two 16-bit values are exact in fp32, so only
                               the additions round, at most once per added term in any order.  128 cps_ub = the pixels of the longest
                               split (cps_ub = chunks if splits == 1 else ceil(chunks / (splits - 1)), chunks = B ceil(HW / 128));
                               20 = the 16 + 4 sequential adds of one pw_wgrad_reduce_kernel pass; passes = 1 up to 64 splits, else 2.
                               ``splits`` is recovered from ssdk_pw_wgrad_workspace_bytes = (splits + ceil(splits / 64)) Cout Cin 4,
                               which is strictly increasing in splits: no mirror of the plan.
  sums[:,0]      per channel   |err| <= Ds u sum|y| + (K + 1) u sum My            (against the fp64 sums of the UNROUNDED y)
  sums[:,1]      per channel   |err| <= Ds u sum y^2 + 2 (K + 1) u sum |y| My
                               Ds = 128 ceil(groups / rows) + 20 passes, rows recovered from ssdk_pw_stats_workspace_bytes =
                               (rows + ceil(rows / 64)) M 2 4, groups = B ceil(HW / 128); K + 1: the accumulator's K products + bias
  dbias (pair)   per channel   |err| <= 16 u sum|dy| (a torch reduction)

Exact family.  The bars are loose by construction (a sum of N terms is allowed N roundings), so every case also runs on operands
whose every partial sum, in ANY order, is an exactly representable number: x, dy, w in {-1, 0, 1} at a density that keeps the mean
mass of a 16-bit value near EXACT_MASS ({-2 .. 2} and dense where both contractions have at most 16 terms), integer biases.  The
conditions -- every value stored in 16 bits (y, dcol, dx) has mass <= 256, every fp32 sum (dW, sum y, sum y^2) has mass < 2^24, the
truth is representable in the output type -- are computed from the operands and asserted (``exact_conditions``), they are not a
measurement.  Then y, dx, dW and both statistics equal the truth bit for bit (``torch.equal``, no tolerance) on every path.
Variants: ``ternary``; ``ones`` (x = dy = 1: dW is the pixel count, for 3x3 the per-tap count of in-plane outputs); ``onehot`` (one
element of dy = ONE_HOT: dW[co, :] is one scaled pixel column of x, dx one scaled column of w)."""
import collections
import functools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "ssds.pytorch_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import guardband as G  # noqa: E402

U = 2.0 ** -24
EPS = {"bf16": 2.0 ** -8, "f16": 2.0 ** -10}
DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16}
CODES = {"bf16": 1, "f16": 2}  # include/ssdk.h SSDK_BF16 | SSDK_F16
DTYPE_NAMES = ["bf16", "f16"]
LOC, CONF = 24, 480
ONE_HOT = -1.3125
EXACT_MASS = 16.0  # mean mass of a 16-bit value of the exact family (the conditions need <= 256 at the maximum)
ONES_MASS = 8.0    # ... of the all-ones variant, whose x and dy are dense
VARIANTS = ("ternary", "ones", "onehot")
SHORT, LONG, REDUCE = "pw_gemm_short_kernel", "pw_gemm_long_kernel", "pw_wgrad_reduce_kernel"

# 1x1: (n, cin, cout, h, w) -> splits of the weight gradient, kernel of the forward, kernel of the input gradient, statistics rows
# (None: not pinned).  The smallest shapes that reach each branch of pw_wgrad_plan / pw_gemm_plan at the default switches.
PW = collections.OrderedDict([
    ((1, 8, 8, 1, 1), (1, SHORT, SHORT, 4)),            # wave tile 1x1, one chunk, one pixel; statistics rows = 4, three idle waves
    ((2, 16, 40, 1, 7), (2, SHORT, SHORT, None)),       # 3x1, tail of 7 < 8 pixels; dx with K = 40 (2 k-steps, no multiple of 32)
    ((2, 8, 32, 2, 5), (2, SHORT, SHORT, None)),        # 2x1
    ((3, 32, 16, 5, 29), (6, SHORT, SHORT, None)),      # 1x2, tail 17
    ((2, 40, 24, 9, 15), (4, SHORT, SHORT, None)),      # 2x2, 2 tiles
    ((1, 24, 48, 3, 43), (2, SHORT, SHORT, None)),      # 3x2, HW = 129: a tail of 1 pixel
    ((67, 8, 16, 1, 1), (67, SHORT, SHORT, 68)),        # 67 splits: two reduce passes, last block 3 rows; statistics rows = 68: two passes
    ((3, 32, 48, 23, 126), (69, SHORT, SHORT, None)),   # 69 splits, 2898-pixel planes at 2-byte alignment
    ((2, 64, 64, 13, 10), (4, SHORT, SHORT, None)),     # tiled, one 128 x 128 tile half full, HW = 130
    ((1, 136, 72, 16, 17), (3, LONG, SHORT, None)),     # tiled, 2 tiles, ragged rows both sides; forward long K in one chunk; dx 3 k-steps
    ((5, 96, 200, 2, 2), (5, SHORT, LONG, None)),       # tiled, 4-pixel planes; forward short 3 k-steps, 13 fragments; dx long K = 200
    ((2, 288, 40, 3, 11), (2, LONG, SHORT, None)),      # streaming 3x2, 9 tiles; forward long K in two chunks (8 + 1 k-steps)
    ((2, 960, 320, 4, 4), (2, LONG, LONG, None)),       # tiled, 24 tiles; 30 k-steps in four chunks
    ((3, 40, 960, 1, 4355), (53, SHORT, LONG, None)),   # streaming, 53 splits, cps = 2, ragged last split; forward short K sliced in 2
    ((3, 256, 256, 1, 5381), (65, LONG, LONG, None)),   # tiled, 65 splits, cps = 2, ragged last split, two passes
])
# 3x3 through NativeConv3x3: (n, cin, cout, h, w, stride) -> folded
C3 = collections.OrderedDict([
    ((2, 8, 16, 7, 9, 1), False),       # 126 % 8 != 0
    ((2, 8, 16, 8, 8, 1), True),
    ((2, 3, 32, 12, 10, 2), False),     # Kp 27 -> 32, stride 2
    ((8, 16, 40, 9, 6, 2), True),       # stride 2, odd H
    ((1, 24, 24, 12, 11, 1), False),    # 132 pixels, one image
    ((3, 128, 24, 1, 1, 1), False),     # 1x1 maps: the centre tap only
    ((8, 128, 24, 1, 1, 1), True),
    ((2, 16, 16, 2, 2, 2), False),      # 2x2 -> 1x1
])
# the loc | conf pair: (n, cin, h, w) -> the weight gradients' im2col is folded
HEAD = collections.OrderedDict([((8, 96, 32, 32), False), ((3, 320, 16, 16), False), ((5, 512, 8, 8), True), ((6, 256, 4, 4), True),
                                ((7, 256, 2, 2), False), ((9, 128, 1, 1), False), ((2, 40, 19, 19), False)])
CASES = {"pw": PW, "c3": C3, "head": HEAD}
# guard bands through the C-ABI entry points: the tail and idle-wave shapes
GUARD_PW = [(1, 8, 8, 1, 1), (2, 16, 40, 1, 7), (1, 24, 48, 3, 43), (67, 8, 16, 1, 1), (2, 64, 64, 13, 10), (1, 136, 72, 16, 17)]
GUARD_C3 = [(2, 8, 16, 7, 9, 1), (2, 8, 16, 8, 8, 1), (2, 3, 32, 12, 10, 2), (8, 16, 40, 9, 6, 2), (3, 128, 24, 1, 1, 1)]

Geo = collections.namedtuple("Geo", "kind n cin cout h w k stride ho wo")


def geo(kind, case):
    if kind == "pw":
        n, cin, cout, h, w = case
        k, s = 1, 1
    elif kind == "c3":
        n, cin, cout, h, w, s = case
        k = 3
    else:
        n, cin, h, w = case
        cout, k, s = LOC + CONF, 3, 1
    return Geo(kind, n, cin, cout, h, w, k, s, (h - 1) // s + 1, (w - 1) // s + 1)


def sid(case):
    return "x".join(str(v) for v in case)


def fold_below():
    from ssds.modeling.layers import pointwise as P

    return P.FOLD_BELOW


def folded(g):
    """the layers' own rule (pointwise._Conv3x3Native.forward, headconv._weight_gradients); the case lists pin its answer"""
    p = g.ho * g.wo
    return g.k == 3 and g.n > 1 and p < fold_below() and (g.n * p) % 8 == 0


def gemm_dims(g):
    """-> (B, K, HW) of the ssdk_pw_* calls the layer makes"""
    if g.k == 1:
        return g.n, g.cin, g.h * g.w
    kp = (g.cin * 9 + 7) // 8 * 8
    return (1, kp, g.n * g.ho * g.wo) if folded(g) else (g.n, kp, g.ho * g.wo)


def wgrad_calls(g):
    """[(first output channel, one past the last)] of the layer's ssdk_pw_wgrad calls"""
    return [(0, LOC), (LOC, LOC + CONF)] if g.kind == "head" else [(0, g.cout)]


# ---- what the public workspace queries tell ------------------------------------------------------------------------------------------
def rows_from_total(total):
    """total = s + ceil(s / 64) -> s (strictly increasing in s, so the answer is unique)"""
    s = total - (total + 64) // 65
    assert s >= 1 and s + (s + 63) // 64 == total, (total, s)
    return s


def splits_of(b, cout, cin, hw):
    from ssds import _native as N

    nbytes = int(N.lib.ssdk_pw_wgrad_workspace_bytes(b, cout, cin, hw))
    assert nbytes > 0 and nbytes % (cout * cin * 4) == 0, nbytes
    return rows_from_total(nbytes // (cout * cin * 4))


def stats_rows_of(b, k, m, hw):
    from ssds import _native as N

    nbytes = int(N.lib.ssdk_pw_stats_workspace_bytes(b, k, m, hw))
    assert nbytes > 0 and nbytes % (m * 8) == 0, nbytes
    return rows_from_total(nbytes // (m * 8))


def chunks_of(b, hw):
    return b * ((hw + 127) // 128)


def depth_w(b, hw, splits):
    chunks = chunks_of(b, hw)
    cps_ub = chunks if splits == 1 else -(-chunks // (splits - 1))
    return 128 * cps_ub + 20 * (1 if splits <= 64 else 2)


def depth_s(b, hw, rows):
    return 128 * -(-chunks_of(b, hw) // rows) + 20 * (1 if rows <= 64 else 2)


def plan_of(g):
    """{"dims", "wgrad": [(c0, c1, splits)], "rows": statistics rows (1x1 only), "fold"} by the library's own answers"""
    b, k, hw = gemm_dims(g)
    return {"dims": (b, k, hw), "fold": folded(g), "wgrad": [(c0, c1, splits_of(b, c1 - c0, k, hw)) for c0, c1 in wgrad_calls(g)],
            "rows": stats_rows_of(b, k, g.cout, hw) if g.kind == "pw" else None}


def depth_vector(g, plan):
    """D per output channel"""
    b, _, hw = plan["dims"]
    d = torch.zeros(g.cout, dtype=torch.float64)
    for c0, c1, splits in plan["wgrad"]:
        d[c0:c1] = depth_w(b, hw, splits)
    return d


# ---- operands and truth --------------------------------------------------------------------------------------------------------------
def _gen(g, dtype_name, salt):
    return torch.Generator().manual_seed(1000003 * salt + 100000 * g.stride + 1000 * g.n + 100 * g.cin + 31 * g.cout + 7 * g.h + 3 * g.w
                                         + CODES[dtype_name])


def operands(kind, case, dtype_name):
    """-> x, w (fp32 master holding dtype values), bias (fp32), dy"""
    g = geo(kind, case)
    dtype, gen = DTYPES[dtype_name], _gen(g, dtype_name, 1)
    x = torch.randn(g.n, g.cin, g.h, g.w, generator=gen).to(dtype)
    w = (torch.randn(g.cout, g.cin, g.k, g.k, generator=gen) / (g.cin * g.k * g.k) ** 0.5).to(dtype).float()
    bias = torch.randn(g.cout, generator=gen) * 0.5
    dy = torch.randn(g.n, g.cout, g.ho, g.wo, generator=gen).to(dtype)
    return x, w, bias, dy


def _ints(gen, shape, density, amp):
    val = torch.randint(1, amp + 1, shape, generator=gen).float() * (torch.randint(0, 2, shape, generator=gen).float() * 2 - 1)
    return val if density >= 1.0 else val * (torch.rand(shape, generator=gen) < density).float()


def densities(g):
    """-> (density of x, of w, of dy, amplitude): mean mass of y, dcol and dx near EXACT_MASS, dense {-2 .. 2} where both
    contractions have at most 16 terms"""
    ly, ldx = g.cin * g.k * g.k, g.cout * g.k * g.k
    if max(ly, ldx) <= 16:
        return 1.0, 1.0, 1.0, 2
    return (min(1.0, (EXACT_MASS / ly) ** 0.5), min(1.0, (EXACT_MASS / max(ly, ldx)) ** 0.5), min(1.0, (EXACT_MASS / ldx) ** 0.5), 1)


def onehot_position(g):
    """the last pixel of the last image, last output channel: inside every tail"""
    return (g.n - 1, g.cout - 1, g.ho - 1, g.wo - 1)


def exact_operands(kind, case, dtype_name, variant):
    g = geo(kind, case)
    dtype, gen = DTYPES[dtype_name], _gen(g, dtype_name, 2)
    dx_, dw_, dd_, amp = densities(g)
    if variant == "ones" and amp == 1:  # (against dense ones a row of w IS the mass of y, a column that of dx)
        dw_ = min(1.0, ONES_MASS / (max(g.cin, g.cout) * g.k * g.k))
    x = _ints(gen, (g.n, g.cin, g.h, g.w), dx_, amp)
    w = _ints(gen, (g.cout, g.cin, g.k, g.k), dw_, amp)
    bias = torch.randint(-2, 3, (g.cout,), generator=gen).float()
    dy = _ints(gen, (g.n, g.cout, g.ho, g.wo), dd_, amp)
    if variant == "ones":
        x, dy = torch.ones_like(x), torch.ones_like(dy)
    elif variant == "onehot":
        dy = torch.zeros_like(dy)
        dy[onehot_position(g)] = ONE_HOT
    return x.to(dtype), w, bias, dy.to(dtype)


def _conv(g, x, w, b):
    return F.conv2d(x, w, b, g.stride, g.k // 2)


def _truth(g, x, w, bias, dy, masses):
    x64 = x.detach().double().requires_grad_(True)
    w64 = w.detach().double().requires_grad_(True)
    b64 = bias.detach().double().requires_grad_(True)
    y = _conv(g, x64, w64, b64)
    y.backward(dy.double())
    y = y.detach()
    tr = {"y": y, "dx": x64.grad, "dw": w64.grad, "db": b64.grad, "S_dy": dy.double().abs().sum((0, 2, 3))}
    ax, aw, ab, ad = x.double().abs(), w.double().abs(), bias.double().abs(), dy.double().abs()
    pad = (g.k // 2, g.k // 2)
    tr["Mw"] = torch.nn.grad.conv2d_weight(ax, tuple(w.shape), ad, (g.stride, g.stride), pad)
    if "y" in masses:
        my = _conv(g, ax, aw, ab)
        dims = (0, 2, 3)
        tr.update(My=my, sums=torch.stack([y.sum(dims), y.pow(2).sum(dims)], 1), S_abs=y.abs().sum(dims), S_sq=y.pow(2).sum(dims),
                  S_My=my.sum(dims), S_yMy=(y.abs() * my).sum(dims), S_My2=my.pow(2).sum(dims))
    if "dx" in masses:
        tr["Mdx"] = torch.nn.grad.conv2d_input(tuple(x.shape), aw, ad, (g.stride, g.stride), pad)
        # dcol = W2^T dy, entries that land outside the plane included (they are stored in 16 bits too).  fp32 holds these masses
        # exactly: sums of small integers, or of ONE_HOT multiples with a single non-zero term
        tr["Mdcol"] = float(torch.matmul(aw.float().reshape(g.cout, -1).t(), ad.float().reshape(g.n, g.cout, -1)).max())
    return tr


@functools.lru_cache(maxsize=4)
def truth(kind, case, dtype_name, family="random"):
    """fp64 y, dx, dW, dbias with the masses the bars need (random: Mw, and My with the statistics' sums for the 1x1 cases; the exact
    variants: all of them).  Cached: compute once, share, leave unchanged."""
    g = geo(kind, case)
    if family == "random":
        ops = operands(kind, case, dtype_name)
        masses = ("y",) if kind == "pw" else ()
    else:
        ops = exact_operands(kind, case, dtype_name, family)
        masses = ("y", "dx")
    tr = _truth(g, *ops, masses=masses)
    tr["ops"] = ops
    return tr


def exact_conditions(g, tr, dtype_name):
    """the operand conditions of the exact family -> list of the violated ones (empty: every partial sum on every path is exact)"""
    dtype, bad = DTYPES[dtype_name], []
    for name, lim in (("My", 256), ("Mdx", 256), ("Mdcol", 256), ("Mw", 2 ** 24 - 1), ("S_My", 2 ** 24 - 1), ("S_My2", 2 ** 24 - 1)):
        v = tr[name]
        top = float(v.max()) if torch.is_tensor(v) else float(v)
        if top > lim:
            bad.append("%s: mass %.6g > %d" % (name, top, lim))
    for k in ("y", "dx"):
        if not torch.equal(tr[k].to(dtype).double(), tr[k]):
            bad.append("%s: the truth is not representable in %s" % (k, dtype_name))
    for k in ("dw", "sums", "db"):
        if not torch.equal(tr[k].float().double(), tr[k]):
            bad.append("%s: the truth is not representable in fp32" % k)
    return bad


# ---- the bars ------------------------------------------------------------------------------------------------------------------------
def new_rec(what):
    return {"what": what, "ratios": {}, "lines": [], "failures": [], "names": None, "plan": None}


def _say(rec, what, err, bar):
    worst = float((err / bar.clamp(min=1e-300)).max()) if err.numel() else 0.0
    rec["ratios"][what] = worst
    rec["lines"].append("%s %s: worst |err| / bar = %.3f" % (what, rec["what"], worst))
    bad = int((~(err <= bar)).sum())  # (a NaN is outside every bar)
    if bad:
        rec["failures"].append("%s: %d elements outside the bar, worst %.3g of it" % (what, bad, worst))


def _equal(rec, what, got, want):
    got, want = got.detach().cpu(), want.detach().cpu()
    if tuple(got.shape) != tuple(want.shape) or not torch.equal(got, want):
        diff = int((got != want).sum()) if tuple(got.shape) == tuple(want.shape) else -1
        rec["failures"].append("%s: not equal (%d elements differ)" % (what, diff))


def dx_factor(g):
    """16-bit roundings on the way to dx: NativeConv3x3 sums up to 9 terms of a 16-bit dcol (factor 3, as the existing test derives);
    the 1x1 layers and the head pair (one convolution on the inference kernels) store once"""
    return 3.0 if g.kind == "c3" else 1.0


def judge(rec, g, got, tr, dtype_name, plan):
    """got: {"y", "dx", "dw", "sums", "db"} (any subset, any device) against the random family's bars"""
    eps = EPS[dtype_name]
    for k, f in (("y", 1.0), ("dx", dx_factor(g))):
        if got.get(k) is not None:
            want = tr[k]
            err = (got[k].detach().double().cpu() - want).abs()
            _say(rec, k, err, f * (eps * want.abs() + 4 * eps * float(want.pow(2).mean().sqrt())))
    if got.get("dw") is not None:
        d = depth_vector(g, plan).view(-1, 1, 1, 1)
        _say(rec, "dW", (got["dw"].detach().double().cpu() - tr["dw"]).abs(), d * U * tr["Mw"])
    if got.get("sums") is not None:
        b, k, hw = plan["dims"]
        ds = depth_s(b, hw, plan["rows"])
        err = (got["sums"].detach().double().cpu() - tr["sums"]).abs()
        _say(rec, "sum", err[:, 0], ds * U * tr["S_abs"] + (k + 1) * U * tr["S_My"])
        _say(rec, "sumsq", err[:, 1], ds * U * tr["S_sq"] + 2 * (k + 1) * U * tr["S_yMy"])
    if got.get("db") is not None:
        _say(rec, "dbias", (got["db"].detach().double().cpu() - tr["db"]).abs(), 16 * U * tr["S_dy"])
    return rec


def judge_exact(rec, got, tr, dtype_name):
    """the exact family: bit equality with the fp64 truth cast to the output type"""
    dtype = DTYPES[dtype_name]
    for k in ("y", "dx", "dw", "sums", "db"):
        if got.get(k) is None:
            continue
        want = tr[k].to(dtype if k in ("y", "dx") else torch.float32)
        if got[k].dtype != want.dtype:
            rec["failures"].append("%s: dtype %s" % (k, got[k].dtype))
        _equal(rec, {"dw": "dW", "db": "dbias"}.get(k, k), got[k], want)
    return rec


# ---- an fp32 CPU model of the passes: chunked fp32 partials added in index order, stores rounded to the dtype -------------------------
def im2col(g, x, mut=()):
    """x [B, C, H, W] fp32 -> col [B, C * 9, Ho * Wo] (k = ci * 9 + ky * 3 + kx, torch's own flattening).  Mutations: ``border``
    (taps outside the plane read the nearest pixel instead of zero), ``parity`` (the stride-2 window starts one pixel late),
    ``swap_tap`` (taps (0, 1) and (1, 0) of channel 0 change places)."""
    s, off = g.stride, (1 if "parity" in mut else 0)
    xp = F.pad(x, (1, 1 + off, 1, 1 + off), mode="replicate" if "border" in mut else "constant")
    taps = [xp[:, :, ky + off:ky + off + s * (g.ho - 1) + 1:s, kx + off:kx + off + s * (g.wo - 1) + 1:s] for ky in range(3) for kx in range(3)]
    col = torch.stack(taps, 2).reshape(g.n, g.cin * 9, g.ho * g.wo).clone()
    if "swap_tap" in mut:
        col[:, [1, 3]] = col[:, [3, 1]]
    return col


def col2im(g, dcol):
    """dcol [B, C * 9, Ho * Wo] -> dx [B, C, H, W] in dcol's type: every input pixel gathers its <= 9 contributions"""
    dx = torch.zeros(g.n, g.cin, g.h + 2, g.w + 2, dtype=dcol.dtype)
    d = dcol.reshape(g.n, g.cin, 9, g.ho, g.wo)
    s = g.stride
    for t in range(9):
        ky, kx = divmod(t, 3)
        dx[:, :, ky:ky + s * (g.ho - 1) + 1:s, kx:kx + s * (g.wo - 1) + 1:s] += d[:, :, t]
    return dx[:, :, 1:g.h + 1, 1:g.w + 1]


def fold(t):
    """[B, C, P] -> [1, C, B * P], pixel index b * P + p (pointwise._fold)"""
    b, c, p = t.shape
    return t.permute(1, 0, 2).reshape(1, c, b * p)


def unfold(t, b):
    c, bp = t.shape[1:]
    return t.view(c, b, bp // b).permute(1, 0, 2)


def reduce_model(t):
    """pw_wgrad_reduce_kernel, applied until one row is left: blocks of 64 rows, four quarters of 16 sequential adds, the quarters
    added in order"""
    while True:
        rows, out = t.shape[0], []
        for blk in range((rows + 63) // 64):
            q = []
            for kq in range(4):
                r = t[blk * 64 + kq * 16:min(rows, blk * 64 + kq * 16 + 16)]
                s = torch.zeros_like(t[0])
                for row in r:
                    s = s + row
                q.append(s)
            out.append(((q[0] + q[1]) + q[2]) + q[3])
        if len(out) == 1:
            return out[0]
        t = torch.stack(out)


def wgrad_model(dyf, col, splits, mut=()):
    """dyf [B, M, P], col [B, K, P] fp32 -> dW [M, K]: 128-pixel chunk partials added in index order inside a split, the splits'
    rows through reduce_model.  Mutations: ``drop_pixel`` / ``drop_chunk`` (the last of the last image), ``omit_split`` /
    ``double_split`` (the last split's row), ``bf16_partial`` (the first split's row rounded to bf16 before the reduce)."""
    b, m, p = dyf.shape
    cpi = (p + 127) // 128
    chunks = b * cpi
    cps = chunks if splits == 1 else -(-chunks // splits)
    assert -(-chunks // cps) == splits, (chunks, cps, splits)
    parts = []
    for s in range(splits):
        acc = torch.zeros(m, col.shape[1])
        for c in range(s * cps, min(chunks, (s + 1) * cps)):
            img, j = divmod(c, cpi)
            lo, hi = j * 128, min(p, j * 128 + 128)
            if c == chunks - 1 and "drop_chunk" in mut:
                continue
            if c == chunks - 1 and "drop_pixel" in mut:
                hi -= 1
            acc = acc + dyf[img, :, lo:hi] @ col[img, :, lo:hi].t()
        parts.append(acc)
    if "omit_split" in mut:
        parts[-1] = torch.zeros_like(parts[-1])
    if "double_split" in mut:
        parts[-1] = parts[-1] * 2
    if "bf16_partial" in mut:
        parts[0] = parts[0].to(torch.bfloat16).float()
    return reduce_model(torch.stack(parts))


def stats_model(y32, y16, rows, mut=()):
    """y32 [B, M, P] (the fp32 accumulators) -> sums [M, 2]: wave ``r`` of ``rows`` adds the 128-pixel groups r, r + rows, ... in
    order, idle waves write zeros, the rows go through reduce_model.  Mutations: ``sumsq_rounded`` (the squares of the stored y),
    ``idle_garbage`` (an idle wave's row holds what the workspace held; with no idle wave, one more row is read)."""
    b, m, p = y32.shape
    gpi = (p + 127) // 128
    table = torch.zeros(rows, m, 2)
    for grp in range(b * gpi):
        img, j = divmod(grp, gpi)
        seg = y32[img, :, j * 128:min(p, j * 128 + 128)]
        sq = y16[img, :, j * 128:min(p, j * 128 + 128)].float() if "sumsq_rounded" in mut else seg
        table[grp % rows, :, 0] += seg.sum(1)
        table[grp % rows, :, 1] += (sq * sq).sum(1)
    if "idle_garbage" in mut:
        junk = torch.full((1, m, 2), 3.0)
        if b * gpi < rows:
            table[rows - 1] = junk[0]
        else:
            table = torch.cat([table, junk])
    return reduce_model(table)


def model(g, ops, dtype_name, plan, mut=()):
    """-> {"y", "dx", "dw", "sums" (1x1), "db"} as the layers compute them, in fp32 on the CPU"""
    x, w, bias, dy = ops
    dtype = DTYPES[dtype_name]
    b, kp, hw = plan["dims"]
    if g.k == 1:
        col, w2 = x.float().view(g.n, g.cin, hw), w.view(g.cout, g.cin)
    else:
        col = F.pad(im2col(g, x.float(), mut), (0, 0, 0, kp - g.cin * 9))
        w2 = F.pad(w.reshape(g.cout, g.cin * 9), (0, kp - g.cin * 9))
    dyf = dy.float().view(g.n, g.cout, g.ho * g.wo)
    if plan["fold"]:
        col, dyf = fold(col), fold(dyf)
    y32 = torch.matmul(w2, col) + bias.view(1, -1, 1)
    y16 = y32.to(dtype)
    dcol = torch.matmul(w2.t(), dyf).to(dtype)
    dyw = dyf
    if "mix_fold" in mut:  # the gradient in pixel order p * B + b against a col in b * P + p
        dyw = dy.float().view(g.n, g.cout, -1).permute(1, 2, 0).reshape(1, g.cout, -1)
    dw = torch.cat([wgrad_model(dyw[:, c0:c1], col, splits, mut) for c0, c1, splits in plan["wgrad"]])
    if "transpose" in mut:
        dw = dw.t().contiguous()
    out = {"db": dy.float().sum((0, 2, 3))}
    if g.k == 1:
        out.update(y=y16.view(g.n, g.cout, g.h, g.w), dx=dcol.view(x.shape), dw=dw.view(w.shape),
                   sums=stats_model(y32, y16, plan["rows"], mut))
    else:
        yb, db_ = (unfold(y16, g.n), unfold(dcol, g.n)) if plan["fold"] else (y16, dcol)
        out.update(y=yb.reshape(g.n, g.cout, g.ho, g.wo), dx=col2im(g, db_.float()[:, :g.cin * 9]).to(dtype),
                   dw=dw[:, :g.cin * 9].reshape(w.shape))
    return out


# ---- running the layers --------------------------------------------------------------------------------------------------------------
def _module(cls, g, w, bias, c0=0, c1=None, **kw):
    c1 = g.cout if c1 is None else c1
    m = cls(g.cin, c1 - c0, g.k, g.stride, g.k // 2, bias=True, **kw).cuda()
    with torch.no_grad():
        m.weight.copy_(w[c0:c1])
        m.bias.copy_(bias[c0:c1])
    return m


def native(g, ops, dtype_name, want_sums=False):
    """the layer under autocast with its fp32 master parameters (the product path) -> {"y", "dx", "dw", "db", "sums"}"""
    from ssds.modeling.layers import headconv as HC
    from ssds.modeling.layers import pointwise as P

    dtype = DTYPES[dtype_name]
    x, w, bias, dy = ops
    xd, dyd = x.cuda().requires_grad_(True), dy.cuda()
    out = {"sums": None}
    with torch.autocast("cuda", dtype=dtype):
        if g.kind == "head":
            mods = [_module(torch.nn.Conv2d, g, w, bias, 0, LOC), _module(torch.nn.Conv2d, g, w, bias, LOC, LOC + CONF)]
            assert HC.supported(xd, *mods)
            ys = HC.head_pair(xd, *mods)
            torch.autograd.backward(list(ys), [dyd[:, :LOC].contiguous(), dyd[:, LOC:].contiguous()])
            out["y"] = torch.cat([t.detach() for t in ys], 1)
        else:
            mods = [_module(P.PointwiseConv2d if g.kind == "pw" else P.NativeConv3x3, g, w, bias)]
            y = mods[0](xd)
            y.backward(dyd)
            out["y"] = y.detach()
    out.update(dx=xd.grad, dw=torch.cat([m.weight.grad for m in mods]), db=torch.cat([m.bias.grad for m in mods]))
    if want_sums:
        ys = P.pointwise_conv(xd.detach(), mods[0].weight.detach(), mods[0].bias.detach(), want_sums=True)
        out["sums"], out["y_stats"] = ys._ssdk_bn_sums, ys.detach()
    torch.cuda.synchronize()
    return out


def direct_pw(g, ops, dtype_name):
    """the three entry points on the calling thread (ssdk_last_kernel is per thread, autograd's backward runs on another one)
    -> {"y", "dx", "dw"}, [kernel name per pass]"""
    from ssds import _native as N

    dtype, code = DTYPES[dtype_name], CODES[dtype_name]
    x, w, bias, dy = ops
    hw = g.h * g.w
    xd, dyd, bd = x.cuda(), dy.cuda(), bias.cuda()
    w16 = w.view(g.cout, g.cin).to(dtype).cuda()
    wt16 = w16.t().contiguous()
    y, dx = torch.empty_like(dyd), torch.empty_like(xd)
    dw = torch.empty((g.cout, g.cin, 1, 1), device="cuda", dtype=torch.float32)
    need = int(N.lib.ssdk_pw_wgrad_workspace_bytes(g.n, g.cout, g.cin, hw))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    sp, names = N.stream_ptr(xd.device), []
    N.check(N.lib.ssdk_pw_forward(xd.data_ptr(), w16.data_ptr(), bd.data_ptr(), y.data_ptr(), g.n, g.cin, g.cout, hw, code, sp), "pw_forward")
    names.append(N.last_kernel())
    N.check(N.lib.ssdk_pw_forward(dyd.data_ptr(), wt16.data_ptr(), None, dx.data_ptr(), g.n, g.cout, g.cin, hw, code, sp), "pw_forward (dx)")
    names.append(N.last_kernel())
    N.check(N.lib.ssdk_pw_wgrad(dyd.data_ptr(), xd.data_ptr(), dw.data_ptr(), ws.data_ptr(), need, g.n, g.cout, g.cin, hw, code, sp), "pw_wgrad")
    names.append(N.last_kernel())
    torch.cuda.synchronize()
    return {"y": y, "dx": dx, "dw": dw}, names


def check_case(kind, case, dtype_name, family="random"):
    """one case of one family through its layer: the plan against the case list, the kernel names where ssdk_last_kernel can tell
    (1x1: through the entry points, bit-equal to the layer), and the family's checks"""
    g = geo(kind, case)
    rec = new_rec("%s %s %s %s" % (kind, sid(case), dtype_name, family))
    plan = rec["plan"] = plan_of(g)
    pinned = CASES[kind][case]
    if kind == "pw":
        splits, fwd, dxk, rows = pinned
        if plan["wgrad"][0][2] != splits or (rows is not None and plan["rows"] != rows):
            rec["failures"].append("plan: splits %d rows %d, listed %s %s" % (plan["wgrad"][0][2], plan["rows"], splits, rows))
    elif plan["fold"] != pinned:
        rec["failures"].append("plan: folded %s, listed %s" % (plan["fold"], pinned))
    tr = truth(kind, case, dtype_name, family)
    if family != "random":
        bad = exact_conditions(g, tr, dtype_name)
        assert not bad, bad  # (a condition on the operands: the judge's own fault, not the kernels')
    got = native(g, tr["ops"], dtype_name, want_sums=kind == "pw")
    if kind == "pw":
        raw, names = direct_pw(g, tr["ops"], dtype_name)
        rec["names"] = names
        if names != [fwd, dxk, REDUCE]:
            rec["failures"].append("kernels %s, listed %s" % (names, [fwd, dxk, REDUCE]))
        for k in ("y", "dx", "dw"):
            _equal(rec, k + " (entry point against the layer)", raw[k], got[k])
        _equal(rec, "y with statistics against the plain forward", got["y_stats"], got["y"])
    for k in ("y", "dx", "dw", "db"):
        if got[k].dtype != (DTYPES[dtype_name] if k in ("y", "dx") else torch.float32) or tuple(got[k].shape) != tuple(tr[k].shape):
            rec["failures"].append("%s: dtype %s shape %s" % (k, got[k].dtype, tuple(got[k].shape)))
    if kind != "head":
        got["db"] = None  # (asked for the pair only: the 16 u bar is the pair's)
    if family == "random":
        return judge(rec, g, got, tr, dtype_name, plan)
    return judge_exact(rec, got, tr, dtype_name)


# ---- guard bands through the C-ABI entry points ---------------------------------------------------------------------------------------
def _place(gs, name, t, off=0, is_input=True, poison=False):
    """``t`` as a view ``off`` elements past a 256-byte boundary in the middle of one 0xFF-filled allocation (``poison``: its
    interior holds 0xFF too -- an output, or a scratch nobody may rely on)"""
    es = t.element_size()
    gb, body = G.guard_bytes(t.shape, t.dtype), t.numel() * es
    lead = gb + off * es
    dev = gs.device
    storage = torch.cat([G._pattern(0xFF, lead, dev), G._pattern(0xFF if poison else 0, body, dev), G._pattern(0xFF, gb, dev)])
    view = storage[lead:lead + body].view(t.dtype).view(t.shape)
    assert view.data_ptr() == storage.data_ptr() + lead and view.is_contiguous()
    if not poison:
        view.copy_(t)
    return gs.adopt(name, storage, view, 0xFF, is_input)


def _finish(rec, gs, outs):
    for p in gs.problems():
        rec["failures"].append(p)
    for k, v in outs.items():
        if G.has_nan(v):
            rec["failures"].append("%s: NaN (an element nobody wrote, or a read outside a tensor)" % k)


def guard_pw(case, dtype_name, off, ws_fill):
    """ssdk_pw_forward (y and dx), ssdk_pw_forward_stats and ssdk_pw_wgrad with every tensor a guarded view: x, dy, y, dx ``off``
    elements into their allocations, the weight matrices and workspaces aligned, the workspaces pre-filled with ``ws_fill``"""
    from ssds import _native as N

    g = geo("pw", case)
    rec = new_rec("guard pw %s %s off%d ws%02x" % (sid(case), dtype_name, off, ws_fill))
    dtype, code = DTYPES[dtype_name], CODES[dtype_name]
    x, w, bias, dy = operands("pw", case, dtype_name)
    hw = g.h * g.w
    gs = G.GuardSet("cuda")
    w16 = w.view(g.cout, g.cin).to(dtype)
    xv, dv = _place(gs, "x", x, off), _place(gs, "dy", dy, off)
    wv, wtv, bv = _place(gs, "w16", w16), _place(gs, "wt16", w16.t().contiguous()), _place(gs, "bias", bias)
    outs = {"y": _place(gs, "y", dy, off, False, True), "y_stats": _place(gs, "y_stats", dy, off, False, True),
            "dx": _place(gs, "dx", x, off, False, True), "sums": _place(gs, "sums", torch.empty(g.cout, 2), 0, False, True),
            "dw": _place(gs, "dw", torch.empty(g.cout, g.cin), 0, False, True)}
    need_s = int(N.lib.ssdk_pw_stats_workspace_bytes(g.n, g.cin, g.cout, hw))
    need_w = int(N.lib.ssdk_pw_wgrad_workspace_bytes(g.n, g.cout, g.cin, hw))
    ws_s = _place(gs, "stats workspace", torch.full((need_s,), ws_fill, dtype=torch.uint8), 0, False)
    ws_w = _place(gs, "wgrad workspace", torch.full((need_w,), ws_fill, dtype=torch.uint8), 0, False)
    assert wv.data_ptr() % 16 == 0 and wtv.data_ptr() % 16 == 0 and ws_s.data_ptr() % 16 == 0 and ws_w.data_ptr() % 16 == 0
    assert xv.data_ptr() % 16 == (2 * off) % 16
    gs.arm()
    sp = N.stream_ptr(xv.device)
    N.check(N.lib.ssdk_pw_forward(xv.data_ptr(), wv.data_ptr(), bv.data_ptr(), outs["y"].data_ptr(), g.n, g.cin, g.cout, hw, code, sp), "pw_forward")
    N.check(N.lib.ssdk_pw_forward(dv.data_ptr(), wtv.data_ptr(), None, outs["dx"].data_ptr(), g.n, g.cout, g.cin, hw, code, sp), "pw_forward (dx)")
    N.check(N.lib.ssdk_pw_forward_stats(xv.data_ptr(), wv.data_ptr(), bv.data_ptr(), outs["y_stats"].data_ptr(), outs["sums"].data_ptr(),
                                        ws_s.data_ptr(), need_s, g.n, g.cin, g.cout, hw, code, sp), "pw_forward_stats")
    N.check(N.lib.ssdk_pw_wgrad(dv.data_ptr(), xv.data_ptr(), outs["dw"].data_ptr(), ws_w.data_ptr(), need_w, g.n, g.cout, g.cin, hw, code, sp),
            "pw_wgrad")
    torch.cuda.synchronize()
    _finish(rec, gs, outs)
    return rec, {k: v.clone() for k, v in outs.items()}


def guard_c3(case, dtype_name, off, fold_):
    """ssdk_im2col3x3 / ssdk_col2im3x3 (``fold_``: the two _folded) with x, col, dcol and dx guarded views ``off`` elements into
    their allocations; col must be the copy the definition gives, bit for bit"""
    from ssds import _native as N

    g = geo("c3", case)
    rec = new_rec("guard c3 %s %s off%d %s" % (sid(case), dtype_name, off, "folded" if fold_ else "plain"))
    dtype, code = DTYPES[dtype_name], CODES[dtype_name]
    x = operands("c3", case, dtype_name)[0]
    kp, p = (g.cin * 9 + 7) // 8 * 8, g.ho * g.wo
    want = F.pad(im2col(g, x.float()), (0, 0, 0, kp - g.cin * 9))
    want = (fold(want) if fold_ else want).to(dtype).contiguous()
    dcol = torch.randn(want.shape, generator=_gen(g, dtype_name, 3)).to(dtype)
    gs = G.GuardSet("cuda")
    xv, dcv = _place(gs, "x", x, off), _place(gs, "dcol", dcol, off)
    outs = {"col": _place(gs, "col", want, off, False, True), "dx": _place(gs, "dx", x, off, False, True)}
    gs.arm()
    sp = N.stream_ptr(xv.device)
    fi, fo = (N.lib.ssdk_im2col3x3_folded, N.lib.ssdk_col2im3x3_folded) if fold_ else (N.lib.ssdk_im2col3x3, N.lib.ssdk_col2im3x3)
    N.check(fi(xv.data_ptr(), outs["col"].data_ptr(), g.n, g.cin, g.h, g.w, g.stride, code, sp), "im2col3x3")
    N.check(fo(dcv.data_ptr(), outs["dx"].data_ptr(), g.n, g.cin, g.h, g.w, g.stride, code, sp), "col2im3x3")
    torch.cuda.synchronize()
    _finish(rec, gs, outs)
    _equal(rec, "col against the definition", outs["col"], want)
    # dx: <= 9 16-bit terms added in fp32 (<= 8 additions, a rounding each: 16 u of the mass with room to spare) and rounded once
    # to 16 bits (eps |want|), against the fp64 gather of the same terms
    d64 = (unfold(dcol.double(), g.n) if fold_ else dcol.double())[:, :g.cin * 9]
    want_dx, mass = col2im(g, d64), col2im(g, d64.abs())
    _say(rec, "dx(col2im)", (outs["dx"].double().cpu() - want_dx).abs(), EPS[dtype_name] * want_dx.abs() + 16 * U * mass)
    return rec, {k: v.clone() for k, v in outs.items()}


def same_results(rec, base, other, what):
    for k in base:
        if not G.same_bits(base[k], other[k]):
            rec["failures"].append("%s: %s differs from the aligned run on a zeroed workspace" % (what, k))


# ---- the table of ratios one GPU run leaves behind ------------------------------------------------------------------------------------
def log_ratios(rec):
    """PWJUDGE_RATIOS=<file>: one JSON line per judged case (profiles/r26_pwjudge_ratios.jsonl is such a run)"""
    path = os.environ.get("PWJUDGE_RATIOS")
    if path and rec["ratios"]:
        with open(path, "a") as f:
            f.write(json.dumps({"case": rec["what"], "plan": rec["plan"], "ratios": {k: round(v, 4) for k, v in rec["ratios"].items()}}) + "\n")
