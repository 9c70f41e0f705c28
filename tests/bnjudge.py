"""The judge of the BatchNorm training kernels (csrc/ssdk_bntrain.hip: the per-plane pair bn_reduce_kernel / bn_apply_kernel, the
flat pair bn_reduce_flat_kernel / bn_apply_flat_kernel, bn_fwd_finalize_kernel for handed-over sums, and the split path of the
synchronised BatchNorm): operands, the fp64 truth per channel and per element with its absolute-value masses, the bars, the case
list and the checks that tests/test_gpu_bntrain.py runs in process under the default dispatch and -- SSDK_BN_FLAT is read once per
process -- in ONE child process per forced family (``python tests/bnjudge.py --family per_plane|flat`` prints one ``RESULT`` JSON
line).  tests/test_bnjudge_cpu.py turns the judge on an fp32 CPU model of the passes and on mutations of it.  Not a conftest.

Operands (seeded CPU generators, rounded to the dtype): x ~ 2 N(0,1) + 3 per channel; channel 0 at mean 50 / std 0.1 (the case the
pivot exists for); the last channel's first element -- its pivot -- an outlier at +40; dy ~ N(0,1); gamma in [0.5, 1.5], beta ~
N(1,1), so that pre-activations fall on both sides of 0 and of 6 (between 5 % and 95 % of every case is open: a condition on the
inputs, met by walking the seed); random running statistics; momentum 0.1, eps 1e-5 as the fp32 values the entry points receive.

Truth: fp64 on those operands, per channel: mu, biased var, invstd, the unbiased running update, a = gamma invstd, b = beta - mu a,
y = act(a x + b).  The backward truth is the fp64 formula on the forward KERNEL's own save_mean / save_invstd (widened) with the
mask taken from the forward kernel's stored y ((y > 0) & (y < 6) | y > 0: the kernels' contract, "recomputed from the rounded
pre-activation"): the backward pass is judged alone, no element is excluded, no model of FMA contraction is needed.

Bars.  u = 2^-24, eps = dwjudge.EPS (2^-8 bf16, 2^-10 fp16), D = ``depth``.  With the pivot k, m1 = mean(x - k), A1 = mean|x - k|,
A2 = mean (x - k)^2 over the channel, M = N HW:
  save_mean     (D+2) u A1 + 2u (|k| + |m1|)          terms x-k rounded once, D additions, one division; k + m1 rounded once
  variance      bvar = (D+3) u A2 + 2 |m1| (D+2) u A1 + 4u (A2 + m1^2)
  save_invstd   1/2 invstd^3 bvar + 4u invstd           first order in bvar; var + eps, sqrt, division rounded once each
  running_*     momentum x the bar (x M/(M-1) for the variance) + 3u |result|
  a             |gamma| bar_invstd + u |a|
  b             |a| bar_mean + |mu| bar_a + u |mu a| + u |b|
  y             |x| bar_a + bar_b + 2u (|a x| + |b|)  [+ eps |want| in 16 bit]; the clamp is 1-Lipschitz, the bar passes through
  dbeta         D u sum|g|
  dgamma        (D+4) u sum|g xhat|
  dx            4u (|a g| + |k1 x| + |k1 mu| + |a sum(g)/M|) + |a|/M (bar_dbeta + |xhat| bar_dgamma)  [+ eps |want| in 16 bit]
Handed-over sums (``_fwd_sums``, ``_stats`` / ``ssdk_bn_sync_local_stats`` with ``sums``): the same formulas with k = 0 and D = 0
(the fp64 sums rounded to fp32 are handed over; the finalize adds nothing up).  Those bars widen with (mean / std)^2 -- what
pivot-0 arithmetic can promise -- so the hand-over is judged on operands WITHOUT the 50 / 0.1 channel (asserted: bar_invstd /
invstd <= 1e-3 there), and for the 50 / 0.1 channel the achieved error and both bars are only printed.
Split path: the same bars with the masses about the common pivot P widened by each rank's |pivot_r - P| and D increased by the
number of ranks.  "eps |want|" is the rounding to a 16-bit NORMAL number; below the format's smallest normal number the rounding is
absolute, so every 16-bit bar also carries the spacing of the subnormals (2^-24 in fp16, 2^-133 in bf16: the one-hot gradients'
dx ~ 1e-5 is subnormal in fp16).  No other tolerance exists here; the exact checks (counts, integers, constants, one-hot
gradients, bit equality under misalignment) have none."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "ssds.pytorch_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import torch  # noqa: E402

import guardband as G  # noqa: E402
from dwjudge import CODES, DTYPES, EPS, U, _equal, _say, new_rec, sid  # noqa: E402

DEPTH_CAP = 256
MOMENTUM = float(torch.tensor(0.1, dtype=torch.float32))  # the fp32 values the entry points receive
BN_EPS = float(torch.tensor(1e-5, dtype=torch.float32))
ACTS = (0, 1, 2)  # 0 none | 1 ReLU6 | 2 ReLU
DTYPE_NAMES = ("f32", "bf16", "f16")
CHUNK = 8192  # kBnChunk: elements per workgroup of the flat apply pass
ONE_HOT = -1.3125
TINY = {"bf16": 2.0 ** -133, "f16": 2.0 ** -24}  # the spacing of the format's subnormals

# (N, C, H, W): the smallest shapes that reach each branch
CASES = [(2, 3, 1, 1),        # M = 2; no vector, tails only; in the flat apply every element is its own plane, the channel wraps mod 3
         (3, 5, 3, 3),        # one vector + tail (16 bit), two + one (fp32); vectors straddle planes
         (70, 3, 10, 10),     # 81 planes per apply workgroup, ragged last workgroup; split 64 with one or two planes per slice
         (5, 7, 19, 19),      # odd plane: 2-byte-aligned plane bases
         (4, 32, 16, 24),     # aligned planes: per-plane vector apply by default, flat only under the switch
         (66, 16, 8, 8),      # split 64, N not a multiple of it
         (3, 1100, 2, 4),     # C > 1024: split 1; HW equals one 16-bit vector; C no multiple of 64 for bn_fwd_finalize_kernel
         (2, 2, 128, 64),     # exactly one 8192-element chunk
         (1, 2, 91, 91),      # one chunk plus 89 elements (11 vectors + 1); N = 1
         (2, 6, 150, 150)]    # three chunks, ragged last; three reduction trips; HW % 8 = 4, % 4 = 0: fp32 vector-eligible, 16 bit not
ONEHOT_CASES = [(3, 5, 3, 3), (70, 3, 10, 10), (66, 16, 8, 8), (2, 2, 128, 64), (2, 6, 150, 150)]
ALIGN_CASES = [(3, 5, 3, 3), (5, 7, 19, 19), (4, 32, 16, 24)]
OFFSETS = {"x": 1, "dy": 3, "y": 5, "dx": 7}  # elements into a 256-byte-aligned interior
SPLIT_CASES = [(11, 5, 19, 19), (11, 5, 32, 32)]
SPLIT_RANKS = [[4, 0, 1, 6], [11]]
FAMILIES = {"default": None, "per_plane": "0", "flat": "1"}  # SSDK_BN_FLAT
REDUCE = {"default": "bn_reduce_flat_kernel", "per_plane": "bn_reduce_kernel", "flat": "bn_reduce_flat_kernel"}
FINALIZE = "bn_fwd_finalize_kernel"


def family_of_this_process():
    v = os.environ.get("SSDK_BN_FLAT")
    return {None: "default", "2": "default", "0": "per_plane", "1": "flat"}[v]


def vec_width(dtype_name):
    return 4 if dtype_name == "f32" else 8


def bn_split(n, c):
    """mirrors bn_split of csrc/ssdk_bntrain.hip: min(ceil(1024 / C), N, 64), at least 1"""
    return max(1, min((1024 + c - 1) // c, n, 64))


def workspace_bytes(n, c):
    """mirrors ssdk_bn_workspace_bytes: tickets [C] | partials [C][split][2] | coefficients [C][4], each part rounded up to 4 words"""
    r4 = lambda v: (v + 3) // 4 * 4  # noqa: E731
    return (r4(c) + r4(c * bn_split(n, c) * 2) + c * 4) * 4


def depth(n, c, hw, dtype_name, ranks=0):
    """D: the longest chain of fp32 additions one term of a per-channel sum passes through.

    A workgroup (c, s) owns the np = ceil(N / split) planes n = s, s + split, ... of its channel (``bn_split``).
      * bn_reduce_flat_kernel: its 256 threads stride over the np * (HW // VN) vectors of those planes as one list (thread t takes
        vectors t, t + 256, ..., VN elements each, added one by one into the thread's accumulator), then over the np * (HW % VN)
        tail elements: ceil(np (HW // VN) / 256) VN + ceil(np (HW % VN) / 256) additions per thread;
      * bn_reduce_kernel: plane by plane, ceil(HW / (256 VN)) VN additions per plane with vectors (HW % VN == 0), ceil(HW / 256)
        without: np times that per thread;
      * block_sum2: six butterfly steps inside a wave (+ 6), then ((w0 + w1) + w2) + w3 over the four waves (+ 3);
      * bn_fold_finalize: the ``split`` partials of the channel added in index order (+ split);
      * the split path: the ranks' records added in rank order (+ ranks).
    The larger of the two kernels' per-thread counts is taken, so one bar serves every family."""
    vn = vec_width(dtype_name)
    split = bn_split(n, c)
    planes = (n + split - 1) // split
    vpp, tail = divmod(hw, vn)
    flat = (planes * vpp + 255) // 256 * vn + (planes * tail + 255) // 256
    per_plane = planes * ((vpp + 255) // 256 * vn if tail == 0 else (hw + 255) // 256)
    d = max(flat, per_plane) + 6 + 3 + split + ranks
    assert d <= DEPTH_CAP, "depth %d of (N %d, C %d, HW %d, %s) is above the cap: the bars are first-order in D u" % (d, n, c, hw, dtype_name)
    return d


# ---- operands ------------------------------------------------------------------------------------------------------------------------
def act_fn(v, act):
    if act:
        v = v.clamp(min=0)
    if act == 1:
        v = v.clamp(max=6)
    return v


def open_mask(y, act):
    """the activation's pass-through mask on a stored output (hardtanh_backward / threshold_backward: open interval)"""
    y = y.double()
    return torch.ones_like(y, dtype=torch.bool) if act == 0 else ((y > 0) & (y < 6) if act == 1 else y > 0)


def _draw(shape, dtype_name, seed, special):
    n, c, h, w = shape
    dtype = DTYPES[dtype_name]
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, c, h, w, generator=g) * 2 + 3
    if special:
        x[:, 0] = 50 + 0.1 * torch.randn(n, h, w, generator=g)
    x[0, c - 1, 0, 0] = 40.0
    dy = torch.randn(n, c, h, w, generator=g)
    return {"x": x.to(dtype), "dy": dy.to(dtype), "gamma": torch.rand(c, generator=g) + 0.5, "beta": torch.randn(c, generator=g) + 1.0,
            "rm": torch.randn(c, generator=g) * 0.2, "rv": torch.rand(c, generator=g) + 0.5}


def open_shares(op):
    """share of the case's elements whose fp64 pre-activation lies in (0, 6), and in (0, inf)"""
    x = op["x"].double()
    mu, var = x.mean((0, 2, 3), keepdim=True), x.var((0, 2, 3), unbiased=False, keepdim=True)
    pre = (x - mu) / (var + BN_EPS).sqrt() * op["gamma"].double().view(1, -1, 1, 1) + op["beta"].double().view(1, -1, 1, 1)
    return float(((pre > 0) & (pre < 6)).double().mean()), float((pre > 0).double().mean())


def operands(shape, dtype_name, special=True):
    """special: channel 0 at 50 / 0.1 (False: the hand-over's operands).  The seed walks on from a value fixed by the case until
    between 5 % and 95 % of the elements are open under both activations (six-element cases need it)."""
    n, c, h, w = shape
    base = 1000 * n + 100 * c + 7 * h + 3 * w + CODES[dtype_name] + (0 if special else 500000)
    for step in range(64):
        op = _draw(shape, dtype_name, base + 7919 * step, special)
        if all(0.05 <= s <= 0.95 for s in open_shares(op)):
            return op
    raise AssertionError("no seed gives %s an open share between 5 %% and 95 %%" % (shape,))


# ---- truth and bars ------------------------------------------------------------------------------------------------------------------
def _cv(t):
    return t.view(1, -1, 1, 1)


def forward_truth(op, act, dtype_name, pivot, d, exact_sums=False, spread=None):
    """-> {quantity: (want, bar)} for mean, invstd, rm, rv, a, b, y.  pivot [C] fp64; d the depth; exact_sums: both pivot sums are
    exact (integers), the D terms of the bars vanish; spread [N, C] fp64: |pivot_r - P| of the element's rank (split path)."""
    x = op["x"].double()
    n, c, h, w = x.shape
    m = n * h * w
    dims = (0, 2, 3)
    mu, var = x.mean(dims), x.var(dims, unbiased=False)
    invstd = 1 / (var + BN_EPS).sqrt()
    dev = (x - _cv(pivot)).abs()
    if spread is not None:
        dev = dev + spread.view(n, -1, 1, 1)
    m1 = (x - _cv(pivot)).mean(dims)
    a1, a2 = dev.mean(dims), dev.pow(2).mean(dims)
    ds = 0.0 if exact_sums else 1.0
    dm1 = ds * (d + 2) * U * a1
    bar_mean = dm1 + 2 * U * (pivot.abs() + m1.abs())
    bvar = ds * (d + 3) * U * a2 + 2 * m1.abs() * dm1 + 4 * U * (a2 + m1 * m1)
    bar_invstd = 0.5 * invstd.pow(3) * bvar + 4 * U * invstd
    unb = m / (m - 1.0) if m > 1 else 1.0
    rm = (1 - MOMENTUM) * op["rm"].double() + MOMENTUM * mu
    rv = (1 - MOMENTUM) * op["rv"].double() + MOMENTUM * var * unb
    gamma, beta = op["gamma"].double(), op["beta"].double()
    a = gamma * invstd
    b = beta - mu * a
    bar_a = gamma.abs() * bar_invstd + U * a.abs()
    bar_b = a.abs() * bar_mean + mu.abs() * bar_a + U * (mu * a).abs() + U * b.abs()
    pre = x * _cv(a) + _cv(b)
    y = act_fn(pre, act)
    bar_y = x.abs() * _cv(bar_a) + _cv(bar_b) + 2 * U * ((x * _cv(a)).abs() + _cv(b.abs()))
    if dtype_name != "f32":
        bar_y = bar_y + EPS[dtype_name] * y.abs() + TINY[dtype_name]
    return {"mean": (mu, bar_mean), "invstd": (invstd, bar_invstd), "rm": (rm, MOMENTUM * bar_mean + 3 * U * rm.abs()),
            "rv": (rv, MOMENTUM * unb * bvar + 3 * U * rv.abs()), "a": (a, bar_a), "b": (b, bar_b), "y": (y, bar_y), "var": (var, bvar)}


def backward_truth(op, dy, y_stored, mean, invstd, act, dtype_name, d, planes=None, extra=None):
    """fp64 formula on the forward kernel's own mean / invstd [C] and the mask of its stored y -> {dbeta, dgamma, dx: (want, bar)}.
    planes: a slice of the batch whose LOCAL sums dbeta / dgamma are wanted (split path; dx always over the whole batch).
    extra: (bar_dbeta, bar_dgamma) to use for dx instead of the local ones (split path: the ranks' bars added up)."""
    x = op["x"].double()
    n, c, h, w = x.shape
    m = n * h * w
    dims = (0, 2, 3)
    mu, istd = mean.double().cpu(), invstd.double().cpu()
    g = dy.double() * open_mask(y_stored.cpu(), act)
    xh = (x - _cv(mu)) * _cv(istd)
    sl = slice(None) if planes is None else planes
    sg, sgx = g[sl].sum(dims), (g[sl] * xh[sl]).sum(dims)
    bar_db, bar_dg = d * U * g[sl].abs().sum(dims), (d + 4) * U * (g[sl] * xh[sl]).abs().sum(dims)
    tg, tgx = g.sum(dims), (g * xh).sum(dims)
    a = op["gamma"].double() * istd
    k1 = -a * istd * tgx / m
    dx = _cv(a) * (g - _cv(tg) / m - xh * _cv(tgx) / m)
    e_db, e_dg = (bar_db, bar_dg) if extra is None else extra
    bar_dx = (4 * U * ((_cv(a) * g).abs() + (_cv(k1) * x).abs() + _cv((k1 * mu).abs()) + _cv((a * tg / m).abs()))
              + _cv(a.abs()) / m * (_cv(e_db) + xh.abs() * _cv(e_dg)))
    if dtype_name != "f32":
        bar_dx = bar_dx + EPS[dtype_name] * dx.abs() + TINY[dtype_name]
    return {"dbeta": (sg, bar_db), "dgamma": (sgx, bar_dg), "dx": (dx, bar_dx)}


def judge(rec, got, tr, keys=None, tag=""):
    """got {name: tensor}, tr {name: (want, bar)} -> a ratio and a line per quantity, a failure per miss"""
    for k in (keys or tr):
        if k in got and got[k] is not None and k in tr:
            want, bar = tr[k]
            _say(rec, tag + k, (got[k].double().cpu() - want).abs(), bar)
    return rec


# ---- an fp32 CPU model of the passes: pivot sums in the kernels' order, bn_fwd_out, bn_bwd_coef, apply, one rounding --------------------
def _thread_order(planes, hw, vn, family):
    """-> idx [256, T] (int64, -1 = no term): the positions (plane * hw + i, planes of one workgroup laid end to end) thread t adds,
    in its order.  flat: bn_reduce_flat_kernel; per_plane: bn_reduce_kernel."""
    import numpy as np

    vpp, tail = divmod(hw, vn)
    thr, key, pos = [], [], []
    if family == "flat":
        v = np.arange(planes * vpp)
        for e in range(vn):
            thr.append(v % 256)
            key.append(v // 256 * vn + e)
            pos.append(v // max(vpp, 1) * hw + v % max(vpp, 1) * vn + e)
        tv = (planes * vpp + 255) // 256 * vn
        t = np.arange(planes * tail)
        thr.append(t % 256)
        key.append(tv + t // 256)
        pos.append(t // max(tail, 1) * hw + vpp * vn + t % max(tail, 1))
    else:
        j = np.repeat(np.arange(planes), hw)
        i = np.tile(np.arange(hw), planes)
        if tail == 0:
            q, e = i // vn, i % vn
            per = (vpp + 255) // 256
            thr.append(q % 256)
            key.append((j * per + q // 256) * vn + e)
        else:
            per = (hw + 255) // 256
            thr.append(i % 256)
            key.append(j * per + i // 256)
        pos.append(j * hw + i)
    thr, key, pos = (np.concatenate(v).astype(np.int64) for v in (thr, key, pos))
    idx = np.full((256, int(key.max()) + 1 if key.size else 1), -1, dtype=np.int64)
    idx[thr, key] = pos
    assert (idx >= 0).sum() == planes * hw
    return torch.from_numpy(idx)


def _block_sum(acc):
    """acc [C, 256] fp32 -> [C]: block_sum2 as lane 0 of each wave sees it, then the four waves in order"""
    c = acc.shape[0]
    v = acc.view(c, 4, 64)
    lanes = torch.arange(64)
    for dd in (32, 16, 8, 4, 2, 1):
        v = v + v[:, :, lanes ^ dd]
    r = v[:, :, 0]
    return ((r[:, 0] + r[:, 1]) + r[:, 2]) + r[:, 3]


def _reduce(terms_a, terms_b, n, hw, vn, family, split, skip_last_of_plane=False, skip_slice=None):
    """terms_* [N, C, HW] fp32 (the addends of the two sums, already formed in fp32) -> s1, s2 [C] fp32 in the kernels' order"""
    c = terms_a.shape[1]
    s1, s2 = torch.zeros(c), torch.zeros(c)
    for s in range(split):
        if s == skip_slice:
            continue
        planes = (n - s + split - 1) // split
        idx = _thread_order(planes, hw, vn, family)
        if skip_last_of_plane:
            idx = torch.where(idx % hw == hw - 1, torch.full_like(idx, -1), idx)
        pad = idx < 0
        idx = idx.clamp(min=0)
        acc = []
        for t in (terms_a, terms_b):
            flat = t[s::split].permute(1, 0, 2).reshape(c, planes * hw)
            tt = flat[:, idx.reshape(-1)].view(c, 256, -1).masked_fill(pad.view(1, 256, -1), 0.0)
            a = torch.zeros(c, 256)
            for j in range(tt.shape[2]):
                a = a + tt[:, :, j]
            acc.append(_block_sum(a))
        s1, s2 = s1 + acc[0], s2 + acc[1]
    return s1, s2


def _round(v, dtype_name):
    return v.to(DTYPES[dtype_name])


def _chan_map(n, c, hw, vn, straddle_mutation):
    """channel whose coefficients each element takes in the apply pass [N, C, HW]; the mutation: the last element of a vector of
    the flat apply pass that straddles two planes takes the channel of the vector's first element"""
    chan = torch.arange(c).view(1, c, 1).expand(n, c, hw).contiguous()
    if straddle_mutation and hw < CHUNK and hw % vn:
        g = CHUNK // hw
        flat = torch.arange(n * c * hw)
        le = flat % (g * hw)
        first = flat - (vn - 1)
        nvec = torch.minimum(torch.full_like(flat, g * hw), (n * c - flat // (g * hw) * g) * hw) // vn
        hit = (le % vn == vn - 1) & (le // vn < nvec) & (first // hw != flat // hw)
        cf = chan.view(-1).clone()
        cf[hit] = (first[hit] // hw) % c
        chan = cf.view(n, c, hw)
    return chan


def model(op, act, dtype_name, family="flat", sums=None, mutation=None):
    """fp32 throughout, one rounding to the dtype.  sums [C,2] fp32: the hand-over (pivot 0, no reduction).
    mutation: None | "tail" | "straddle" | "biased" | "short" | "mask6" | "slice" | "pivot0" -> everything the kernels return."""
    x = op["x"].float()
    n, c, h, w = x.shape
    hw = h * w
    vn = vec_width(dtype_name)
    split = bn_split(n, c)
    xs = x.reshape(n, c, hw)
    skip = split - 1 if (mutation == "slice" and n % split) else None
    if sums is None:
        k = xs[0, :, 0].clone()
        if mutation == "pivot0":
            k[0] = 0.0
        dd = xs - k.view(1, c, 1)
        s1, s2 = _reduce(dd, dd * dd, n, hw, vn, family, split, mutation == "tail", skip)
    else:
        k = torch.zeros(c)
        s1, s2 = sums[:, 0].clone(), sums[:, 1].clone()
    m = torch.tensor(float(n) * float(hw) - (hw if mutation == "short" else 0), dtype=torch.float32)
    m1 = s1 / m
    mean = k + m1
    var = (s2 / m - m1 * m1).clamp(min=0)
    eps, mom = torch.tensor(BN_EPS, dtype=torch.float32), torch.tensor(MOMENTUM, dtype=torch.float32)
    invstd = 1.0 / torch.sqrt(var + eps)
    unbiased = var * (m / (m - 1.0)) if float(m) > 1 and mutation != "biased" else var
    rm = (1.0 - mom) * op["rm"] + mom * mean
    rv = (1.0 - mom) * op["rv"] + mom * unbiased
    a = op["gamma"] * invstd
    b = op["beta"] - mean * a
    chan = _chan_map(n, c, hw, vn, mutation == "straddle")
    y = _round(act_fn(xs * a[chan] + b[chan], act), dtype_name)
    out = {"mean": mean, "invstd": invstd, "rm": rm, "rv": rv, "a": a, "b": b, "y": y.view(n, c, h, w),
           "coef": torch.stack([a, b, torch.zeros(c), torch.zeros(c)], 1)}

    # backward: the mask recomputed from the rounded pre-activation
    def opened(aa, bb):
        v = _round(xs * aa + bb, dtype_name).float()
        if act == 0:
            return torch.ones_like(v, dtype=torch.bool)
        if act == 1:
            return (v > 0) & ((v <= 6) if mutation == "mask6" else (v < 6))
        return v > 0

    gy = op["dy"].float().reshape(n, c, hw)
    g = gy * opened(a.view(1, c, 1), b.view(1, c, 1))
    d = xs - mean.view(1, c, 1)
    sg, sgx = _reduce(g, g * d * invstd.view(1, c, 1), n, hw, vn, family, split, mutation == "tail", skip)
    k1 = -a * invstd * sgx / m
    k0 = -a * sg / m - k1 * mean
    ga = gy * opened(a[chan], b[chan])
    out.update(dbeta=sg, dgamma=sgx, dx=_round(ga * a[chan] + xs * k1[chan] + k0[chan], dtype_name).view(n, c, h, w))
    return out


def exact_sums32(x):
    """the fp64 sums (x, x^2) of every channel rounded to fp32: what a producer hands over"""
    x = x.double()
    return torch.stack([x.sum((0, 2, 3)), x.pow(2).sum((0, 2, 3))], 1).float().contiguous()


# ---- running the kernels (entry points on the calling thread: ssdk_last_kernel is per thread) ----------------------------------------
def _lib():
    from ssds import _native as N

    return N, N.lib, N.stream_ptr(torch.device("cuda"))


def _ws(n, c):
    N, L, _ = _lib()
    need = int(L.ssdk_bn_workspace_bytes(max(n, 1), c))
    return torch.zeros(need, dtype=torch.uint8, device="cuda"), need  # (zero ticket words: include/ssdk.h)


def _ptr(t):
    return t.data_ptr() if t.numel() else None


def device_operands(op):
    return {k: v.cuda() for k, v in op.items()}


def run_fwd(dv, act, y=None, sums=None, stats_only=False):
    """dv: operands on the device.  -> {y, mean, invstd, rm, rv, coef, name}"""
    N, L, st = _lib()
    x = dv["x"]
    n, c, h, w = (int(v) for v in x.shape)
    hw = h * w
    rm, rv = dv["rm"].clone(), dv["rv"].clone()
    mean, invstd = torch.full((c,), float("nan"), device="cuda"), torch.full((c,), float("nan"), device="cuda")
    ws, need = _ws(n, c)
    dc = N.dtype_code(x)
    coef = None
    sp = None if sums is None else sums.data_ptr()
    if stats_only:
        coef = torch.full((c, 4), float("nan"), device="cuda")
        N.check(L.ssdk_bn_act_train_stats(x.data_ptr(), sp, dv["gamma"].data_ptr(), dv["beta"].data_ptr(), rm.data_ptr(), rv.data_ptr(),
                                          mean.data_ptr(), invstd.data_ptr(), coef.data_ptr(), ws.data_ptr(), need, n, c, hw, MOMENTUM,
                                          BN_EPS, dc, st), "bn_train_stats")
    else:
        y = torch.full_like(x, float("nan")) if y is None else y
        if sums is None:
            N.check(L.ssdk_bn_act_train_fwd(x.data_ptr(), dv["gamma"].data_ptr(), dv["beta"].data_ptr(), rm.data_ptr(), rv.data_ptr(),
                                            y.data_ptr(), mean.data_ptr(), invstd.data_ptr(), ws.data_ptr(), need, n, c, hw, MOMENTUM,
                                            BN_EPS, act, dc, st), "bn_train_fwd")
        else:
            N.check(L.ssdk_bn_act_train_fwd_sums(x.data_ptr(), sp, dv["gamma"].data_ptr(), dv["beta"].data_ptr(), rm.data_ptr(),
                                                 rv.data_ptr(), y.data_ptr(), mean.data_ptr(), invstd.data_ptr(), ws.data_ptr(), need,
                                                 n, c, hw, MOMENTUM, BN_EPS, act, dc, st), "bn_train_fwd_sums")
    name = N.last_kernel()
    torch.cuda.synchronize()
    out = {"y": y, "mean": mean, "invstd": invstd, "rm": rm, "rv": rv, "coef": coef, "name": name}
    if coef is not None:
        out["a"], out["b"] = coef[:, 0], coef[:, 1]
    return out


def run_bwd(dv, dy, mean, invstd, act, dx=None):
    N, L, st = _lib()
    x = dv["x"]
    n, c, h, w = (int(v) for v in x.shape)
    dx = torch.full_like(x, float("nan")) if dx is None else dx
    dw, db = torch.full((c,), float("nan"), device="cuda"), torch.full((c,), float("nan"), device="cuda")
    ws, need = _ws(n, c)
    N.check(L.ssdk_bn_act_train_bwd(x.data_ptr(), dy.data_ptr(), dv["gamma"].data_ptr(), dv["beta"].data_ptr(), mean.data_ptr(),
                                    invstd.data_ptr(), dx.data_ptr(), dw.data_ptr(), db.data_ptr(), ws.data_ptr(), need, n, c, h * w,
                                    act, N.dtype_code(x), st), "bn_train_bwd")
    name = N.last_kernel()
    torch.cuda.synchronize()
    return {"dx": dx, "dgamma": dw, "dbeta": db, "name": name}


def split_path(shards, dys, weight, bias, rm, rv, momentum, eps, act, sums=None):
    """Every shard as one rank: local records -> stacked (the all-gather) -> merge -> apply; backward the same way."""
    N, L, st = _lib()
    c = int(shards[0].shape[1])
    hw = int(shards[0].shape[2] * shards[0].shape[3])
    sends = []
    for i, x in enumerate(shards):
        send = torch.empty(3 * c + 1, device="cuda")
        ws, need = _ws(x.shape[0], c)
        s = None if sums is None else sums[i].data_ptr()
        N.check(L.ssdk_bn_sync_local_stats(_ptr(x), s, send.data_ptr(), ws.data_ptr(), need, x.shape[0], c, hw, N.dtype_code(x), st),
                "local_stats")
        sends.append(send)
    gathered = torch.stack(sends)
    mean, invstd = torch.empty(c, device="cuda"), torch.empty(c, device="cuda")
    coef = torch.empty(c, 4, device="cuda")
    N.check(L.ssdk_bn_sync_fwd_finalize(gathered.data_ptr(), len(shards), weight.data_ptr(), bias.data_ptr(), rm.data_ptr(),
                                        rv.data_ptr(), mean.data_ptr(), invstd.data_ptr(), coef.data_ptr(), c, momentum, eps, st),
            "fwd_finalize")
    ys, bsends, dws, dbs = [], [], [], []
    for x, dy in zip(shards, dys):
        y = torch.empty_like(x)
        N.check(L.ssdk_bn_act_apply(_ptr(x), coef.data_ptr(), _ptr(y), x.shape[0], c, hw, act, N.dtype_code(x), st), "apply")
        ys.append(y)
        send, dw, db = torch.empty(2 * c, device="cuda"), torch.empty(c, device="cuda"), torch.empty(c, device="cuda")
        ws, need = _ws(x.shape[0], c)
        N.check(L.ssdk_bn_sync_bwd_local(_ptr(x), _ptr(dy), weight.data_ptr(), bias.data_ptr(), mean.data_ptr(), invstd.data_ptr(),
                                         send.data_ptr(), dw.data_ptr(), db.data_ptr(), ws.data_ptr(), need, x.shape[0], c, hw, act,
                                         N.dtype_code(x), st), "bwd_local")
        bsends.append(send)
        dws.append(dw)
        dbs.append(db)
    bgathered = torch.stack(bsends)
    dxs = []
    for x, dy in zip(shards, dys):
        dx = torch.empty_like(x)
        N.check(L.ssdk_bn_sync_bwd_apply(_ptr(x), _ptr(dy), bgathered.data_ptr(), len(shards), gathered.data_ptr(), weight.data_ptr(),
                                         bias.data_ptr(), mean.data_ptr(), invstd.data_ptr(), _ptr(dx), x.shape[0], c, hw, act,
                                         N.dtype_code(x), st), "bwd_apply")
        dxs.append(dx)
    return dict(y=ys, mean=mean, invstd=invstd, coef=coef, dx=dxs, dw=dws, db=dbs)


# ---- kernel names ----------------------------------------------------------------------------------------------------------------------
def apply_name(shape, dtype_name, family, aligned=True):
    """default: the flat apply exactly where HW is no multiple of the vector width or a pointer is misaligned"""
    hw = shape[2] * shape[3]
    if family == "per_plane":
        return "bn_apply_kernel"
    if family == "flat":
        return "bn_apply_flat_kernel"
    return "bn_apply_kernel" if (hw % vec_width(dtype_name) == 0 and aligned) else "bn_apply_flat_kernel"


def _names(rec, names, want):
    rec["names"] = (rec["names"] or []) + list(names)
    if list(names) != list(want):
        rec["failures"].append("kernels %s, expected %s" % (list(names), list(want)))


def _pivot(op):
    return op["x"][0, :, 0, 0].double()


# ---- the checks ------------------------------------------------------------------------------------------------------------------------
FWD_KEYS = ("mean", "invstd", "rm", "rv", "y")


def check_random(shape, dtype_name, family, runner=None):
    """ssdk_bn_act_train_fwd -> ssdk_bn_act_train_bwd on random operands, all three activations: every quantity per channel and per
    element.  runner: None (the kernels) or a function (op, act) -> results (the CPU model)."""
    rec = new_rec("%s %s %s" % (sid(shape), dtype_name, family))
    n, c, h, w = shape
    op = operands(shape, dtype_name)
    d = depth(n, c, h * w, dtype_name)
    dv = device_operands(op) if runner is None else None
    for act in ACTS:
        tr = forward_truth(op, act, dtype_name, _pivot(op), d)
        if runner is None:
            got = run_fwd(dv, act)
            back = run_bwd(dv, dv["dy"], got["mean"], got["invstd"], act)
            _names(rec, [got["name"], back["name"]], [REDUCE[family] + "+" + apply_name(shape, dtype_name, family)] * 2)
        else:
            got = back = runner(op, act)
        tag = "act%d " % act
        judge(rec, got, tr, FWD_KEYS, tag)
        judge(rec, back, backward_truth(op, op["dy"], got["y"], got["mean"], got["invstd"], act, dtype_name, d), None, tag)
    return rec


def check_stats(shape, dtype_name, family, runner=None):
    """the stats-only entry with and without handed-over sums, and ssdk_bn_act_train_fwd_sums: coef[:, 0:2] against (a, b),
    coef[:, 2] == 0, the statistics, y.  The hand-over is judged on operands without the 50 / 0.1 channel (k = 0, D = 0); the
    50 / 0.1 channel goes through it too and is only printed.  runner: (op, act, sums | None) -> results (the CPU model)."""
    rec = new_rec("stats %s %s %s" % (sid(shape), dtype_name, family))
    n, c, h, w = shape
    d = depth(n, c, h * w, dtype_name)
    act = 1
    op = operands(shape, dtype_name)
    tr = forward_truth(op, act, dtype_name, _pivot(op), d)
    if runner is None:
        got = run_fwd(device_operands(op), act, stats_only=True)
        _names(rec, [got["name"]], [REDUCE[family]])
    else:
        got = runner(op, act, None)
    judge(rec, got, tr, ("mean", "invstd", "rm", "rv", "a", "b"), "own sums ")
    _equal(rec, "coef[:, 2] (own sums)", got["coef"][:, 2], torch.zeros(c))
    # the hand-over: pivot 0, no reduction
    plain = operands(shape, dtype_name, special=False)
    trh = forward_truth(plain, act, dtype_name, torch.zeros(c, dtype=torch.float64), 0)
    rel = float((trh["invstd"][1] / trh["invstd"][0]).max())
    if not rel <= 1e-3:
        rec["failures"].append("operands: bar_invstd / invstd = %.3g > 1e-3 on the hand-over's operands" % rel)
    sums = exact_sums32(plain["x"])
    if runner is None:
        dv = device_operands(plain)
        st = run_fwd(dv, act, sums=sums.cuda(), stats_only=True)
        full = run_fwd(dv, act, sums=sums.cuda())
        _names(rec, [st["name"], full["name"]], [FINALIZE, FINALIZE + "+" + apply_name(shape, dtype_name, family)])
    else:
        st = full = runner(plain, act, sums)
    judge(rec, st, trh, ("mean", "invstd", "rm", "rv", "a", "b"), "handed-over stats ")
    _equal(rec, "coef[:, 2] (handed-over)", st["coef"][:, 2], torch.zeros(c))
    judge(rec, full, trh, FWD_KEYS, "handed-over fwd ")
    # the 50 / 0.1 channel through the hand-over: printed only
    sp = run_fwd(device_operands(op), act, sums=exact_sums32(op["x"]).cuda(), stats_only=True) if runner is None else \
        runner(op, act, exact_sums32(op["x"]))
    tr0 = forward_truth(op, act, dtype_name, torch.zeros(c, dtype=torch.float64), 0)
    err = abs(float(sp["invstd"][0]) - float(tr["invstd"][0][0]))
    rec["lines"].append("50/0.1 channel through the hand-over %s: |err invstd| %.3g, pivot-0 bar %.3g, pivot bar %.3g, invstd %.4g"
                        % (rec["what"], err, float(tr0["invstd"][1][0]), float(tr["invstd"][1][0]), float(tr["invstd"][0][0])))
    return rec


def count_operands(shape, dtype_name, kind):
    op = operands(shape, dtype_name)
    n, c, h, w = shape
    g = torch.Generator().manual_seed(17 * n + 5 * c + h + w)
    if kind == "integer":  # both pivot sums are exact integers below 2^24
        op["x"] = torch.randint(-8, 9, shape, generator=g).float().to(DTYPES[dtype_name])
    elif kind == "constant":  # one channel at 1000.5 (rounded to the dtype), the others at small constants
        v = (torch.arange(c).float() % 7) * 0.75 - 1.5
        v[c // 2] = 1000.5
        op["x"] = v.view(1, c, 1, 1).expand(shape).contiguous().to(DTYPES[dtype_name])
    return op


def check_counts(shape, dtype_name, family, runner=None):
    """dy = 1, no activation: dbias == N HW exactly in every channel.  x integer in [-8, 8]: save_mean within 2u (|k| + |m1|), the
    variance within 4u (A2 + m1^2).  x constant per channel: save_mean is the constant, the variance exactly 0."""
    rec = new_rec("counts %s %s %s" % (sid(shape), dtype_name, family))
    n, c, h, w = shape
    m = n * h * w
    assert 256 * m < 2 ** 24
    run = (lambda op, act: runner(op, act)) if runner else (lambda op, act: run_fwd(device_operands(op), act))
    op = operands(shape, dtype_name)
    op["dy"] = torch.ones(shape, dtype=DTYPES[dtype_name])
    if runner is None:
        dv = device_operands(op)
        f = run_fwd(dv, 0)
        back = run_bwd(dv, dv["dy"], f["mean"], f["invstd"], 0)
    else:
        back = runner(op, 0)
    _equal(rec, "dbias with dy = 1", back["dbeta"].double(), torch.full((c,), float(m), dtype=torch.float64))
    op = count_operands(shape, dtype_name, "integer")
    tr = forward_truth(op, 0, dtype_name, _pivot(op), 0, exact_sums=True)
    judge(rec, run(op, 0), tr, ("mean", "invstd"), "integer x ")
    op = count_operands(shape, dtype_name, "constant")
    got = run(op, 0)
    _equal(rec, "save_mean of constant channels", got["mean"].float(), op["x"][0, :, 0, 0].float())
    mom = torch.tensor(MOMENTUM, dtype=torch.float32)
    _equal(rec, "running_var of constant channels (variance exactly 0)", got["rv"].float(), (1.0 - mom) * op["rv"] + mom * torch.zeros(c))
    want = torch.full((c,), 1.0 / BN_EPS ** 0.5, dtype=torch.float64)
    _say(rec, "constant x invstd", (got["invstd"].double().cpu() - want).abs(), 4 * U * want)
    return rec


def onehot_positions(shape, dtype_name):
    """(n, c, i): the last element of the last plane, the first of the second plane, both sides of every seam of the apply passes
    (8192-element chunks of a large plane | groups of 8192 // HW small planes; 256 vectors of the per-plane pass) and of the first
    and the last slice seam of the reductions"""
    n, c, h, w = shape
    hw = h * w
    planes = n * c
    pos = {(n - 1, c - 1, hw - 1), (1 // c, 1 % c, 0)}
    flat = set()  # (plane, element)
    if hw >= CHUNK:
        for q in range(CHUNK, hw, CHUNK):
            flat.update({(planes - 1, q - 1), (planes - 1, q)})
    else:
        g = CHUNK // hw
        seams = list(range(g, planes, g))
        for p in seams[:2] + seams[-1:]:
            flat.update({(p - 1, hw - 1), (p, 0)})
    per = 256 * vec_width(dtype_name)
    for q in list(range(per, hw, per))[:2]:
        flat.update({(0, q - 1), (0, q)})
    pos.update((p // c, p % c, i) for p, i in flat)
    split = bn_split(n, c)
    if split < n:
        last = (n - 1) // split * split
        pos.update({(split - 1, c // 2, hw - 1), (split, c // 2, 0), (last - 1, 0, hw - 1), (last, 0, 0)})
    return sorted(pos)


def check_onehot(shape, dtype_name, family, runner=None):
    """dy one-hot, no activation: dbias holds the one value exactly, every other channel's dbias, dgamma and dx are zero, the hot
    channel's dgamma and dx within the bars"""
    rec = new_rec("onehot %s %s %s" % (sid(shape), dtype_name, family))
    n, c, h, w = shape
    op = operands(shape, dtype_name)
    d = depth(n, c, h * w, dtype_name)
    if runner is None:
        dv = device_operands(op)
        f = run_fwd(dv, 0)
        gy = torch.zeros_like(dv["x"])
    else:
        f = runner(op, 0)
    plist = onehot_positions(shape, dtype_name)
    for (pn, pc, pi) in plist:
        dy = torch.zeros(shape, dtype=DTYPES[dtype_name])
        dy.view(n, c, -1)[pn, pc, pi] = ONE_HOT
        if runner is None:
            gy.zero_()
            gy.view(n, c, -1)[pn, pc, pi] = ONE_HOT
            back = run_bwd(dv, gy, f["mean"], f["invstd"], 0)
        else:
            back = runner(dict(op, dy=dy), 0)
        want = torch.zeros(c)
        want[pc] = ONE_HOT
        at = " at %s" % ((pn, pc, pi),)
        _equal(rec, "dbias" + at, back["dbeta"].float(), want)
        others = [j for j in range(c) if j != pc]
        if others:
            _equal(rec, "dgamma of the other channels" + at, back["dgamma"].float()[others], torch.zeros(len(others)))
            _equal(rec, "dx of the other channels" + at, back["dx"].float()[:, others], torch.zeros(n, len(others), h, w))
        tr = backward_truth(dict(op, dy=dy), dy, f["y"], f["mean"], f["invstd"], 0, dtype_name, d)
        sub = new_rec(rec["what"])
        judge(sub, back, tr, ("dgamma", "dx"))
        for k, v in sub["ratios"].items():
            rec["ratios"][k] = max(rec["ratios"].get(k, 0.0), v)
        rec["failures"] += [f_ + at for f_ in sub["failures"]]
    rec["lines"].append("onehot %s: %d positions, worst |err| / bar: dgamma %.3f dx %.3f"
                        % (rec["what"], len(plist), rec["ratios"].get("dgamma", 0.0), rec["ratios"].get("dx", 0.0)))
    return rec


def carve(t, offset, output=False):
    """``t`` as a contiguous device view ``offset`` elements into the interior of a guardband allocation (guards and the rest of
    the interior NaN; an output's own elements NaN too) -> storage, view"""
    storage, inner = G.guarded_like((t.numel() + 8,), t.dtype, device="cuda")
    view = inner[offset:offset + t.numel()].view(t.shape)
    if not output:
        view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % 16 == (offset * t.element_size()) % 16
    return storage, view


def check_alignment(shape, dtype_name, family):
    """x, dy, y, dx carved 1 / 3 / 5 / 7 elements into NaN-filled guardband allocations, forward and backward (ReLU6): guards intact,
    inputs unchanged, no NaN in any output, the bits of the aligned call"""
    rec = new_rec("align %s %s %s" % (sid(shape), dtype_name, family))
    act = 1
    op = operands(shape, dtype_name)
    dv = device_operands(op)
    f0 = run_fwd(dv, act)
    b0 = run_bwd(dv, dv["dy"], f0["mean"], f0["invstd"], act)
    sx, xv = carve(dv["x"], OFFSETS["x"])
    sd, dyv = carve(dv["dy"], OFFSETS["dy"])
    sy, yv = carve(dv["x"], OFFSETS["y"], output=True)
    sdx, dxv = carve(dv["x"], OFFSETS["dx"], output=True)
    before = [s.clone() for s in (sx, sd)]
    dm = dict(dv, x=xv, dy=dyv)
    f1 = run_fwd(dm, act, y=yv)
    b1 = run_bwd(dm, dyv, f1["mean"], f1["invstd"], act, dx=dxv)
    flat = apply_name(shape, dtype_name, family, aligned=False)
    _names(rec, [f1["name"], b1["name"]], [REDUCE[family] + "+" + flat] * 2)
    for k, a, b in [("y", f1["y"], f0["y"]), ("dx", b1["dx"], b0["dx"])] + [(k, f1[k], f0[k]) for k in ("mean", "invstd", "rm", "rv")] + \
            [(k, b1[k], b0[k]) for k in ("dgamma", "dbeta")]:
        if G.has_nan(a):
            rec["failures"].append(k + ": NaN (a guard was read, or an element never written)")
        if not G.same_bits(a.contiguous(), b.contiguous()):
            rec["failures"].append(k + ": not the bits of the aligned call")
    for k, s, v in (("x", sx, xv), ("dy", sd, dyv), ("y", sy, yv), ("dx", sdx, dxv)):
        if not G.guards_intact(s, v):
            rec["failures"].append(k + ": written outside the tensor")
    for k, s, was in (("x", sx, before[0]), ("dy", sd, before[1])):
        if not torch.equal(s, was):
            rec["failures"].append(k + ": an input allocation was written")
    rec["lines"].append("align %s: kernels %s" % (rec["what"], rec["names"]))
    return rec


def check_split(shape, dtype_name, sizes):
    """the emulated ranks ``sizes`` through the split entry points, per channel: the bars of the local path, masses about the common
    pivot widened by each rank's |pivot_r - P|, D increased by the number of ranks"""
    rec = new_rec("split %s %s ranks %s" % (sid(shape), dtype_name, sizes))
    n, c, h, w = shape
    op = operands(shape, dtype_name)
    dv = device_operands(op)
    live = [s for s in sizes if s]
    d = max(depth(s, c, h * w, dtype_name) for s in live) + len(sizes)
    starts = [sum(sizes[:i]) for i in range(len(sizes))]
    first = next(st for st, s in zip(starts, sizes) if s)
    piv = op["x"][first, :, 0, 0].double()
    spread = torch.zeros(n, c, dtype=torch.float64)
    for st, s in zip(starts, sizes):
        if s:
            spread[st:st + s] = (op["x"][st, :, 0, 0].double() - piv).abs()
    for act in ACTS:
        rm, rv = dv["rm"].clone(), dv["rv"].clone()
        got = split_path([t.contiguous() for t in torch.split(dv["x"], sizes)], [t.contiguous() for t in torch.split(dv["dy"], sizes)],
                         dv["gamma"], dv["beta"], rm, rv, MOMENTUM, BN_EPS, act)
        torch.cuda.synchronize()
        tr = forward_truth(op, act, dtype_name, piv, d, spread=spread)
        res = {"mean": got["mean"], "invstd": got["invstd"], "rm": rm, "rv": rv, "y": torch.cat(got["y"]),
               "a": got["coef"][:, 0], "b": got["coef"][:, 1]}
        tag = "act%d " % act
        judge(rec, res, tr, FWD_KEYS + ("a", "b"), tag)
        bars = [torch.zeros(c, dtype=torch.float64), torch.zeros(c, dtype=torch.float64)]
        mass = [torch.zeros(c, dtype=torch.float64), torch.zeros(c, dtype=torch.float64)]
        for r, (st, s) in enumerate(zip(starts, sizes)):
            if not s:
                if float(got["dw"][r].abs().max()) != 0 or float(got["db"][r].abs().max()) != 0:
                    rec["failures"].append("the empty rank has a gradient")
                continue
            loc = backward_truth(op, op["dy"], res["y"], got["mean"], got["invstd"], act, dtype_name, depth(s, c, h * w, dtype_name),
                                 planes=slice(st, st + s))
            judge(rec, {"dbeta": got["db"][r], "dgamma": got["dw"][r]}, loc, ("dbeta", "dgamma"), tag + "rank %d " % r)
            bars[0], bars[1] = bars[0] + loc["dbeta"][1], bars[1] + loc["dgamma"][1]
            mass[0], mass[1] = mass[0] + loc["dbeta"][0].abs(), mass[1] + loc["dgamma"][0].abs()
        extra = (bars[0] + len(sizes) * U * mass[0], bars[1] + len(sizes) * U * mass[1])  # the records added in rank order
        whole = backward_truth(op, op["dy"], res["y"], got["mean"], got["invstd"], act, dtype_name, d, extra=extra)
        judge(rec, {"dx": torch.cat(got["dx"])}, whole, ("dx",), tag)
    return rec


# ---- the case lists of a forced family's child process (ids are known to the parent without running it) ------------------------------
def child_cases():
    cases = []
    for dt in DTYPE_NAMES:
        cases += [("random", sh, dt) for sh in CASES]
        cases += [("counts", sh, dt) for sh in CASES]
        cases += [("onehot", sh, dt) for sh in ONEHOT_CASES]
        cases += [("align", sh, dt) for sh in ALIGN_CASES]
    return cases


def case_id(case):
    return "%s-%s-%s" % (case[0], sid(case[1]), case[2])


CHECKS = {"random": check_random, "counts": check_counts, "onehot": check_onehot, "align": check_alignment, "stats": check_stats}


def main(argv):
    if len(argv) != 2 or argv[0] != "--family" or argv[1] not in ("per_plane", "flat"):
        print("usage: bnjudge.py --family per_plane|flat   (with SSDK_BN_FLAT=0|1 in the environment)")
        return 2
    if os.environ.get("SSDK_BN_FLAT") != FAMILIES[argv[1]]:
        print("SSDK_BN_FLAT=%s is not set: this process would run another family" % FAMILIES[argv[1]])
        return 2
    out = {}
    for case in child_cases():
        rec = CHECKS[case[0]](case[1], case[2], argv[1])
        for line in rec["lines"]:
            print(line)
        out[case_id(case)] = rec
    print("RESULT " + json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
