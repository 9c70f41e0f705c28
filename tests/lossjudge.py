"""The judge of the fused loss kernels (csrc/ssdk_match.hip: match_kernel<1|2>, mine_select_kernel, mine_apply_kernel, loss_finalize_kernel)
behind ssds/core/fused_loss.py::match_loss.  Operands, the fp64 truth with its absolute-value masses, the bars, the case lists, an fp32 CPU
model with its mutations, and the checks tests/test_gpu_loss.py runs.  tests/test_lossjudge_cpu.py turns the judge on the model and on the
mutations.  Plain torch / numpy, importable on the CPU.  Not a conftest.

Truth.  The assignment (depth, label, winning box of every anchor) is oracle/box_oracle.py::extract_targets, numpy in the fp32 arithmetic of
the reference; the kernel's assignment must equal it on every anchor (the foreground count is compared exactly, every gradient depends on
it).  The winning box is recovered from the oracle alone: the first valid row whose fp32 encoding against the anchor is the oracle's
box_target, bit for bit.  Everything else is fp64 on the stored inputs (logits and box predictions rounded to the case's dtype, then
widened): the deltas by box2delta in fp64 on the fp32 corner coordinates, focal / BCE / smooth-L1 values and gradients in closed form,
the IoU-family values and gradients by fp64 autograd through criterion.IOULoss, the mined set by its definition (criterion.py
MultiBoxLoss.forward), the three sums with the absolute-value mass of each.

Bars.  u = 2^-24; eps = 2^-8 (bf16), 2^-10 (fp16), 2u (fp32); tiny = the flush threshold of the stored type, 2^-24 (fp16), 2^-126
otherwise.  No other tolerance exists in this file.  The gradients are judged after a backward with the scale s = 0.37 / #foreground
(fused_loss._MatchLoss.backward: stored gradient x fp32 scalar, stored again), so the store term is 2 eps |want| with want = s x truth;
the two stores together lose at most tiny (fp16: two half-spacings of the subnormals; otherwise s tiny + a subnormal spacing).
Every count below is in units of u, first order, for the operations of the kernel's own comment block; the compiler flags keep IEEE
division and no contraction (csrc/Makefile), so +, -, x, / and a constant's conversion cost 1 each (relative), v_exp_f32 / v_log_f32 and
ocml's expf / logf 2 (one ulp), ocml's log1pf 4.

  d_conf, focal, per element   |err| <= 2 eps |want| + tiny + D_c u (1 + |z|) |want|
      e = __expf(-|z|) = exp2(-|z| log2 e): the product and the constant's representation shift the exponent by 2 |z| log2 e u, i.e.
      the value by 2 |z| ln 2 log2 e u = 2 |z| u, plus v_exp 2: e <= 2 (1 + |z|) -- the source of the (1 + |z|) factor; every count from
      here on is in units of u (1 + |z|).  e: 3 (rounded up).  1 + e: 1 + 3 e / (1 + e) <= 2.5.  inv: 3.5.  pr, qr: inv or e x inv <=
      3 + 3.5 + 1 = 7.5.  l1p = log1pf(e): 4 + 3 (its condition number in e is <= 1) = 7.  logp, logq = -(l1p + max(-+z, 0)): both terms
      >= 0, so 7 + 1 = 8.  w = alpha or 1 - alpha: 1.  gamma v lg: 1 + 7.5 + 1 + 8 = 17.5; (gamma v lg - u): both terms <= 0, no
      cancellation, max(17.5, 7.5) + 1 = 18.5.  ug = u x u: 7.5 + 7.5 + 1 = 16.  grad = (w x ug) x (...): 1 + 16 + 1 + 18.5 + 1 = 37.5.
          D_c(gamma = 2) = 38
      general gamma: ug = __powf(u, gamma) = exp2(gamma log2 u): v_log 2 and the product 1, relative to |log2 u| <= (1 + |z|) log2 e,
      shift the value by 3 gamma (1 + |z|) ln 2 log2 e u = 3 gamma units; u's own 7.5 enter gamma-fold; v_exp 2: 10.5 gamma + 2.
          D_c(gamma) = 22 + ceil(10.5 gamma + 2)        (40 at gamma = 1.5, 30 at gamma = 0.5)
      Where ug underflows (|z| > 44 at gamma = 2) the gradient is below 2^-126 and ``tiny`` carries it.
  d_conf, MultiBoxLoss, per element   |err| <= 2 eps |want| + tiny + D_b u max(sigmoid(z), |want|),  D_b = 7
      expf (ocml, full range reduction: no |z| factor) 2; 1 + e: 1 + 2 / 2 = 2; inv 3; sigmoid = inv or e x inv <= 2 + 3 + 1 = 6; the
      gradient sigmoid - t is a subtraction of that value from 1 on the labelled class, so its error is 6 u sigmoid + 1 u |want|
      ABSOLUTE: relative to |want| = 1 - sigmoid it grows with e^z.  That is what the formula of criterion.py costs in fp32 and
      harmless (the gradient itself is below 2^-7 there), so the bar carries max(sigmoid, |want|) instead of |want|.
  d_loc, smooth-L1, per element   |err| <= 2 eps |want| + tiny + D_l u (|loc| + |delta| + 1) / beta,  D_l = 6
      The cases keep every corner coordinate exact in fp32 (integer ground truth, anchor corners at multiples of 0.5: a
      precondition), so box2delta rounds in its two divisions (1 |delta| each way: (bc - ac) / aw, bw / aw) and logf (1 absolute from
      the quotient + 2 |delta|): delta <= 1 + 2 |delta|.  d = loc - delta: 1 (|loc| + |delta|).  So d carries 3 (|loc| + |delta| + 1)
      absolute; d x (1 / beta) with beta converted to fp32: 3 |d| / beta <= 3 (|loc| + |delta|) / beta.  One bar for both branches:
      the gradient is continuous at |d| = beta.
  d_loc, IoU family, per element: the conditioning of the forward-mode chain is not derivable by counting, so it is measured.  The
      unit is u (|want| + S), S the largest of the anchor's four partials.  criterion.IOULoss in fp32 on the CPU against the fp64 truth
      gives every case its worst reference ratio; the kernel (after the store terms 2 eps |want| + tiny) is allowed 4 x that and at
      least 16 units: the same expression in another order with the device's expf and atanf, a few ulp each, over a chain about four
      operations deeper (forward-mode products).  Anchors on which the fp32 reference itself exceeds 32 units (disjoint boxes under
      GIoU, a max / min tie, a clamp edge) are left out; their share may not exceed 1 % of a case's foreground, asserted from the
      reference alone before any output is looked at.  The per-element cases draw the predictions as target deltas + N(0, 0.3); one
      case per kind draws N(0, 1.5), is judged on the anchors that remain and on loc_sum, and is exempt from the 1 % cap.  Both
      columns of every case (for loc_sum: the errors of the fp32 reference's sum and of sums[1] in units of u mass) go to the file
      SSDK_LOSSJUDGE_RATIOS names (profiles/r28_lossjudge_ratios.jsonl holds one MI355X run), with the worst |err| / bar of every
      derived bar beside them.
  sums[0], sums[1]   |err| <= (D_term + ceil(rows / 256) + 20) u mass,  mass = the fp64 sum of |terms|
      20 = the 6 + 4 adds of the workgroup tree plus the 6 + 4 of loss_finalize_kernel; rows (x 2 with mining) is recovered from
      ssdk_match_loss_workspace_bytes / 12.  D_term = ceil(sum_i b_i / (u mass)) with b_i the error bound of term i:
        focal          (ceil-free count: w 1, ug 16 or 10.5 gamma + 2, lg 8, two products 2) u (1 + |z_i|) |term_i|
        BCE            7 u |term_i|  (expf 2, log1pf 4 + 2 / 2 ... <= 6, the sum of two terms >= 0: 1)
        smooth-L1      4 u |term_i| + |L'(d_i)| 3 u (|loc| + |delta| + 1): the term's own operations (x x x, x (1 / beta), beta; or
                       x - beta / 2) plus the error of d derived above through the slope |L'| = min(|d| / beta, 1) -- the term is
                       not relatively well conditioned in d (it vanishes quadratically), so a plain count cannot bound it
        IoU family     max(4 r_v, 16) u (|term_i| + 1), r_v the worst ratio of the fp32 reference's values in units u (|term| + 1)
      sums[2] (the foreground count) is exact.
  mined set   count per image exactly min(ceil(min(ratio #pos, N - 1)), #negatives); nothing left out is harder than anything kept
      (fp64, margin 4 u hardness); among the negatives whose fp64 hardness
      EQUALS the smallest kept one (equal logits) the kept are the first in index order, the order mine_select_kernel documents;
      ignored anchors and unmined negatives have gradient exactly 0 (the mined set is read off the gradients: sigmoid(z) of the
      families used with mining never rounds to 0).

Preconditions (``preconditions``; conditions on the inputs, asserted from the oracle on the CPU for every case): exact coordinates
(above); every IoU-matching case has >= 8 foreground, 8 ignored and 8 negative anchors -- with N <= 6 anchors per image one foreground
and one negative, and in the single-anchor case (1, 3, 1, 1, 1, 1, 64), where both cannot exist, one foreground; in the 200- and 256-row
cases dropping the rows of any of [0, 64), [64, 128), [128, 192), [192, G) changes the assignment (a winner lies in each: staging over
four waves); every scale-matching case has foreground and background; the iou_radius cases have an anchor of depth 0 with a class
label; with B >= 2 the last image has no valid row; valid rows are interleaved with label = -1 rows.

Logit families: ``prior`` N(-4.6, 1) (the regime training runs in), ``centred`` N(0, 3), ``saturated`` (uniform over +-30, half of
the fp32 elements over +-60, with +-0.0, +-30, +-65504 and for fp32 +-60 planted), ``ties`` ({-2, -1, 0, 1}: mining thresholds fall
inside large tie groups).  Each is rounded to the dtype."""
import collections
import functools
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "ssds.pytorch_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from oracle import box_oracle as O  # noqa: E402

U = 2.0 ** -24
EPS = {"bf16": 2.0 ** -8, "f16": 2.0 ** -10, "f32": 2.0 * U}
TINY = {"bf16": 2.0 ** -126, "f16": 2.0 ** -24, "f32": 2.0 ** -126}
DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}
CODES = {"f32": 0, "bf16": 1, "f16": 2}  # include/ssdk.h SSDK_F32 | SSDK_BF16 | SSDK_F16
D_B, D_L, D_D = 7, 6, 3
ALPHA, BETA, SCALE = 0.25, 0.11, 0.37
LOC_KINDS = ("iou", "giou", "diou", "ciou")
RATIOS_ENV = "SSDK_LOSSJUDGE_RATIOS"

# (B, G, A, C, H, W, stride): the smallest shapes that reach each branch
GEOS = [
    (2, 9, 6, 7, 20, 24, 16),     # N = 2880: three chunks of mine_select_kernel, a ragged last workgroup
    (3, 200, 6, 5, 5, 7, 32),     # staging over four waves
    (2, 256, 6, 3, 3, 3, 64),     # G = SSDK_MAX_GT; N = 54 is less than one wave
    (2, 70, 6, 4, 1, 1, 128),     # the 1x1 level: N = 6, num_neg capped at 5
    (1, 3, 1, 1, 1, 1, 64),       # N = 1: N - 1 = 0, nothing is mined; C = 1
    (2, 12, 16, 3, 4, 4, 32),     # A = SSDK_MAX_ANCHORS; N = 256 is exactly one workgroup
    (2, 12, 6, 81, 2, 43, 16),    # C = 81; N = 516: the third workgroup has 4 live threads
    (130, 4, 3, 2, 10, 9, 16),    # 260 partial rows (520 with mining): loss_finalize_kernel loops
    # the contract edges of match_loss (EDGE_GEOS; in no case list): no row at all, one row more than SSDK_MAX_GT
    (2, 0, 3, 2, 2, 2, 32),
    (2, 257, 3, 2, 2, 2, 32),
]
# ratios x scales by A: integer scales keep every anchor corner at a multiple of 0.5
ANCHOR_SHAPES = {1: ([1], [2.0]), 3: ([1, 2, 0.5], [2.0]), 6: ([1, 2, 0.5], [2.0, 3.0]), 16: ([1, 2, 0.5, 3], [1.0, 2.0, 3.0, 4.0])}
# ground truth per geometry: seed, share of valid rows, share of rows drawn next to a grid anchor, largest jitter of those (in anchor
# sizes), share of the map's width they are drawn from (the rest stays background), the anchor shapes they are drawn from (all);
# ``last``: the last row is valid in every image that has ground truth
GEN = [
    dict(seed=11, valid=0.8, near=0.7, jit=0.35, span=0.7),
    dict(seed=12, valid=0.6, near=0.9, jit=0.40, span=0.6),
    dict(seed=13, valid=0.9, near=1.0, jit=0.30, span=0.34, shapes=[1, 4]),
    dict(seed=14, valid=0.8, near=1.0, jit=0.12, span=1.0, shapes=[1]),
    dict(seed=15, valid=0.7, near=1.0, jit=0.05, span=1.0),
    dict(seed=16, valid=0.8, near=0.8, jit=0.35, span=0.8),
    dict(seed=17, valid=0.8, near=0.8, jit=0.35, span=0.7),
    dict(seed=18, valid=0.75, near=0.8, jit=0.35, span=0.7),
    dict(seed=19, valid=1.0, near=1.0, jit=0.3, span=1.0),
    dict(seed=20, valid=0.5, near=1.0, jit=0.3, span=0.5, shapes=[0], last=True),
]
EDGE_GEOS = (8, 9)
IOU_MATCH = [0.5, 0.4]
SCALE_MATCH = [[0.55, 1.45], [0.55, 1.45]]  # (the boxes under [-1, 6] are all foreground)
RADIUS = {"iou": 0, "iou_radius": 0.5, "scale": 0, "scale_center": 1.5}

N_GEOS = 8  # the geometries of the case lists
Case = collections.namedtuple("Case", "geo mode dtype family cls gamma ratio loc_loss spread")


def _case(geo, mode="iou", dtype="bf16", family="prior", cls="focal", gamma=2.0, ratio=None, loc_loss="smoothl1", spread=0.3):
    return Case(geo, mode, dtype, family, cls, gamma, ratio, loc_loss, spread)


def _focal_cases():
    out = [_case(g) for g in range(N_GEOS)]
    for g in (0, 1):
        out += [_case(g, mode=m) for m in ("iou_radius", "scale", "scale_center")]
        out += [_case(g, gamma=v) for v in (1.5, 0.5)]
        out += [_case(g, dtype=d, loc_loss=k) for k in LOC_KINDS for d in ("bf16", "f16", "f32")]
        out += [_case(g, family=f) for f in ("centred", "saturated", "ties")]
        out += [_case(g, dtype=d) for d in ("f16", "f32")]
        out += [_case(g, dtype=d, family="saturated") for d in ("f16", "f32")]
    out += [_case(1, dtype="f32", loc_loss=k, spread=1.5) for k in LOC_KINDS]
    return out


def _multibox_cases():
    out = [_case(g, cls="multibox", ratio=r) for g in range(N_GEOS) for r in (3, 0.5, 1000)]
    out += [_case(g, cls="multibox", ratio=3, family="ties") for g in (0, 1, 2)]
    out += [_case(0, mode="iou_radius", cls="multibox", ratio=1000)]
    return out


FOCAL_CASES = _focal_cases()
MULTIBOX_CASES = _multibox_cases()
ALL_CASES = FOCAL_CASES + MULTIBOX_CASES
GUARD_GEOS = [1, 2, 3, 4, 5, 6]  # rows 2 to 7 of the table: the tail geometries, through the C-ABI entry points


def cid(c):
    s = "g%d-%s-%s-%s" % (c.geo, c.mode, c.dtype, c.family)
    s += "-mb%g" % c.ratio if c.cls == "multibox" else "-fl%g" % c.gamma
    return s + "-%s%s" % (c.loc_loss, "" if c.spread == 0.3 else "-wide")


def d_c(gamma):
    return 22 + (16 if gamma == 2.0 else int(math.ceil(10.5 * gamma + 2)))


def focal_value_count(gamma):
    return 1 + (16 if gamma == 2.0 else 10.5 * gamma + 2) + 8 + 2


# ---- operands ---------------------------------------------------------------------------------------------------------------------
def anchors_of(geo):
    B, G, A, C, H, W, stride = GEOS[geo]
    ratios, scales = ANCHOR_SHAPES[A]
    return collections.OrderedDict((s, O.generate_anchors(s, ratios, scales)) for s in (stride, 2 * stride))


def grid_anchors(geo):
    """-> [A, H, W, 4] fp32 corners in the kernel's anchor order, computed like box.py:151-159 (one fp32 add)"""
    B, G, A, C, H, W, stride = GEOS[geo]
    anc = anchors_of(geo)[stride].astype(np.float32)
    fx = (np.arange(W, dtype=np.float32) * np.float32(stride))[None, None, :, None]
    fy = (np.arange(H, dtype=np.float32) * np.float32(stride))[None, :, None, None]
    off = np.concatenate([fx + 0 * fy, fy + 0 * fx, fx + 0 * fy, fy + 0 * fx], -1)  # [1, H, W, 4]
    return (off + anc[:, None, None, :]).astype(np.float32)


@functools.lru_cache(maxsize=None)
def targets_of(geo):
    """-> [B, G, 5] fp32 (x, y, w, h, label), integer valued; label -1 = padding"""
    B, G, A, C, H, W, stride = GEOS[geo]
    p = GEN[geo]
    rs = np.random.RandomState(p["seed"])
    ga = grid_anchors(geo)
    t = np.full((B, G, 5), -1.0, np.float32)
    xs_allowed = max(1, int(math.ceil(W * p["span"])))
    for b in range(B):
        if B >= 2 and b == B - 1:
            continue  # an image without ground truth
        for g in range(G):
            if rs.rand() >= p["valid"] and not (g == G - 1 and (p.get("last") or not (t[b, :, 4] > -1).any())):
                continue
            if g == G - 1 and p.get("last"):  # the last row wins an anchor of its own: the far corner's, copied
                x1, y1, x2, y2 = [float(v) for v in ga[A - 1, H - 1, W - 1]]
                cx, cy, w, h = (x1 + x2) / 2, (y1 + y2) / 2, x2 - x1 + 1, y2 - y1 + 1
            elif rs.rand() < p["near"]:
                shapes = p.get("shapes") or list(range(A))
                a, iy, ix = shapes[rs.randint(len(shapes))], rs.randint(H), rs.randint(xs_allowed)
                x1, y1, x2, y2 = [float(v) for v in ga[a, iy, ix]]
                w, h = x2 - x1 + 1, y2 - y1 + 1
                j = rs.rand() * p["jit"]
                cx = (x1 + x2) / 2 + rs.uniform(-j, j) * w
                cy = (y1 + y2) / 2 + rs.uniform(-j, j) * h
                w, h = w * math.exp(rs.uniform(-j, j)), h * math.exp(rs.uniform(-j, j))
            else:
                w, h = rs.uniform(0.5, 6) * stride, rs.uniform(0.5, 6) * stride
                cx, cy = rs.uniform(0, W * stride), rs.uniform(0, H * stride)
            w, h = max(2.0, round(w)), max(2.0, round(h))
            t[b, g] = [round(cx - w / 2), round(cy - h / 2), w, h, rs.randint(C)]
    return t


Assign = collections.namedtuple("Assign", "depth lab onehot delta lt fg")


def _oracle(geo, mode, targets):
    B, G, A, C, H, W, stride = GEOS[geo]
    match = SCALE_MATCH if mode.startswith("scale") else IOU_MATCH
    return O.extract_targets(targets, anchors_of(geo), C, stride, (H, W), match, RADIUS[mode])


def _box2delta64(boxes, anchors):
    boxes, anchors = boxes.astype(np.float64), anchors.astype(np.float64)
    awh = anchors[:, 2:] - anchors[:, :2] + 1
    actr = anchors[:, :2] + 0.5 * awh
    bwh = boxes[:, 2:] - boxes[:, :2] + 1
    bctr = boxes[:, :2] + 0.5 * bwh
    return np.concatenate([(bctr - actr) / awh, np.log(bwh / awh)], 1)


def assign(geo, mode, targets):
    """the oracle's assignment of ``targets`` plus the fp64 deltas of every anchor's winning box"""
    B, G, A, C, H, W, stride = GEOS[geo]
    ct, lt, depth = _oracle(geo, mode, targets)
    ga = grid_anchors(geo).reshape(-1, 4)  # [N, 4]
    n = ga.shape[0]
    delta = np.zeros((B, n, 4), np.float64)
    for b in range(B):
        rows = targets[b][targets[b][:, 4] > -1]
        if rows.shape[0] == 0:
            continue
        boxes = np.concatenate([rows[:, :2], rows[:, :2] + rows[:, 2:4] - np.float32(1)], 1).astype(np.float32)
        want = lt[b].reshape(A, 4, H * W).transpose(0, 2, 1).reshape(n, 4)
        enc = O.box2delta(np.repeat(boxes, n, 0), np.tile(ga, (boxes.shape[0], 1))).reshape(boxes.shape[0], n, 4)
        same = (enc.view(np.int32) == want.view(np.int32)[None]).all(-1)  # [G', N]
        assert same.any(0).all(), "an anchor's box_target is the encoding of no valid row"
        delta[b] = _box2delta64(boxes[same.argmax(0)], ga)
    delta = delta.reshape(B, A, H * W, 4).transpose(0, 1, 3, 2).reshape(B, A, 4, H, W)
    onehot = torch.from_numpy(ct).double()
    has, lab = onehot.max(2)
    lab = torch.where(has > 0, lab, torch.full_like(lab, C))
    d = torch.from_numpy(depth)[:, :, 0]
    return Assign(d, lab, onehot, torch.from_numpy(delta), torch.from_numpy(lt), int((d > 0).sum()))


@functools.lru_cache(maxsize=None)
def assignment(geo, mode):
    return assign(geo, mode, targets_of(geo))


def _logits(family, dtype, shape, rs):
    n = int(np.prod(shape))
    if family == "prior":
        z = rs.standard_normal(n) - 4.6
    elif family == "centred":
        z = rs.standard_normal(n) * 3
    elif family == "ties":
        z = rs.randint(-2, 2, n).astype(np.float64)
    else:
        z = rs.uniform(-30, 30, n)
        plant = [0.0, -0.0, 30.0, -30.0, 65504.0, -65504.0]
        if dtype == "f32":
            z[n // 2:] = rs.uniform(-60, 60, n - n // 2)
            plant += [60.0, -60.0]
        k = min(len(plant), n)
        where = rs.permutation(n)[:k]
        z[where] = plant[:k]
    return torch.from_numpy(z.reshape(shape)).float().to(DTYPES[dtype])


Ops = collections.namedtuple("Ops", "targets anchors match radius conf loc asg")


@functools.lru_cache(maxsize=8)
def operands(case):
    B, G, A, C, H, W, stride = GEOS[case.geo]
    asg = assignment(case.geo, case.mode)
    rs = np.random.RandomState(1000 + 7 * case.geo + len(case.family) + int(10 * case.spread))
    conf = _logits(case.family, case.dtype, (B, A * C, H, W), rs)
    noise = torch.from_numpy(rs.standard_normal((B, A, 4, H, W)) * case.spread)
    loc = (asg.lt.double() + noise).float().to(DTYPES[case.dtype]).reshape(B, A * 4, H, W)
    match = SCALE_MATCH if case.mode.startswith("scale") else IOU_MATCH
    return Ops(targets_of(case.geo), anchors_of(case.geo), match, RADIUS[case.mode], conf, loc, asg)


def scale_of(asg):
    return SCALE / max(asg.fg, 1)


def preconditions(case):
    """conditions on the inputs, from the oracle alone"""
    B, G, A, C, H, W, stride = GEOS[case.geo]
    t, asg = targets_of(case.geo), assignment(case.geo, case.mode)
    n = A * H * W
    valid = t[:, :, 4] > -1
    assert np.array_equal(t, np.round(t)), "integer ground truth"
    anc = anchors_of(case.geo)[stride]
    assert np.array_equal(anc * 2, np.round(anc * 2)), "anchor corners at multiples of 0.5"
    if B >= 2:
        assert not valid[B - 1].any(), "one image has no valid row"
    if G >= 9:
        assert any(not valid[b, :int(np.nonzero(valid[b])[0].max())].all() for b in range(B) if valid[b].any()), "interleaved padding"
    fg, ign, neg = asg.fg, int((asg.depth < 0).sum()), int((asg.depth == 0).sum())
    if case.mode.startswith("scale"):
        assert fg >= 1 and neg >= 1, (fg, neg)
    elif B * n == 1:
        assert fg == 1
    elif n <= 6:
        assert fg >= 1 and neg >= 1, (fg, neg)
    else:
        assert fg >= 8 and ign >= 8 and neg >= 8, (fg, ign, neg)
    if case.mode == "iou_radius":
        assert int(((asg.depth == 0) & (asg.lab < C)).sum()) >= 1, "no negative carries a class label"
    if G >= 200:
        for lo in (0, 64, 128, 192):
            cut = t.copy()
            cut[:, lo:min(lo + 64, G), 4] = -1
            other = _oracle(case.geo, case.mode, cut)
            assert not np.array_equal(other[1], asg.lt.numpy()), "no winning row in [%d, %d)" % (lo, lo + 64)


def rows_of(geo):
    from ssds import _native as N

    B, G, A, C, H, W, stride = GEOS[geo]
    return int(N.lib.ssdk_match_loss_workspace_bytes(B, A, H, W)) // 12


# ---- truth ------------------------------------------------------------------------------------------------------------------------
def _sig_parts(z):
    e = torch.exp(-z.abs())
    inv = 1.0 / (1.0 + e)
    p = torch.where(z >= 0, inv, e * inv)
    q = torch.where(z >= 0, e * inv, inv)
    l1p = torch.log1p(e)
    return p, q, -(l1p + torch.relu(-z)), -(l1p + torch.relu(z)), l1p


def focal_terms(z, onehot, alpha, gamma):
    """closed forms of the kernel's comment block -> (loss, dloss/dz), any float dtype"""
    p, q, logp, logq, _ = _sig_parts(z)
    pos = onehot > 0
    u = torch.where(pos, q, p)
    v = torch.where(pos, p, q)
    lg = torch.where(pos, logp, logq)
    w = torch.where(pos, torch.full_like(z, alpha), torch.full_like(z, 1.0) - alpha)
    ug = u * u if gamma == 2.0 else torch.where(u > 0, torch.pow(u, gamma), torch.zeros_like(u))
    grad = w * ug * (gamma * v * lg - u)
    return -w * ug * lg, torch.where(pos, grad, -grad)


def bce_terms(z, onehot):
    p, _, _, _, l1p = _sig_parts(z)
    return torch.relu(z) - onehot * z + l1p, p - onehot


def smoothl1_terms(d, beta):
    x = d.abs()
    lin = x >= beta
    return torch.where(lin, x - 0.5 * beta, 0.5 * x * x / beta), torch.where(lin, torch.sign(d), d / beta)


def iou_terms(loc, delta, fgmask, kind):
    """criterion.IOULoss under autograd in the dtype of ``loc`` -> (values [B,A,1,H,W], gradient of their foreground sum)"""
    from ssds.core import criterion

    l = loc.clone().requires_grad_(True)
    val = criterion.IOULoss(kind)(l, delta)
    (val * fgmask).sum().backward()
    return val.detach(), l.grad * fgmask


def views(case, ops):
    B, G, A, C, H, W, stride = GEOS[case.geo]
    return ops.conf.view(B, A, C, H, W), ops.loc.view(B, A, 4, H, W)


def hardness(case, ops):
    """fp64 [B, N]: the largest per-class BCE term of every negative, 0 elsewhere"""
    conf, _ = views(case, ops)
    ce, _ = bce_terms(conf.double(), ops.asg.onehot)
    hard = ce.max(2)[0]
    return torch.where(ops.asg.depth == 0, hard, torch.zeros_like(hard)).reshape(hard.shape[0], -1)


def num_neg(case, ops):
    n = ops.asg.depth[0].numel()
    out = []
    for b in range(ops.asg.depth.shape[0]):
        pos, neg = int((ops.asg.depth[b] > 0).sum()), int((ops.asg.depth[b] == 0).sum())
        out.append(min(int(math.ceil(min(case.ratio * pos, n - 1))), neg))
    return out


Truth = collections.namedtuple("Truth", "d_conf d_loc cls_sum cls_mass cls_bound loc_sum loc_mass loc_bound iou")


def truth(case, ops, mined=None):
    """fp64 gradients (unscaled), sums, masses and the summed per-term error bounds; ``mined`` [B,A,H,W] bool for MultiBoxLoss"""
    asg = ops.asg
    conf, loc = views(case, ops)
    z, l = conf.double(), loc.double()
    fg = (asg.depth > 0).unsqueeze(2)
    if case.cls == "focal":
        care = (asg.depth >= 0).unsqueeze(2).double()
        loss, grad = focal_terms(z, asg.onehot, ALPHA, case.gamma)
        cls_bound = float((focal_value_count(case.gamma) * U * (1 + z.abs()) * loss.abs() * care).sum())
    else:
        care = ((asg.depth > 0) | mined).unsqueeze(2).double()
        loss, grad = bce_terms(z, asg.onehot)
        cls_bound = float((7 * U * loss.abs() * care).sum())
    d_conf, cls_sum, cls_mass = grad * care, float((loss * care).sum()), float((loss.abs() * care).sum())
    iou = None
    if case.loc_loss == "smoothl1":
        d = l - asg.delta
        lloss, lgrad = smoothl1_terms(d, BETA)
        size = l.abs() + asg.delta.abs() + 1
        slope = torch.clamp(d.abs() / BETA, max=1.0)
        loc_bound = float(((4 * U * lloss.abs() + slope * D_D * U * size) * fg).sum())
        d_loc = lgrad * fg
    else:
        val, d_loc = iou_terms(l, asg.delta, fg.double(), case.loc_loss)
        val32, g32 = iou_terms(loc.float(), asg.lt, fg.float(), case.loc_loss)
        S = d_loc.abs().amax(2, keepdim=True)
        unit = U * (d_loc.abs() + S)
        err = (g32.double() - d_loc).abs()
        rr = torch.where(err == 0, torch.zeros_like(err), err / unit.clamp(min=1e-300)) * fg
        left = (rr > 32).any(2, keepdim=True) & fg
        keep = fg & ~left
        rv = ((val32.double() - val).abs() / (U * (val.abs() + 1)) * fg)
        iou = dict(unit=unit, keep=keep, left=int(left.sum()), ref=float((rr * keep).max()) if bool(keep.any()) else 0.0,
                   ref_value=float(rv.max()), ref_sum=float((val32 * fg.float()).sum()))
        lloss = val
        loc_bound = float((max(4 * iou["ref_value"], 16.0) * U * (val.abs() + 1) * fg).sum())
    loc_sum, loc_mass = float((lloss * fg).sum()), float((lloss.abs() * fg).sum())
    return Truth(d_conf, d_loc, cls_sum, cls_mass, cls_bound, loc_sum, loc_mass, loc_bound, iou)


def check_left_out(case, ops):
    """the 1 % cap on the anchors the fp32 reference cannot judge: from the reference alone"""
    if case.loc_loss == "smoothl1" or case.spread != 0.3:
        return
    t = truth(case, ops, mined=torch.zeros_like(ops.asg.depth, dtype=torch.bool))
    assert t.iou["left"] <= 0.01 * ops.asg.fg, "%s: the reference leaves out %d of %d foreground anchors" % (
        cid(case), t.iou["left"], ops.asg.fg)


# ---- the judge --------------------------------------------------------------------------------------------------------------------
Out = collections.namedtuple("Out", "gc gl cls_sum loc_sum fg")  # scaled gradients in the case's dtype, the three sums as floats
RECORDS = []


def _worst(case, what, err, bar, problems):
    live = bar > 0
    RECORDS.append(dict(case=cid(case), dtype=case.dtype, quantity=what,
                        worst_err_over_bar=round(float((err[live] / bar[live]).max()), 4) if bool(live.any()) else 0.0))
    bad = err > bar
    if bool(bad.any()):
        over = torch.where(bad, err / bar.clamp(min=1e-300), torch.zeros_like(err))
        i = int(over.argmax())
        problems.append("%s: %d elements outside the bar, worst at flat index %d: err %.3g, bar %.3g" % (
            what, int(bad.sum()), i, float(err.reshape(-1)[i]), float(bar.reshape(-1)[i])))


def mined_of(case, ops, out, problems):
    """the mined set the output used (negatives that received a gradient), checked by its defining properties"""
    B, G, A, C, H, W, stride = GEOS[case.geo]
    got_any = (out.gc.view(B, A, C, H, W) != 0).any(2)
    if bool((got_any & (ops.asg.depth < 0)).any()):
        problems.append("an ignored anchor received a gradient")
    mined = got_any & (ops.asg.depth == 0)
    hard = hardness(case, ops)
    for b, want in enumerate(num_neg(case, ops)):
        m, negs = mined[b].reshape(-1), (ops.asg.depth[b] == 0).reshape(-1)
        if int(m.sum()) != want:
            problems.append("image %d: %d negatives mined, %d wanted" % (b, int(m.sum()), want))
            continue
        if not 0 < want < int(negs.sum()):
            continue
        kept, left = hard[b][m], hard[b][negs & ~m]
        thr = float(kept.min())
        if float(left.max()) > thr + 4 * U * float(left.max()):
            problems.append("image %d: a negative of hardness %.9g was left out, one of %.9g kept" % (b, float(left.max()), thr))
        tied = torch.nonzero(negs & (hard[b] == thr)).reshape(-1)
        k = int(m[tied].sum())
        if not bool(m[tied[:k]].all()):
            problems.append("image %d: the ties at the threshold are not kept in index order" % b)
    return mined


def judge(case, ops, out):
    """-> the list of problems of ``out`` (empty: it passes every bar)"""
    B, G, A, C, H, W, stride = GEOS[case.geo]
    asg, problems = ops.asg, []
    eps, tiny, s = EPS[case.dtype], TINY[case.dtype], scale_of(ops.asg)
    check_left_out(case, ops)
    if out.gc.dtype != DTYPES[case.dtype] or out.gl.dtype != DTYPES[case.dtype]:
        problems.append("gradient dtypes %s, %s" % (out.gc.dtype, out.gl.dtype))
    if float(out.fg) != float(asg.fg):
        problems.append("foreground count %r, the oracle's assignment has %d" % (float(out.fg), asg.fg))
    mined = mined_of(case, ops, out, problems) if case.cls == "multibox" else None
    t = truth(case, ops, mined)
    conf, loc = views(case, ops)
    z = conf.double()

    want = s * t.d_conf
    err = (out.gc.view(B, A, C, H, W).double() - want).abs()
    if case.cls == "focal":
        bar = 2 * eps * want.abs() + tiny + d_c(case.gamma) * U * (1 + z.abs()) * want.abs()
    else:
        bar = 2 * eps * want.abs() + tiny + D_B * U * s * torch.maximum(torch.sigmoid(z), t.d_conf.abs())
    bar = torch.where(want == 0, torch.zeros_like(bar), bar)  # ignored anchors, unmined negatives: exactly 0
    _worst(case, "d_conf", err, bar, problems)

    wantl = s * t.d_loc
    got = out.gl.view(B, A, 4, H, W).double()
    errl = (got - wantl).abs()
    fg = (asg.depth > 0).unsqueeze(2).expand_as(errl)
    if bool((got[~fg] != 0).any()):
        problems.append("d_loc: an anchor that is no foreground received a gradient")
    if case.loc_loss == "smoothl1":
        barl = 2 * eps * wantl.abs() + tiny + s * D_L * U * (loc.double().abs() + asg.delta.abs() + 1) / BETA
        _worst(case, "d_loc", errl * fg, barl, problems)
    else:
        keep = t.iou["keep"].expand_as(errl)
        ratio = torch.clamp(errl - 2 * eps * wantl.abs() - tiny, min=0) / (s * t.iou["unit"]).clamp(min=1e-300) * keep
        allow = max(4 * t.iou["ref"], 16.0)
        worst = float(ratio.max())
        RECORDS.append(dict(case=cid(case), dtype=case.dtype, quantity="d_loc", foreground=asg.fg, left_out=t.iou["left"],
                            reference_ratio=round(t.iou["ref"], 3), kernel_ratio=round(worst, 3), bar=round(allow, 3)))
        if worst > allow:
            problems.append("d_loc (%s): %.3g units, the fp32 reference %.3g, allowed %.3g" % (case.loc_loss, worst, t.iou["ref"], allow))

    rows = rows_of(case.geo) * (2 if case.cls == "multibox" else 1)
    for what, got_sum, want_sum, mass, bound in (("cls_sum", out.cls_sum, t.cls_sum, t.cls_mass, t.cls_bound),
                                                 ("loc_sum", out.loc_sum, t.loc_sum, t.loc_mass, t.loc_bound)):
        d_term = int(math.ceil(bound / (U * mass))) if mass > 0 else 0
        bar_sum = (d_term + (rows + 255) // 256 + 20) * U * mass
        e = abs(float(got_sum) - want_sum)
        if case.loc_loss != "smoothl1" and what == "loc_sum":
            RECORDS.append(dict(case=cid(case), dtype=case.dtype, quantity="loc_sum", foreground=asg.fg, left_out=t.iou["left"],
                                reference_ratio=round(abs(t.iou["ref_sum"] - want_sum) / (U * mass), 3) if mass > 0 else 0.0,
                                kernel_ratio=round(e / (U * mass), 3) if mass > 0 else 0.0,
                                bar=d_term + (rows + 255) // 256 + 20))
        else:
            RECORDS.append(dict(case=cid(case), dtype=case.dtype, quantity=what, worst_err_over_bar=round(e / bar_sum, 4) if bar_sum > 0 else 0.0))
        if not e <= bar_sum:
            problems.append("%s: %.9g, truth %.9g: err %.3g, bar %.3g (D_term %d, rows %d)" % (what, float(got_sum), want_sum, e, bar_sum,
                                                                                             d_term, rows))
    return problems


def flush_records():
    path = os.environ.get(RATIOS_ENV)
    if path and RECORDS:
        with open(path, "a") as f:
            for r in RECORDS:
                f.write(json.dumps(r, sort_keys=True) + "\n")
    del RECORDS[:]


# ---- the fp32 CPU model and its mutations -------------------------------------------------------------------------------------------
MUTATIONS = {  # name -> the case it must fail on (``prior`` logits except where ties are the point)
    "zero_small": _case(0),
    "alpha_swap": _case(0),
    "gamma2": _case(0, gamma=1.5),
    "drop_rows64": _case(1),
    "num_neg_off": _case(0, cls="multibox", ratio=3),
    "zero_target_neg": _case(0, mode="iou_radius", cls="multibox", ratio=1000),
    "ties_desc": _case(0, cls="multibox", ratio=3, family="ties"),
    "dloc_sign": _case(0),
    "cls_fg_only": _case(0),
    "ignored_grad": _case(0),
}


def model(case, ops, mutate=None):
    """the documented closed forms in torch fp32 on the CPU, stored to the dtype, scaled like _MatchLoss.backward -> Out"""
    B, G, A, C, H, W, stride = GEOS[case.geo]
    dt = DTYPES[case.dtype]
    asg = ops.asg
    if mutate == "drop_rows64":
        cut = ops.targets.copy()
        cut[:, 64:, 4] = -1
        asg = assign(case.geo, case.mode, cut)
    conf, loc = views(case, ops)
    z, l = conf.float(), loc.float()
    onehot = asg.onehot.float()
    fgm = (asg.depth > 0).unsqueeze(2)
    if case.cls == "focal":
        gamma = 2.0 if mutate == "gamma2" else case.gamma
        loss, grad = focal_terms(z, onehot, ALPHA, gamma)
        if mutate == "alpha_swap":
            wrong = focal_terms(z, onehot, 1.0 - ALPHA, gamma)[1]
            grad = torch.where(onehot > 0, grad, wrong)
        care = ((asg.depth > 0) if mutate == "cls_fg_only" else (asg.depth >= 0)).unsqueeze(2)
        cls_sum = float((loss * care).sum())
        d_conf = grad * (asg.depth >= 0).unsqueeze(2)
    else:
        loss, grad = bce_terms(z, onehot)
        hard = loss.max(2)[0]
        hard = torch.where(asg.depth == 0, hard, torch.zeros_like(hard)).reshape(B, -1)
        mined = torch.zeros_like(hard, dtype=torch.bool)
        n = hard.shape[1]
        for b in range(B):
            pos, neg = int((asg.depth[b] > 0).sum()), int((asg.depth[b] == 0).sum())
            k = min(int(math.ceil(min(case.ratio * pos, n - 1))), neg)
            if mutate == "num_neg_off":
                k = min(k + 1, neg)
            h = hard[b].flip(0) if mutate == "ties_desc" else hard[b]
            order = torch.sort(h, descending=True, stable=True)[1][:k]  # equal keys: the first in index order
            mined[b, (n - 1 - order) if mutate == "ties_desc" else order] = True
        mined = mined.view_as(asg.depth)
        if mutate == "zero_target_neg":
            zl, zg = bce_terms(z, torch.zeros_like(onehot))
            neg = (asg.depth == 0).unsqueeze(2)
            loss, grad = torch.where(neg, zl, loss), torch.where(neg, zg, grad)
        care = ((asg.depth > 0) | mined).unsqueeze(2)
        cls_sum = float((loss * care).sum())
        d_conf = grad * care
    if case.loc_loss == "smoothl1":
        lloss, lgrad = smoothl1_terms(l - asg.lt, np.float32(BETA).item())
        d_loc = lgrad * fgm
    else:
        lloss, d_loc = iou_terms(l, asg.lt, fgm.float(), case.loc_loss)
    loc_sum = float((lloss * fgm).sum())
    s = torch.tensor(scale_of(asg), dtype=torch.float32)
    gc, gl = d_conf.to(dt) * s, d_loc.to(dt) * s  # (the 0-dim fp32 scale keeps the dtype: fp32 arithmetic, one more store)
    if mutate == "zero_small":
        want = scale_of(asg) * truth(case, ops).d_conf
        gc = torch.where(want.abs() < 1e-5, torch.zeros_like(gc), gc)
    if mutate == "dloc_sign":
        flat = gl.reshape(-1)
        i = int(torch.nonzero(flat.float().abs() > 0.5 * float(flat.float().abs().max()))[0])
        flat[i] = -flat[i]
    if mutate == "ignored_grad":
        b, a, y, x = [int(v) for v in torch.nonzero(asg.depth < 0)[0]]
        gc[b, a, 0, y, x] = 2.0 ** -20
    return Out(gc.reshape(B, A * C, H, W), gl.reshape(B, A * 4, H, W), cls_sum, loc_sum, float(asg.fg))


def torch_focal_fp32(case, ops):
    """criterion.FocalLoss in fp32 under autograd (the truth of tests/test_gpu_train.py) in the model's place: d_conf only"""
    from ssds.core import criterion

    B, G, A, C, H, W, stride = GEOS[case.geo]
    good = model(case, ops)
    c = views(case, ops)[0].float().clone().requires_grad_(True)
    onehot = ops.asg.onehot.float()
    care = (ops.asg.depth >= 0).unsqueeze(2).float()
    (care * criterion.FocalLoss(ALPHA, case.gamma)(c, onehot)).sum().backward()
    gc = c.grad.to(DTYPES[case.dtype]) * torch.tensor(scale_of(ops.asg), dtype=torch.float32)
    return good._replace(gc=gc.reshape(B, A * C, H, W))
