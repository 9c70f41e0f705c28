"""Shared by tests/test_dense_train_cpu.py and tests/test_gpu_dense_train.py: the operands and fp64 truths of the dense-block training
kernels (csrc/ssdk_densetrain.hip), and the judges.

EXACT operands.  The operand transform op(x) = round_dtype(max(fmaf(a, x, b), 0)) and the ReLU mask fmaf(a, x, b) > 0 are compared
against a CPU model, so the pre-activation must not depend on how it is evaluated:
    x = k / 16        integer |k| <= 127                     (8 significant bits: exact in bf16 and fp16)
    a = j / 8         integer 1 <= |j| <= 40
    b = l / 8         l = -j r0 with r0 = k0 / 16 an integer in [-7, 7]
so a x + b = j (k - k0) / 128 with |j (k - k0)| < 2^14: exact in fp32 with or without a fused multiply-add, in any order, and op(x)
is reproduced on the CPU bit for bit (fp32 value -> one rounding to the dtype; values up to 75 need that rounding in both
dtypes).  6 % of the elements of a channel are set to k0: their pre-activation is exactly 0, which the strict > 0 must mask.
``exact_case`` asserts that between 1 % and 20 % of the pre-activations are exactly zero."""
import functools

import torch

import dwjudge as DJ
import shufflejudge as SJ

U, EPS, DTYPES = DJ.U, DJ.EPS, DJ.DTYPES
DTYPE_NAMES = ("bf16", "f16")
# (B, Ctot, K, M, H, W)
CASES = [
    (2, 96, 64, 128, 7, 9),      # pixel tail, short K
    (3, 160, 128, 128, 13, 13),  # odd plane, long K
    (2, 104, 72, 128, 5, 5),     # K tail
    (1, 288, 256, 128, 16, 8),   # exactly one 128-pixel group
    (2, 64, 64, 24, 6, 6),       # contiguous, M tail
]


def cid(case):
    return "x".join(str(v) for v in case)


@functools.lru_cache(maxsize=None)
def exact_case(case, name):
    """Operands (CPU) and fp64 truths of one case in one dtype, computed once and never modified."""
    b, ctot, k, m, h, w = case
    dt = DTYPES[name]
    hw = h * w
    g = torch.Generator().manual_seed(977 * ctot + 31 * k + 7 * h + w + (0 if name == "bf16" else 3))
    ri = lambda lo, hi, shape: torch.randint(lo, hi + 1, shape, generator=g)  # noqa: E731
    j = ri(1, 40, (k,)) * (2 * ri(0, 1, (k,)) - 1)
    r0 = ri(-7, 7, (k,))
    kk = ri(-127, 127, (b, ctot, h, w))
    planted = torch.rand((b, k, h, w), generator=g) < 0.06
    kk[:, :k] = torch.where(planted, (16 * r0).view(1, k, 1, 1).expand(b, k, h, w), kk[:, :k])
    F = (kk.float() / 16).to(dt)
    assert torch.equal(F.float() * 16, kk.float())
    a, bb = j.float() / 8, (-j * r0).float() / 8
    coef = torch.zeros(k, 4)
    coef[:, 0], coef[:, 1] = a, bb
    coef[:, 2:] = float("nan")  # (what the kernels must not read)
    coef[:, 2] = 0.0
    x = F[:, :k].float()
    pre = a.view(1, k, 1, 1) * x + bb.view(1, k, 1, 1)  # exact (see above)
    assert torch.equal(pre.double(), a.double().view(1, k, 1, 1) * x.double() + bb.double().view(1, k, 1, 1))
    zero_share = float((pre == 0).float().mean())
    assert 0.01 <= zero_share <= 0.20, zero_share
    op = pre.clamp(min=0).to(dt)  # the CPU model of op(x), bit for bit
    mask = pre > 0
    wt = SJ.weights(m, k, dt, 13 * k + m)
    dm = SJ.tensor((b, m, h, w), dt, 17 * k + m)
    s = SJ.tensor((b, k, h, w), dt, 19 * k + m)
    gold = SJ.tensor((b, ctot, h, w), dt, 23 * k + m)
    mean = torch.randn(k, generator=g)
    invstd = torch.rand(k, generator=g) + 0.5
    gamma = torch.randn(k, generator=g)
    op64, w64 = op.double(), wt.double().view(m, k)
    y = torch.einsum("mk,bkp->bmp", w64, op64.view(b, k, hw)).view(b, m, h, w)
    my = torch.einsum("mk,bkp->bmp", w64.abs(), op64.abs().view(b, k, hw)).view(b, m, h, w)
    dw = torch.einsum("bmp,bkp->mk", dm.double().view(b, m, hw), op64.view(b, k, hw))
    mw = torch.einsum("bmp,bkp->mk", dm.double().abs().view(b, m, hw), op64.abs().view(b, k, hw))
    dims = (0, 2, 3)
    gm = s.double() * mask.double()
    xh = (x.double() - mean.double().view(1, k, 1, 1)) * invstd.double().view(1, k, 1, 1)
    red = torch.stack([gm.sum(dims), (gm * xh).sum(dims)], 1)
    red32 = red.float()  # what ssdk_dense_train_bn1_apply is handed
    n = b * hw
    dx = (gamma.double() * invstd.double()).view(1, k, 1, 1) * (gm - red32[:, 0].double().view(1, k, 1, 1) / n
                                                                - xh * red32[:, 1].double().view(1, k, 1, 1) / n)
    return dict(F=F, coef=coef, op=op, zero_share=zero_share, w=wt, dm=dm, s=s, gold=gold, mean=mean, invstd=invstd, gamma=gamma,
                y=y, sums=torch.stack([y.sum(dims), y.pow(2).sum(dims)], 1), S_abs=y.abs().sum(dims), S_sq=y.pow(2).sum(dims),
                S_My=my.sum(dims), S_yMy=(y.abs() * my).sum(dims), dw=dw, Mw=mw, red=red, red32=red32,
                R_g=gm.abs().sum(dims), R_gx=(gm * xh).abs().sum(dims), gnew=gold[:, :k].double() + dx)


def judge16(what, got, want, name):
    """The per-element bar of tests/dwjudge.py for a 16-bit result: |err| <= eps |want| + 4 eps rms(want)."""
    err = (got.double().cpu() - want).abs()
    bar = EPS[name] * want.abs() + 4 * EPS[name] * float(want.pow(2).mean().sqrt())
    print("%s: worst |err| / bar = %.3f" % (what, float((err / bar).max())))
    assert bool((err <= bar).all()), (what, int((~(err <= bar)).sum()))


def judge_abs(what, got, want, bar):
    err = (got.double().cpu() - want).abs()
    print("%s: worst |err| / bar = %.3f" % (what, float((err / bar.clamp(min=1e-300)).max())))
    assert bool((err <= bar).all()), (what, int((~(err <= bar)).sum()))


def bits(t):
    return t.contiguous().view(torch.int16)
