"""The judge of the inference convolutions behind ``ssdk_conv`` (csrc/ssdk_conv.hip, ssdk_conv3x3.hip, ssdk_conv3x3s.hip, ssdk_gemmp.hip,
ssdk_pwflow.hip, ssdk_smallmap.hip): operands, the fp64 truth with its absolute-value mass, the bars, the case tables with the template
instance every row must reach, an fp32 CPU model of the layer with its mutations, and the checks tests/test_gpu_convjudge.py runs.
tests/test_convjudge_cpu.py turns the judge on the model and on the mutations.  Plain torch, importable on the CPU.  Not a conftest.

Scope.  What ``ssdk_conv`` runs with groups == 1 and no dilation, plus the stem and the depthwise layer of the same entry point:
conv_gemm_kernel (five tile shapes, n64, resv, split-K), conv_wave_kernel (split and unsplit), conv_gemm256_kernel, conv_gemmp_kernel,
pwflow_kernel, conv3x3_halo_kernel (persistent form, first form, the form that takes a split planned for the GEMM), conv3x3_short_kernel,
conv_smallmap_kernel (single launches, stride 1 and 2, fragment image and KRSC), conv_first_kernel, dwconv3x3_kernel.  Everything goes
through ``fused_conv.conv_native`` with a ``ConvPack``, as tests/test_gpu_conv.py does.
Out of scope: the grouped and dilated kernels, the transposed convolution, xpair and the fused blocks (mbk / mbflow / mbsplit / mbconv: they
keep fp16 internals in units of six and need a judge of their own); the grouped small-map launch (tests/test_gpu_conv.py pins it bit for bit
to the single launches judged here); SSDK_HALO_SPLITK (off by default and read once per process).

Numerical model (csrc/ssdk_conv_common.h epilogue4, add_residual8 / add_residual1, f32_to_bits16; the library is built with
-ffp-contract=off).  Products of two 16-bit values are exact in fp32; the accumulator, and the fp32 slabs of a split, add them in some order;
v = acc * scale + bias in fp32; the activation in fp32; ONE round-to-nearest-even store to 16 bits; with a residual one further step,
rn16(post(rn16(v) + res)).  (The stem multiplies fp32 weights, BN scale folded in, by fused multiply-adds from the bias: one rounding per
product as well.)

Truth and mass.  The layer in fp64 on the CPU on the rounded operands and on the pack's OWN tensors (``pack.w``, fp32 ``pack.scale`` /
``pack.bias``: what the kernel reads).  The same contraction on absolute values gives the mass M = |scale| sum|x||w| + |bias|.

Random family.  x ~ N(0, 1), w ~ N(0, 1) / sqrt(K), both rounded to the dtype; BatchNorm statistics as in tests/test_gpu_conv.py, or a conv bias.

Bars (u = 2^-24; r16 = 2^-8 bf16, 2^-11 fp16: the unit roundoff of the 16-bit store).  No other tolerance exists here.
  e32 = (T + 2 + splits) u M L + A(v)
        T = the real products of one output, k^2 Cin (9 for the depthwise layer): each is added once, every addition rounds at most once
        (relative u of a partial sum whose magnitude the mass bounds), in any order; + 2 for the scale and the bias, + splits for the
        additions of the slabs.  L = the activation's Lipschitz constant, which carries the error of v through it: 1 for none / relu /
        relu6; 1/4 for sigmoid (s' = s (1 - s) <= 1/4); SILU_L = 1.1 for silu: f(v) = v s(v), f' = s (1 + v (1 - s)), whose maximum, where
        f'' = s (1 - s) (2 + v (1 - 2 s)) = 0, is 1.09984 at v = 2.3994.
        A(v) = the activation's own fp32 error, zero for the clamps.  Sigmoid is ``rcp(1 + exp2(c v))`` with c = -1.442695041f and exp2 /
        rcp good to 1 ulp = 2 u relative (the header comment of epilogue4).  c (itself rounded) times v rounds once: the argument t is off by
        <= 2 u |t|, and 2^t by the factor 2^(2 u |t|) = e^(2 u |v|): relative 2 u |v|; exp2 adds 2 u; so E = 2^t carries (2 |v| + 2) u.  The
        sum 1 + E carries that times E / (1 + E) <= 1, plus u for its own rounding; rcp adds 2 u: the sigmoid is off by <= (2 |v| + 5) u
        relative.  silu multiplies by v and rounds once more: (2 |v| + 6) u.  A(v) = (6 + 2 |v|) u |want| for both -- a few u (1 + |v|) |want|.
  no residual     |err| <= e32 + r16 (|want| + e32)                    (+ 2^-25 in fp16: half a spacing of its subnormals)
  residual        |err| <= e1 + (r16 + u) (|want| + e1), e1 = the bar above on the PRE-ADD value, want = the fp64 value of
                  post(rn16(v64) + res) (same / half / post).  u: the fp32 add of two 16-bit values rounds once.
If rn16 of the true pre-add value sits within e32 of a rounding boundary, the first store may legitimately land on the other side.  e1
bounds the distance of the stored pre-add value from the UNROUNDED true one, whichever side it fell, so the bar is sound against
post(pre64 + res); against the want above, which rounds pre64 first, it is not: the two stores are one 16-bit spacing apart, up to
2 r16 |pre|, and e1 holds r16 |pre| of it.  Against that want the fp32 model of this file (exactly the arithmetic above) leaves the bar on
the rows with a residual at K <= 256: by up to 1.78 (pw_ks4_three, fp16, K = 96; pw_half 1.70, gemmp_half 1.68, pw_ks2_nf8 bf16 1.60), on
about one element in 50 000 in fp16 and one in 500 000 to a million in bf16; at K >= 320 e32 is large enough that no element leaves.
``residual_error`` therefore takes such an element's error against the nearer of the wants that the two legitimate stores give,
rn16(pre64 -+ e32).  Nothing else is relaxed: the bar and every other element's want are as stated.
These bars are loose at long K by construction (T roundings are allowed).  That is why the exact family exists, not a reason for a factor.
``log_ratios`` writes the worst |err| / bar per case, dtype and family (profiles/r31_convjudge_ratios.jsonl is such a run).

Exact family.  Operands whose every partial sum, in ANY order, is representable: x, w in {-1, 0, 1} at a density that keeps the mean mass near
EXACT_MASS ({-2 .. 2} and dense where K <= 16 terms); scale = +-2^j, j in {-1, 0, 1} -- fold_bn's gamma / sqrt(var + eps) does not produce
those by luck, so ``exact_operands`` OVERWRITES pack.scale (and pack.bias) and ``exact_conditions`` asserts the tensor holds exactly them; the
stem folds its scale into fp32 weights and a dense layer without BatchNorm has no scale tensor: scale 1 there; integer biases and residuals;
activations none / relu / relu6 (a sigmoid-type case runs its exact family with "none").  ``exact_conditions`` computes from the operands,
it does not measure: every stored value, the pre-add one included, has mass <= 256 and IS representable in the output type; every fp32 sum
has mass < 2^24; at least a quarter of the truth is non-zero; every output channel, row and column has a non-zero truth element.  The check
is torch.equal on y (and on y2 of a split head); no tolerance.
Variants: ``ternary``; ``ones`` (x = 1, w = 1 on a thin subset of the input channels that differs per output channel: y is the count of
in-image taps times the subset size, so every border pixel's tap count shows); ``onehot_x`` (ONE input element per image = ONE_HOT, dense small-integer
weights: y[b, :, oy, ox] is one scaled column of w for each tap that reaches it and the bias everywhere else; spots: the four corners,
the last column, the last image, channels Cin - 1, 31, 32 and the last channel of the last 64-wide slab -- one spot per image, several
runs where the images are fewer than the spots); ``onehot_w`` (ONE weight = ONE_HOT
in every output channel, at a tap and an input channel that change with the channel, dense small-integer x: y[:, co] is a shifted copy of
one input channel -- every pixel's address arithmetic shows, at every stride and layout)."""
import collections
import functools
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "ssds.pytorch_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import torch  # noqa: E402
import torch.nn as nn  # noqa: E402
import torch.nn.functional as F  # noqa: E402

U = 2.0 ** -24
R16 = {"bf16": 2.0 ** -8, "f16": 2.0 ** -11}
DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16}
CODES = {"bf16": 1, "f16": 2}  # include/ssdk.h SSDK_BF16 | SSDK_F16
DTYPE_NAMES = ["bf16", "f16"]
SILU_L = 1.1
ONE_HOT = -1.3125
EXACT_MASS = 16.0
VARIANTS = ("ternary", "ones", "onehot_x", "onehot_w")
FAMILIES = ("random",) + VARIANTS
CLAMPS = ("none", "relu", "relu6")
RES_MODE = {None: 0, "same": 0, "half": 1, "post": 2}

GEMM, WAVE, G256, GEMMP, PWFLOW = "conv_gemm_kernel", "conv_wave_kernel", "conv_gemm256_kernel", "conv_gemmp_kernel", "pwflow_kernel"
HALO, SHORT, SMALLMAP, FIRST, DW = ("conv3x3_halo_kernel", "conv3x3_short_kernel", "conv_smallmap_kernel", "conv_first_kernel",
                                    "dwconv3x3_kernel")

Case = collections.namedtuple("Case", "name kernel variant n cin cout k stride h w act rmode nchw split act2 wfrag bn kind in_nchw splits")


def _c(name, kernel, variant, n, cin, cout, k, stride, h, w, act="none", rmode=None, nchw=False, split=None, act2=None, wfrag=True,
       bn=True, kind="dense", in_nchw=False, splits=1):
    """``variant``: the part of ssdk_last_variant() before " | " the row must reach (include/ssdk_variant.h); ``splits``: the slabs the
    row runs with on 256 CUs (the device test reads the real number back from the variant; the CPU model sums this many)."""
    return Case(name, kernel, variant, n, cin, cout, k, stride, h, w, act, rmode, nchw, split, act2, wfrag, bn, kind, in_nchw, splits)


# The smallest shapes that reach each instance; the gates are read from the launchers and assume 256 CUs.  If the variant assertion
# refuses a shape, the shape changes, not the assertion.  Every row's comment names the branch it is for.
CASES = [
    # ---- conv_gemm_kernel (launch_gemm): M > 256, else conv_wave; 3x3 / stride 1 stays off the halo kernel with Cout < 96 or Cin < 32
    _c("gemm_bn128", GEMM, "gemm bn=128 n64=0 resv=0 unsplit", 5, 24, 144, 1, 1, 9, 7, "relu6"),     # Cout > 64: SSDK_GEMM(2, 2, 4, 4); K tail 24
    _c("gemm_bn64", GEMM, "gemm bn=64 n64=0 resv=0 unsplit", 5, 24, 40, 1, 1, 9, 7, "none"),          # Cout > 32: (4, 1, 2, 4); channel tail 40
    _c("gemm_bn32", GEMM, "gemm bn=32 n64=0 resv=0 unsplit", 5, 24, 24, 1, 1, 9, 7, "relu"),          # Cout > 16: (4, 1, 2, 2)
    _c("gemm_bn16", GEMM, "gemm bn=16 n64=0 resv=0 unsplit", 5, 24, 16, 1, 1, 9, 7, "silu"),          # else: (4, 1, 2, 1)
    _c("gemm_n64", GEMM, "gemm bn=64 n64=1 resv=0 unsplit", 3, 320, 256, 1, 1, 10, 10, "relu"),       # n64: Cout % 64 == 0, KT = 10 <= 12
    _c("gemm_resv", GEMM, "gemm bn=128 n64=0 resv=1 unsplit", 2, 64, 136, 1, 1, 16, 20, "none", "same", bn=False),  # resv: residual, NHWC, Cout % 8 == 0 (136: not n64)
    _c("gemm_resv_post", GEMM, "gemm bn=64 n64=1 resv=1 unsplit", 2, 64, 256, 1, 1, 16, 20, "relu", "post"),       # 64 -> 256 is n64 (KT = 2): resv with the activation after the add
    _c("gemm_split_res", GEMM, "gemm bn=128 n64=0 resv=0 split", 2, 64, 192, 3, 1, 14, 14, "none", "same", splits=2),  # 3x3, < 96 halo tiles: a split with a residual
    _c("gemm_split_1x1", GEMM, "gemm bn=128 n64=0 resv=0 split", 3, 512, 256, 1, 1, 12, 12, "relu", splits=2),     # plan_splits: KT = 16, tiles = 8
    _c("gemm_split_3x3", GEMM, "gemm bn=128 n64=0 resv=0 split", 2, 96, 504, 3, 1, 19, 19, "none", nchw=True, split=24, act2="sigmoid",
       bn=False, wfrag=False, splits=3),                                                               # SSD head L0 at batch 2: KT = 27, three splits
    _c("gemm_resv_bn64", GEMM, "gemm bn=64 n64=0 resv=1 unsplit", 2, 64, 64, 1, 1, 16, 20, "relu6", "same"),       # resv on the 64-wide tile
    _c("gemm_resv_n64", GEMM, "gemm bn=64 n64=1 resv=1 unsplit", 3, 320, 256, 1, 1, 10, 10, "none", "half", bn=False),  # resv on the n64 form
    _c("gemm_split_bn64", GEMM, "gemm bn=64 n64=0 resv=0 split", 3, 512, 64, 1, 1, 12, 12, "relu", "post", splits=2),    # split-K on each narrower tile
    _c("gemm_split_bn32", GEMM, "gemm bn=32 n64=0 resv=0 split", 3, 512, 24, 1, 1, 12, 12, "relu", splits=2),
    _c("gemm_split_bn16", GEMM, "gemm bn=16 n64=0 resv=0 split", 3, 512, 16, 1, 1, 12, 12, "sigmoid", nchw=True, splits=2),
    _c("gemm_ctail", GEMM, "gemm bn=128 n64=0 resv=0 unsplit", 3, 40, 132, 1, 2, 21, 17, "sigmoid"),  # channel tail 132 = 128 + 4; stride 2, odd map
    # ---- conv_wave_kernel (wave_plan): M <= 256 and M Cout K <= 3e8
    _c("wave_split", WAVE, "wave split", 8, 64, 64, 3, 1, 2, 2, "relu6", splits=4),                   # KT = 18: s = min(768 / tiles, KT / 4)
    _c("wave_unsplit", WAVE, "wave unsplit", 2, 24, 40, 1, 1, 3, 5, "silu"),                          # KT = 1 < 4: unsplit
    _c("wave_half", WAVE, "wave unsplit", 8, 64, 64, 1, 1, 2, 2, "none", "half", bn=False),           # the half-resolution residual (KT = 2)
    _c("wave_post", WAVE, "wave split", 8, 64, 64, 3, 1, 2, 2, "relu6", "post", splits=4),            # act after the add
    # ---- conv_gemm256_kernel (use_gemm256): Cout >= 192, >= 128 tiles of 256 x 256, KT >= 32, not gemmp's layer
    _c("g256_s2", G256, "gemm256", 16, 128, 320, 3, 2, 64, 64, "relu6"),                               # 3x3 stride 2: KT = 36, 64 x 2 tiles
    _c("g256_ragged", G256, "gemm256", 16, 1064, 200, 1, 1, 45, 50, "silu"),                           # ragged M, K and channels
    _c("g256_c194", G256, "gemm256", 32, 1024, 194, 1, 1, 32, 32, "none", bn=False),                   # Cout % 4 != 0 keeps gemmp off
    # ---- conv_gemmp_kernel (launch_conv_gemmp): Cin >= 256, Cout >= 128 and % 4 == 0, 96 <= tiles, tiles <= CUs or fill >= 0.7
    _c("gemmp_even", GEMMP, "gemmp even", 24, 256, 128, 1, 1, 32, 32, "relu"),                        # 96 m-tiles x 1: grid = tiles, tr = 0
    _c("gemmp_rem", GEMMP, "gemmp remainder", 30, 256, 384, 1, 1, 32, 32, "none", "same"),            # 120 x 3 = 360 tiles: tq = 1, tr = 104
    _c("gemmp_s2", GEMMP, "gemmp even", 16, 256, 256, 1, 2, 63, 65, "relu6", "post"),                 # stride 2 on an odd map (32 x 33)
    _c("gemmp_half", GEMMP, "gemmp even", 8, 256, 256, 1, 1, 48, 56, "none", "half", bn=False),       # FPN lateral + x2 top-down add
    _c("gemmp_ktail", GEMMP, "gemmp even", 4, 264, 128, 1, 1, 100, 64, "silu"),                       # K tail of 8
    # ---- pwflow_kernel (launch_conv_pwflow): Cin % 32 == 0 and <= 128, Cout % 64 == 0, M >= 16384
    _c("pw_ks2_half", PWFLOW, "pwflow ks=2 nf=4", 4, 32, 64, 1, 1, 64, 64, "relu"),                   # Cin 32: KS 2 half used; Cout 64: nf 4
    _c("pw_ks2_nf8", PWFLOW, "pwflow ks=2 nf=8", 4, 64, 128, 1, 1, 64, 64, "relu6", "same"),          # nf 8: Cout % 256 != 0
    _c("pw_ks4_three", PWFLOW, "pwflow ks=4 nf=16", 1, 96, 256, 1, 1, 37, 443, "none", "post"),       # KS 4 three used; M = 16384 + 7: a ragged last group
    _c("pw_ks4_slices", PWFLOW, "pwflow ks=4 nf=8", 4, 128, 384, 1, 1, 64, 64, "silu"),               # 384: nf 8, three slices
    _c("pw_ks4_nf4", PWFLOW, "pwflow ks=4 nf=4", 4, 96, 64, 1, 1, 64, 64, "relu6"),                   # the last ks x nf pair
    _c("pw_s2", PWFLOW, "pwflow ks=2 nf=16", 4, 64, 256, 1, 2, 127, 129, "relu"),                     # stride 2 from an odd map (64 x 65)
    _c("pw_half", PWFLOW, "pwflow ks=2 nf=16", 4, 64, 256, 1, 1, 64, 64, "none", "half", bn=False),   # half-resolution residual
    # ---- conv3x3_halo_kernel (launch_conv3x3_halo): Cin >= 32; Cout >= 96, or >= 32 with Cin >= 128; >= 96 tiles
    _c("halo_slab", HALO, "halo persistent nhwc unsplit", 96, 40, 128, 3, 1, 16, 16, "relu"),           # one partial slab, one whole map per tile
    _c("halo_nchw_first", HALO, "halo first nchw unsplit vec_nchw=0", 16, 64, 720, 3, 1, 19, 19, "relu", nchw=True),  # ragged patches, scalar stores: Wo % 4 != 0
    _c("halo_nhwc_first", HALO, "halo first nhwc unsplit", 32, 64, 134, 3, 1, 19, 19, "none"),      # NHWC first form: Cout % 4 != 0
    _c("halo_four_maps", HALO, "halo persistent nhwc unsplit", 96, 384, 504, 3, 1, 8, 8, "none"),       # four maps per tile
    _c("halo_box_head", HALO, "halo persistent nchw unsplit", 16, 256, 36, 3, 1, 40, 40, "none", nchw=True, bn=False),  # narrow box head: 7 patches of 6x40 per map; 200 GEMM tiles, so no split is planned
    _c("halo_gemm_split", HALO, "halo first nhwc split", 32, 256, 256, 3, 1, 10, 10, "relu", splits=2),  # the GEMM's split carried over
    _c("halo_split_nchw", HALO, "halo first nchw split vec_nchw=0", 32, 256, 256, 3, 1, 10, 10, "none", nchw=True, bn=False, splits=2),
    _c("halo_split_vec", HALO, "halo first nchw split vec_nchw=1", 16, 256, 504, 3, 1, 16, 16, "sigmoid", nchw=True, wfrag=False, splits=2),  # 16-byte NCHW stores
    _c("halo_heads", HALO, "halo persistent nchw unsplit", 8, 96, 504, 3, 1, 32, 32, "none", nchw=True, split=24, act2="sigmoid",
       bn=False, wfrag=False),                                                                         # loc | conf with y2 (no fragment image: not the short kernel)
    _c("halo_res", HALO, "halo persistent nhwc unsplit", 48, 256, 256, 3, 1, 16, 16, "none", "same"),   # plain residual
    _c("halo_post", HALO, "halo persistent nhwc unsplit", 48, 128, 256, 3, 1, 16, 16, "relu", "post"),  # act after the add
    # ---- conv3x3_short_kernel (launch_conv3x3_short): fragment image; Cin % 32 == 0 and <= 128, or 256 on <= 2500 pixels; Cout >= 96;
    #      tpw >= 2; patches nsplit >= 256 (Cin <= 128) or >= 128 (Cin = 256)
    _c("short_cs1_nchw", SHORT, "short cs=1 nchw", 52, 32, 132, 3, 1, 20, 20, "none", nchw=True),     # Wo % 8 == 4: NCHW, not wide; ragged second channel tile
    _c("short_cs2", SHORT, "short cs=2 nhwc", 32, 64, 160, 3, 1, 24, 48, "relu6"),                    # NHWC with relu6, non-square map
    _c("short_cs3_heads", SHORT, "short cs=3 nchw-wide", 16, 96, 504, 3, 1, 32, 32, "none", nchw=True, split=24, act2="sigmoid", bn=False),  # split head
    _c("short_cs4", SHORT, "short cs=4 nhwc", 20, 128, 256, 3, 1, 40, 40, "relu"),                    # ragged patches (40 = 2.5 x 16)
    _c("short_cs8", SHORT, "short cs=8 nhwc", 9, 256, 256, 3, 1, 40, 40, "relu"),                    # Cin = 256: one workgroup per CU
    # ---- conv_smallmap_kernel (launch_conv_smallmap): Cin in {128, 256, 512}, <= 64 output pixels
    _c("sm_p1_packed", SMALLMAP, "smallmap mfr=4 taps=1 packed=1 na=1 stride=1 kw=1", 64, 128, 504, 3, 1, 1, 1, "silu"),   # P = 1: the centre tap only
    _c("sm_p1_krsc", SMALLMAP, "smallmap mfr=4 taps=1 packed=0 na=1 stride=1 kw=1", 9, 256, 40, 3, 1, 1, 1, "none", wfrag=False, bn=False),
    _c("sm_3x5", SMALLMAP, "smallmap mfr=4 taps=9 packed=1 na=1 stride=1 kw=1", 9, 128, 504, 3, 1, 3, 5, "none", nchw=True, split=24,
       act2="sigmoid", bn=False),                                                                      # 15 pixels: four maps per group, ragged last group
    _c("sm_4x4_krsc", SMALLMAP, "smallmap mfr=4 taps=9 packed=0 na=1 stride=1 kw=1", 6, 256, 100, 3, 1, 4, 4, "relu", wfrag=False),  # partial channel range
    _c("sm_2x2", SMALLMAP, "smallmap mfr=4 taps=9 packed=1 na=1 stride=1 kw=1", 35, 256, 40, 3, 1, 2, 2, "relu6"),         # sixteen maps per group, Cout = 40
    _c("sm_big_na2", SMALLMAP, "smallmap mfr=4 taps=9 packed=1 na=2 stride=1 kw=2", 64, 512, 504, 3, 1, 8, 8, "none", nchw=True),  # big: 32 x 8 >= 256
    _c("sm_big_krsc", SMALLMAP, "smallmap mfr=8 taps=9 packed=0 na=1 stride=1 kw=1", 64, 512, 504, 3, 1, 8, 8, "relu", wfrag=False),  # mfr 8
    _c("sm_s2_8x8", SMALLMAP, "smallmap mfr=4 taps=9 packed=1 na=2 stride=2 kw=1", 5, 256, 512, 3, 2, 16, 16, "relu"),     # stride 2 onto 8x8
    _c("sm_s2_4x4", SMALLMAP, "smallmap mfr=4 taps=9 packed=1 na=2 stride=2 kw=1", 33, 128, 256, 3, 2, 8, 8, "relu6"),     # onto 4x4, ragged last group
    _c("sm_s2_2x2", SMALLMAP, "smallmap mfr=4 taps=9 packed=1 na=2 stride=2 kw=1", 70, 128, 100, 3, 2, 4, 4, "silu"),      # onto 2x2, partial channels
    # ---- conv_first_kernel: Cout 16 / 32 / 64, NCHW and NHWC input
    _c("first_16_nchw", FIRST, "first cout=16 nchw", 2, 3, 16, 3, 2, 33, 30, "relu6", kind="stem", in_nchw=True),         # stride 2 on an odd map
    _c("first_32_nhwc", FIRST, "first cout=32 nhwc", 2, 3, 32, 3, 2, 33, 30, "relu", kind="stem"),
    _c("first_64_nchw", FIRST, "first cout=64 nchw", 2, 3, 64, 3, 1, 9, 11, "relu6", kind="stem", in_nchw=True, bn=False),
    _c("first_16_nhwc", FIRST, "first cout=16 nhwc", 1, 3, 16, 3, 1, 5, 7, "none", kind="stem", bn=False),
    _c("first_32_nchw", FIRST, "first cout=32 nchw", 1, 3, 32, 3, 2, 8, 6, "relu6", kind="stem", in_nchw=True),
    _c("first_64_nhwc", FIRST, "first cout=64 nhwc", 3, 3, 64, 3, 2, 7, 5, "relu", kind="stem"),
    # ---- dwconv3x3_kernel: C = 8 and 960, stride 1 and 2, odd maps
    _c("dw_8_s1", DW, "dw stride=1", 2, 8, 8, 3, 1, 7, 9, "relu6", kind="dw"),
    _c("dw_960_s2", DW, "dw stride=2", 2, 960, 960, 3, 2, 11, 13, "relu6", kind="dw"),
    _c("dw_8_s2", DW, "dw stride=2", 3, 8, 8, 3, 2, 10, 5, "none", kind="dw"),
    _c("dw_960_s1", DW, "dw stride=1", 1, 960, 960, 3, 1, 5, 6, "relu", kind="dw"),
]
BY_NAME = collections.OrderedDict((c.name, c) for c in CASES)
assert len(BY_NAME) == len(CASES)
SPLIT_CASES = [c.name for c in CASES if c.splits > 1]
# the rows the MUTATION sweep of tests/test_convjudge_cpu.py runs on (ten mutations x five families x two dtypes per row: the cap keeps
# that sweep to seconds); the unmutated model runs on every row of the table
CPU_MACS = 0.2e9


def out_hw(c):
    pad = c.k // 2
    return (c.h + 2 * pad - c.k) // c.stride + 1, (c.w + 2 * pad - c.k) // c.stride + 1


def terms(c):
    """T: the real products of one output"""
    return 9 if c.kind == "dw" else c.k * c.k * c.cin


def macs(c):
    ho, wo = out_hw(c)
    return c.n * ho * wo * c.cout * terms(c)


def cpu_cases():
    return [c for c in CASES if macs(c) <= CPU_MACS]


def exact_act(a):
    return a if a in CLAMPS else "none"


# ---- operands ------------------------------------------------------------------------------------------------------------------------
def _gen(c, dtype_name, salt):
    return torch.Generator().manual_seed(1000003 * salt + 7919 * CASES.index(BY_NAME[c.name]) + CODES[dtype_name])


def _module(c, w, bias):
    groups = c.cin if c.kind == "dw" else 1
    conv = nn.Conv2d(c.cin, c.cout, c.k, c.stride, c.k // 2, groups=groups, bias=bias is not None)
    with torch.no_grad():
        conv.weight.copy_(w)
        if bias is not None:
            conv.bias.copy_(bias)
    return conv


def _pack(c, conv, bn, act, dtype_name):
    from ssds.modeling.layers import fused_conv as FC

    pack = FC.ConvPack(conv, bn, act, DTYPES[dtype_name])
    assert pack.kind == c.kind, (pack.kind, c.kind)
    return pack


def _res_shape(c):
    ho, wo = out_hw(c)
    return (c.n, c.cout, ho // 2, wo // 2) if c.rmode == "half" else (c.n, c.cout, ho, wo)


Ops = collections.namedtuple("Ops", "x pack res act act2 hint w")  # w: the weights as generated, [Cout, Cin / groups, k, k]


def operands(c, dtype_name):
    """the random family -> Ops(x 16-bit NCHW, the ConvPack on the CPU, residual or None, act, act2)"""
    dtype, gen = DTYPES[dtype_name], _gen(c, dtype_name, 1)
    x = torch.randn(c.n, c.cin, c.h, c.w, generator=gen).to(dtype)
    wshape = (c.cout, 1 if c.kind == "dw" else c.cin, c.k, c.k)
    w = (torch.randn(wshape, generator=gen) / terms(c) ** 0.5).to(dtype).float()
    if c.bn:
        bn = nn.BatchNorm2d(c.cout)
        bn.running_mean.copy_(torch.randn(c.cout, generator=gen) * 0.2)
        bn.running_var.copy_(torch.rand(c.cout, generator=gen) + 0.5)
        with torch.no_grad():
            bn.weight.copy_(torch.rand(c.cout, generator=gen) + 0.5)
            bn.bias.copy_(torch.randn(c.cout, generator=gen) * 0.2)
        conv = _module(c, w, None)
    else:
        bn, conv = None, _module(c, w, torch.randn(c.cout, generator=gen) * 0.5)
    res = torch.randn(_res_shape(c), generator=gen).to(dtype) if c.rmode else None
    return Ops(x, _pack(c, conv, bn, c.act, dtype_name), res, c.act, c.act2 if c.act2 is not None else c.act, None, w)


def _ints(gen, shape, density, amp):
    val = torch.randint(1, amp + 1, shape, generator=gen).float() * (torch.randint(0, 2, shape, generator=gen).float() * 2 - 1)
    return val if density >= 1.0 else val * (torch.rand(shape, generator=gen) < density).float()


def onehot_x_spots(c):
    """(channel, row, column) of the ONE_HOT input elements: the four corners and the last column, on channels Cin - 1, 31, 32 and the
    last channel of the last FULL 64-wide slab, 64 floor(Cin / 64) - 1 (where the layer has them; Cin - 1 again where Cin is a multiple
    of 64, another channel at Cin = 96, 264, 320, 1064)"""
    chans = sorted({c.cin - 1, min(31, c.cin - 1), min(32, c.cin - 1), max(0, 64 * (c.cin // 64) - 1) if c.cin >= 64 else c.cin - 1})
    where = [(0, 0), (0, c.w - 1), (c.h - 1, 0), (c.h - 1, c.w - 1), (c.h // 2, c.w - 1)]
    spots = [(chans[i % len(chans)], iy, ix) for i, (iy, ix) in enumerate(where)]
    spots += [(ch, c.h - 1, c.w - 1) for ch in chans if all(s[0] != ch for s in spots)]
    return sorted(set(spots), key=spots.index)


def onehot_x_positions(c):
    """the runs of the onehot_x variant: a list of (image, channel, row, column) per run.  ONE hot element per image, so that every output
    element still sees at most one product; spot i of a run sits in image N - 1 - i (the first in the LAST image), and a layer with fewer
    images than spots takes several runs"""
    spots = onehot_x_spots(c)
    return [[(c.n - 1 - i, ) + s for i, s in enumerate(spots[r:r + c.n])] for r in range(0, len(spots), c.n)]


def exact_scale(c, gen):
    """+-2^j, j in {-1, 0, 1}, per output channel -- where the layer has a scale tensor; else ones (the stem folds the scale into its fp32
    weights, a dense layer without BatchNorm passes no scale)"""
    if not c.bn or c.kind == "stem":
        return torch.ones(c.cout)
    return 2.0 ** torch.randint(-1, 2, (c.cout,), generator=gen).float() * (torch.randint(0, 2, (c.cout,), generator=gen).float() * 2 - 1)


def exact_operands(c, dtype_name, variant, position=0):
    """-> Ops of the exact family (``position``: which of onehot_x_positions)"""
    dtype, gen = DTYPES[dtype_name], _gen(c, dtype_name, 2)
    t = terms(c)
    amp = 2 if t <= 16 else 1
    dens = 1.0 if t <= 16 else min(1.0, (EXACT_MASS / t) ** 0.5)
    wshape = (c.cout, 1 if c.kind == "dw" else c.cin, c.k, c.k)
    xshape = (c.n, c.cin, c.h, c.w)
    x = _ints(gen, xshape, dens, amp) if variant == "ternary" else None  # (the other variants draw only what they keep)
    w = _ints(gen, wshape, dens, amp) if variant == "ternary" else None
    act, act2 = exact_act(c.act), exact_act(c.act2 if c.act2 is not None else c.act)
    if variant == "ones":  # (a clamp at 6 would hide the tap counts)
        act = act2 = "none"
    clamped = act != "none" or act2 != "none"
    # a clamp at zero would hide a channel whose bias is negative from the one-hot variants: positive biases there
    bias = torch.randint(1, 3, (c.cout,), generator=gen).float()
    if not clamped:
        bias = bias * (torch.randint(0, 2, (c.cout,), generator=gen).float() * 2 - 1)
    scale = exact_scale(c, gen)
    if variant == "ones":  # positive scale and bias: a count times the scale must not cancel against the bias
        x, scale, bias = torch.ones(xshape), scale.abs(), bias.abs()
        if c.kind == "dw":
            w = torch.ones(wshape)
        else:  # 1 .. 4 input channels per output channel, another subset for each
            w = torch.zeros(wshape)
            for co in range(c.cout):
                for j in range(1 + co % 4):
                    w[co, (7 * co + 13 * j) % c.cin] = 1.0
    elif variant == "onehot_x":
        x = torch.zeros(xshape)
        for spot in onehot_x_positions(c)[position]:
            x[spot] = ONE_HOT
        w = _ints(gen, wshape, 1.0, 2)
    elif variant == "onehot_w":
        x = _ints(gen, xshape, 1.0, 2)
        w = torch.zeros(wshape)
        for co in range(c.cout):
            ci = 0 if c.kind == "dw" else (c.cin - 1 - 5 * co) % c.cin
            w[co, ci, (co // 3) % c.k, co % c.k] = ONE_HOT
    res = None
    if c.rmode:
        res = torch.randint(-2, 3, _res_shape(c), generator=gen).float().to(dtype)
    conv = _module(c, w, None if (c.bn and c.kind != "stem") else bias)
    bn = nn.BatchNorm2d(c.cout) if (c.bn and c.kind != "stem") else None
    pack = _pack(c, conv, bn, act, dtype_name)
    if pack.scale is not None:  # OVERWRITTEN: fold_bn's gamma / sqrt(var + eps) is never exactly a power of two
        pack.scale = scale.clone()
        pack.bias = bias.clone()
    return Ops(x.to(dtype), pack, res, act, act2, None if variant == "ternary" else variant, w)


# ---- truth ----------------------------------------------------------------------------------------------------------------------------
def pack_weight(c, pack):
    """the pack's own weight tensor as [Cout, Cin / groups, k, k] fp64"""
    w = pack.w.detach().cpu().double()
    if c.kind == "dw":  # [3][3][C]
        return w.permute(2, 0, 1).unsqueeze(1).contiguous()
    return w.permute(0, 3, 1, 2).contiguous()  # KRSC


def pack_scale_bias(c, pack):
    scale = pack.scale.detach().cpu().double() if pack.scale is not None else torch.ones(pack.cout, dtype=torch.float64)
    return scale, pack.bias.detach().cpu().double()


def conv64(c, x, w, hint=None):
    """the contraction in fp64.  Plain: im2col + matmul in chunks of images (torch's fp64 conv2d is a slow path on the CPU).  ``hint``
    names the structure of an exact variant's operands, which makes the same sums cheap (tests/test_convjudge_cpu.py compares every
    short cut with the plain contraction): ``onehot_x`` -- one image is not zero; ``ones`` -- x is 1 everywhere, so the input channels
    can be added up first; ``onehot_w`` -- one weight per output channel, so y[:, co] is a one-tap filter of one input channel."""
    pad = c.k // 2
    if c.kind == "dw":
        return F.conv2d(x, w, None, c.stride, pad, 1, c.cin)
    ho, wo = out_hw(c)
    if hint == "onehot_x":
        hot = x.flatten(1).abs().sum(1).nonzero().flatten()
        out = torch.zeros(c.n, w.shape[0], ho, wo, dtype=x.dtype)
        out[hot] = conv64(c, x[hot], w)
        return out
    if hint == "ones":
        y1 = F.conv2d(torch.ones(1, 1, c.h, c.w, dtype=x.dtype), w.sum(1, keepdim=True), None, c.stride, pad)
        return y1.expand(c.n, -1, -1, -1).contiguous()
    if hint == "onehot_w":
        idx = w.abs().flatten(1).argmax(1)
        rows = torch.arange(w.shape[0])
        ci, tap = idx // (c.k * c.k), idx % (c.k * c.k)
        wd = torch.zeros(w.shape[0], 1, c.k, c.k, dtype=w.dtype)
        wd[rows, 0, tap // c.k, tap % c.k] = w[rows, ci, tap // c.k, tap % c.k]
        return F.conv2d(x[:, ci], wd, None, c.stride, pad, 1, w.shape[0])
    w2 = w.reshape(w.shape[0], -1)
    step = max(1, int(2.0e7 // max(1, w2.shape[1] * ho * wo)))
    outs = []
    for b in range(0, x.shape[0], step):
        xb = x[b:b + step]
        if c.k == 1:
            col = xb[:, :, ::c.stride, ::c.stride].reshape(xb.shape[0], c.cin, ho * wo)
        else:
            col = F.unfold(xb, c.k, 1, pad, c.stride)
        outs.append(torch.matmul(w2, col).view(xb.shape[0], -1, ho, wo))
    return torch.cat(outs)


def act64(v, act):
    if act == "relu":
        return v.clamp(min=0)
    if act == "relu6":
        return v.clamp(0, 6)
    if act == "silu":
        return v * torch.sigmoid(v)
    if act == "sigmoid":
        return torch.sigmoid(v)
    return v


def _per_channel(c, ops, fn):
    """fn(act) -> tensor [N, Cout, Ho, Wo]; channels from ``split`` on take act2"""
    if c.split is None or ops.act2 == ops.act:
        return fn(ops.act)
    a, b = fn(ops.act), fn(ops.act2)
    return torch.cat([a[:, :c.split], b[:, c.split:]], 1)


def upsample2(res):
    return res.repeat_interleave(2, 2).repeat_interleave(2, 3)


def _truth(c, ops, dtype_name):
    dtype = DTYPES[dtype_name]
    w = pack_weight(c, ops.pack)
    scale, bias = pack_scale_bias(c, ops.pack)
    x = ops.x.double()
    sc, bi = scale.view(1, -1, 1, 1), bias.view(1, -1, 1, 1)
    v = conv64(c, x, w, ops.hint) * sc + bi
    mass = conv64(c, x.abs(), w.abs(), ops.hint) * sc.abs() + bi.abs()
    tr = {"v": v, "M": mass, "ops": ops}
    post = c.rmode == "post"
    pre = v if post else _per_channel(c, ops, lambda a: act64(v, a))  # (post: the staged value is linear)
    tr["pre"] = pre
    if c.rmode:
        res = ops.res.double()
        res = upsample2(res) if c.rmode == "half" else res
        s = pre.to(dtype).double() + res
        tr["res"] = res
        tr["y"] = act64(s, ops.act) if post else s
    else:
        tr["y"] = pre
    return tr


@functools.lru_cache(maxsize=2)
def truth(name, dtype_name, family="random", position=0):
    """fp64 truth of one case and family with its mass.  Cached: compute once, share, leave unchanged."""
    c = BY_NAME[name]
    ops = operands(c, dtype_name) if family == "random" else exact_operands(c, dtype_name, family, position)
    return _truth(c, ops, dtype_name)


def wrong_truth(tr, c):
    """the wrong-truth check: ONE product -- the centre tap of the input channel where it is largest -- taken out of the truth at the last
    pixel of the last image, channel 0.  The change is on the truth, not on the device.  -> (a copy of ``tr``, the product); for a case
    without residual whose channel 0 is linear"""
    ops = tr["ops"]
    assert c.rmode is None and c.kind == "dense" and ops.act == "none"
    w = pack_weight(c, ops.pack)
    scale, _ = pack_scale_bias(c, ops.pack)
    ho, wo = out_hw(c)
    iy, ix = (ho - 1) * c.stride, (wo - 1) * c.stride
    prods = ops.x[c.n - 1, :, iy, ix].double() * w[0, :, c.k // 2, c.k // 2] * scale[0]
    prod = float(prods[int(prods.abs().argmax())])
    bad = dict(tr)
    v = tr["v"].clone()
    v[c.n - 1, 0, ho - 1, wo - 1] -= prod
    bad["v"] = v
    bad["pre"] = bad["y"] = _per_channel(c, ops, lambda a: act64(v, a))
    return bad, prod


def exact_conditions(c, tr, dtype_name):
    """the operand conditions of the exact family -> list of the violated ones (empty: every partial sum on every path is exact)"""
    dtype, bad, ops = DTYPES[dtype_name], [], tr["ops"]
    if ops.pack.scale is not None:
        s = ops.pack.scale.detach().cpu().abs()
        if not bool(((s == 0.5) | (s == 1.0) | (s == 2.0)).all()):
            bad.append("pack.scale holds values outside +-2^{-1, 0, 1}")
    if not torch.equal(ops.pack.bias.detach().cpu(), ops.pack.bias.detach().cpu().round()):
        bad.append("pack.bias is not integer")
    if ops.act not in CLAMPS or ops.act2 not in CLAMPS:
        bad.append("a sigmoid-type activation in the exact family")
    top = float(tr["M"].max())
    if top > 256:
        bad.append("stored value: mass %.6g > 256" % top)
    if top >= 2 ** 24:
        bad.append("fp32 sum: mass %.6g >= 2^24" % top)
    if c.rmode:
        top = float((tr["pre"].abs() + tr["res"].abs()).max())
        if top > 256:
            bad.append("sum with the residual: mass %.6g > 256" % top)
    for k in ("pre", "y"):
        if not torch.equal(tr[k].to(dtype).double(), tr[k]):
            bad.append("%s: the truth is not representable in %s" % (k, dtype_name))
    nz = tr["y"] != 0
    if float(nz.double().mean()) < 0.25:
        bad.append("only %.3f of the truth is non-zero" % float(nz.double().mean()))
    for name, dims in (("channel", (0, 2, 3)), ("row", (0, 1, 3)), ("column", (0, 1, 2))):
        if not bool(nz.sum(dims).gt(0).all()):
            bad.append("an output %s without a non-zero truth element" % name)
    return bad


# ---- the bars ------------------------------------------------------------------------------------------------------------------------
def lipschitz(act):
    return {"sigmoid": 0.25, "silu": SILU_L}.get(act, 1.0)


def act_error(v, want, act):
    """A(v): the fp32 error of the activation itself (module docstring)"""
    if act in ("sigmoid", "silu"):
        return (6.0 + 2.0 * v.abs()) * U * want.abs()
    return torch.zeros_like(v)


def bar(c, tr, dtype_name, splits):
    """-> (the bar per element of y, e32 of the pre-add value) (module docstring)"""
    ops, r16 = tr["ops"], R16[dtype_name]
    depth = (terms(c) + 2 + splits) * U
    sub = 2.0 ** -25 if dtype_name == "f16" else 0.0
    pre_act = "none" if c.rmode == "post" else None

    def e32(a):
        a = pre_act or a
        return depth * tr["M"] * lipschitz(a) + act_error(tr["v"], act64(tr["v"], a), a)

    e = _per_channel(c, ops, e32)
    e1 = e + r16 * (tr["pre"].abs() + e) + sub
    if not c.rmode:
        return e1, e
    return e1 + (r16 + U) * (tr["y"].abs() + e1) + sub, e


def residual_error(c, got, tr, dtype_name, e32):
    """|got - want| of a layer with a residual, want = post(rn16(pre64) + res).  Where pre64 sits within e32 of a rounding boundary the
    first store may legitimately land on the other side: there the error is taken against the nearer of the wants the two legitimate
    stores give, rn16(pre64 - e32) and rn16(pre64 + e32) (everywhere else all three are one value)."""
    dtype, ops = DTYPES[dtype_name], tr["ops"]
    err = (got - tr["y"]).abs()
    for shift in (-1.0, 1.0):
        s = (tr["pre"] + shift * e32).to(dtype).double() + tr["res"]
        err = torch.minimum(err, (got - (act64(s, ops.act) if c.rmode == "post" else s)).abs())
    return err


def new_rec(what):
    return {"what": what, "ratios": {}, "lines": [], "failures": [], "kernel": None, "variant": None, "worst": None}


def _say(rec, what, err, bar_):
    ratio = err / bar_.clamp(min=1e-300)
    worst = float(ratio.max()) if err.numel() else 0.0
    at = int(ratio.argmax()) if err.numel() else 0
    rec["ratios"][what] = worst
    rec["worst"] = [int(i) for i in torch.unravel_index(torch.tensor(at), err.shape)] if err.numel() else None
    rec["lines"].append("%s %s: worst |err| / bar = %.3f at %s" % (what, rec["what"], worst, rec["worst"]))
    bad = int((~(err <= bar_)).sum())  # (a NaN is outside every bar)
    if bad:
        rec["failures"].append("%s: %d elements outside the bar, worst %.3g of it at %s" % (what, bad, worst, rec["worst"]))


def joined(y):
    """conv_native's answer (a tensor, or the (y, y2) of a split head) -> one [N, Cout, Ho, Wo] tensor on the CPU"""
    if isinstance(y, (tuple, list)):
        return torch.cat([t.detach().cpu() for t in y], 1)
    return y.detach().cpu()


def judge(rec, c, got, tr, dtype_name, splits):
    """the random family: ``got`` [N, Cout, Ho, Wo] in the dtype against the bars"""
    if got.dtype != DTYPES[dtype_name] or tuple(got.shape) != tuple(tr["y"].shape):
        rec["failures"].append("y: dtype %s shape %s" % (got.dtype, tuple(got.shape)))
        return rec
    bar_, e32 = bar(c, tr, dtype_name, splits)
    err = residual_error(c, got.double(), tr, dtype_name, e32) if c.rmode else (got.double() - tr["y"]).abs()
    _say(rec, "y", err, bar_)
    return rec


def judge_exact(rec, got, tr, dtype_name):
    """the exact family: bit equality with the fp64 truth cast to the output type"""
    want = tr["y"].to(DTYPES[dtype_name])
    if got.dtype != want.dtype or tuple(got.shape) != tuple(want.shape):
        rec["failures"].append("y: dtype %s shape %s" % (got.dtype, tuple(got.shape)))
    elif not torch.equal(got, want):
        diff = got != want
        at = [int(i) for i in torch.unravel_index(diff.flatten().int().argmax(), diff.shape)]
        rec["failures"].append("y: not equal (%d elements differ, the first at %s: got %s want %s)" % (
            int(diff.sum()), at, float(got[tuple(at)]), float(want[tuple(at)])))
    rec["ratios"]["y"] = 0.0 if not rec["failures"] else float("inf")
    return rec


# ---- an fp32 CPU model of the layer: partial sums per tap and 32-channel chunk, added in index order, the slabs of a split summed
# ---- separately and added in order; the epilogue of the numerical model ------------------------------------------------------------------
MUTATIONS = ("drop_product", "skip_last_chunk", "slab_twice", "round_partials", "bias_before_scale", "no_post", "half_index",
             "swap_split", "ragged_copy", "relu6_no_upper")


def applies(mut, c):
    """whether the mutation changes anything the case runs"""
    ho, wo = out_hw(c)
    return {"slab_twice": c.splits > 1, "no_post": c.rmode == "post" and c.act != "none", "half_index": c.rmode == "half" and ho > 2,
            "swap_split": c.split is not None, "relu6_no_upper": "relu6" in (c.act, c.act2), "skip_last_chunk": c.kind == "dense",
            "ragged_copy": wo > 1, "bias_before_scale": c.bn and c.kind != "stem"}.get(mut, True)  # (no scale tensor: nothing to swap)


def exact_applies(mut, c):
    """... in the exact family: partial sums of mass <= 256 ARE 16-bit values, so rounding them changes nothing there -- by construction
    the exact family cannot see ``round_partials``; a relu6 case keeps its clamp, a sigmoid-type case runs with "none" """
    if mut == "round_partials":
        return False
    if mut == "relu6_no_upper":
        return "relu6" in (exact_act(c.act), exact_act(c.act2 if c.act2 is not None else c.act))
    if mut == "no_post":
        return c.rmode == "post" and exact_act(c.act) != "none"
    return applies(mut, c)


def act32(v, act, mut=()):
    if act == "relu":
        return v.clamp(min=0)
    if act == "relu6":
        return v.clamp(min=0) if "relu6_no_upper" in mut else v.clamp(0, 6)
    if act in ("sigmoid", "silu"):  # rcp(1 + exp2(c v)), every step in fp32
        sg = 1.0 / (1.0 + torch.exp2(torch.tensor(-1.442695041, dtype=torch.float32) * v))
        return sg if act == "sigmoid" else v * sg
    return v


def model(c, ops, dtype_name, mut=()):
    """-> y [N, Cout, Ho, Wo] in the dtype as the numerical model computes it, in fp32 on the CPU"""
    dtype = DTYPES[dtype_name]
    ho, wo = out_hw(c)
    w = pack_weight(c, ops.pack).float()
    scale, bias = (t.float() for t in pack_scale_bias(c, ops.pack))
    x = ops.x.float()
    pad = c.k // 2
    xp = F.pad(x, (pad, pad, pad, pad))
    groups = c.cin if c.kind == "dw" else 1
    cin_g = w.shape[1]
    chunks = [(c0, min(cin_g, c0 + 32)) for c0 in range(0, cin_g, 32)]
    last_c0 = 32 * ((cin_g - 1) // 32)
    steps = [(ky, kx, c0, c1) for ky in range(c.k) for kx in range(c.k) for c0, c1 in chunks]  # tap-major k-tiles
    kt_per = -(-len(steps) // c.splits)
    slabs = []
    for s in range(0, len(steps), kt_per):
        acc = torch.zeros(c.n, c.cout, ho, wo)
        for ky, kx, c0, c1 in steps[s:s + kt_per]:
            if "skip_last_chunk" in mut and c0 == last_c0:
                continue
            xs = xp[:, :, ky:ky + c.stride * (ho - 1) + 1:c.stride, kx:kx + c.stride * (wo - 1) + 1:c.stride]
            if c.kind == "dw":
                part = xs * w[:, 0, ky, kx].view(1, -1, 1, 1)
            else:
                part = torch.einsum("nchw,oc->nohw", xs[:, c0:c1], w[:, c0:c1, ky, kx])
                # ONE product (the centre tap of the last input channel) at the right border column only -- less than the whole tap of
                # all Cin channels a kernel would typically lose there: the smallest fault of that kind, the hardest for a judge to see
                if "drop_product" in mut and ky == pad and kx == pad and c1 == cin_g:
                    part[:, :, :, wo - 1] -= xs[:, cin_g - 1, :, wo - 1].unsqueeze(1) * w[:, cin_g - 1, ky, kx].view(1, -1, 1)
            if c.kind == "dw" and "drop_product" in mut and ky == pad and kx == pad:
                part[:, :, :, wo - 1] = 0
            if "round_partials" in mut:
                part = part.to(dtype).float()
            acc = acc + part
        slabs.append(acc)
    if "slab_twice" in mut and len(slabs) > 1:
        slabs.append(slabs[-1])
    acc = slabs[0]
    for s in slabs[1:]:
        acc = acc + s
    sc, bi = scale.view(1, -1, 1, 1), bias.view(1, -1, 1, 1)
    v = (acc + bi) * sc if "bias_before_scale" in mut else acc * sc + bi
    post = c.rmode == "post"
    pre = v if post else _per_channel(c, ops, lambda a: act32(v, a, mut))
    y = pre.to(dtype)
    if c.rmode:
        res = ops.res.float()
        if c.rmode == "half":
            if "half_index" in mut:  # odd rows read the coarse row below
                rows = torch.tensor([min((oy + 1) // 2, ho // 2 - 1) if oy % 2 else oy // 2 for oy in range(ho)])
                res = res[:, :, rows].repeat_interleave(2, 3)
            else:
                res = upsample2(res)
        s = y.float() + res
        if post and "no_post" not in mut:
            s = act32(s, ops.act, mut)
        y = s.to(dtype)
    if "swap_split" in mut and c.split is not None:
        y = y.clone()
        y[:, [c.split - 1, c.split]] = y[:, [c.split, c.split - 1]]
    if "ragged_copy" in mut and wo > 1:
        y = y.clone()
        y[c.n - 1, :, ho - 1, wo - 1] = y[c.n - 1, :, ho - 1, wo - 2]
    return y


def check_model(name, dtype_name, family, mut=(), position=0):
    """the judge on the CPU model (with mutations) -> rec"""
    c = BY_NAME[name]
    rec = new_rec("%s %s %s%s" % (name, dtype_name, family, " +" + "+".join(mut) if mut else ""))
    tr = truth(name, dtype_name, family, position)
    got = model(c, tr["ops"], dtype_name, mut)
    if family == "random":
        return judge(rec, c, got, tr, dtype_name, c.splits)
    return judge_exact(rec, got, tr, dtype_name)


# ---- running the layer ---------------------------------------------------------------------------------------------------------------
def native(c, ops, dtype_name):
    """the layer through fused_conv.conv_native -> (y joined on the CPU, kernel name, variant string)"""
    from ssds import _native as N
    from ssds.modeling.layers import fused_conv as FC

    pack = ops.pack
    for name in ("w", "scale", "bias"):
        t = getattr(pack, name)
        if t is not None and not t.is_cuda:
            setattr(pack, name, t.cuda())
    x = ops.x.cuda()
    if not c.in_nchw:
        x = x.contiguous(memory_format=torch.channels_last)
    before = FC.USE_WFRAG
    FC.USE_WFRAG = bool(c.wfrag)
    try:
        y = FC.conv_native(x, pack, act=ops.act, residual=ops.res.cuda() if ops.res is not None else None, nchw_out=c.nchw,
                           split=c.split, act2=ops.act2 if c.split is not None else None, res_mode=RES_MODE[c.rmode])
        kernel, variant = N.last_kernel(), N.last_variant()
    finally:
        FC.USE_WFRAG = before
    torch.cuda.synchronize()
    parts = y if isinstance(y, tuple) else (y,)
    for t in parts:
        assert t.is_contiguous() if c.nchw else t.is_contiguous(memory_format=torch.channels_last)
    return joined(y), kernel, variant


def instance_of(variant):
    return variant.split(" | ")[0]


def splits_of(variant):
    """the slabs of the launch, read back from the variant string (1 where the kernel has no split)"""
    m = re.search(r"\bk?splits=(\d+)", variant)
    return int(m.group(1)) if m else 1


def check_case(name, dtype_name, family="random", position=0):
    """one case of one family on the device: dispatch and instance first, then the family's check"""
    c = BY_NAME[name]
    rec = new_rec("%s %s %s%s" % (name, dtype_name, family, " @%d" % position if family == "onehot_x" else ""))
    tr = truth(name, dtype_name, family, position)
    if family != "random":
        bad = exact_conditions(c, tr, dtype_name)
        assert not bad, bad  # (a condition on the operands: the judge's own fault, not the kernels')
    got, rec["kernel"], rec["variant"] = native(c, tr["ops"], dtype_name)
    if rec["kernel"] != c.kernel:
        rec["failures"].append("dispatch: %s, listed %s" % (rec["kernel"], c.kernel))
    if instance_of(rec["variant"]) != c.variant:
        rec["failures"].append("instance: %r, listed %r" % (rec["variant"], c.variant))
    if family == "random":
        return judge(rec, c, got, tr, dtype_name, splits_of(rec["variant"])), got
    return judge_exact(rec, got, tr, dtype_name), got


# ---- the table of ratios one GPU run leaves behind ------------------------------------------------------------------------------------
def log_ratios(rec):
    """CONVJUDGE_RATIOS=<file>: one JSON line per judged case x dtype x family (profiles/r31_convjudge_ratios.jsonl is such a run)"""
    path = os.environ.get("CONVJUDGE_RATIOS")
    if path and rec["ratios"]:
        with open(path, "a") as f:
            f.write(json.dumps({"case": rec["what"], "kernel": rec["kernel"], "variant": rec["variant"], "element": rec["worst"],
                                "ratio": round(rec["ratios"]["y"], 4) if rec["ratios"]["y"] != float("inf") else "inf"}) + "\n")
