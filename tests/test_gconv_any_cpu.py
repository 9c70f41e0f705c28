"""Grouped 3x3 convolutions of any supported group width (csrc/ssdk_gconv_any.hip), the parts that need no GPU:
which layers of the registered RegNetX / ResNeXt backbones the HIP kernels cover, and the packed weight image against
its definition (include/ssdk.h "grouped image", fused_conv.pack_grouped_frag)."""
import numpy as np
import pytest

# group widths (channels per group) of the grouped 3x3 convolutions of every registered grouped backbone, as instantiated
# (nets/regnet.py clamps the width to the stage width and re-quantises the stage widths)
WIDTHS = {
    "RegNetX002": {8}, "RegNetX004": {16}, "RegNetX006": {24}, "RegNetX008": {16}, "RegNetX016": {24},
    "RegNetX032": {48}, "RegNetX040": {40}, "RegNetX064": {56},
    "RegNetX080": {120},  # (its first stage is 80 wide with width 80: ONE group, a dense convolution)
    "ResNeXt50_32x4d": {4, 8, 16, 32}, "ResNeXt101_32x8d": {8, 16, 32, 64},
}


def _registered():
    from ssds.modeling import nets

    return sorted(n for n in dir(nets) if n.startswith("RegNetX") or n.startswith("ResNeXt"))


def test_the_width_table_names_every_registered_grouped_backbone():
    assert _registered() == sorted(WIDTHS)


@pytest.mark.parametrize("name", sorted(WIDTHS))
def test_every_conv_of_the_grouped_backbones_is_covered(name):
    """Every nn.Conv2d of the backbone has a HIP kernel: conv_kind is not None -- for the ResNeXt 7x7 stem, which conv_kind
    does not describe, StemPack.supported (csrc/ssdk_stem.hip) -- and the grouped ones have the widths of the table."""
    import torch
    import torch.nn as nn
    from ssds.modeling import nets
    from ssds.modeling.layers import fused_conv as FC

    with torch.device("meta"):
        net = getattr(nets, name)(outputs=[4] if name.startswith("RegNet") else [5])
    widths, kinds = set(), set()
    for mname, m in net.named_modules():
        if not isinstance(m, nn.Conv2d):
            continue
        if m.kernel_size == (7, 7):
            assert mname == "conv1" and FC.StemPack.supported(m, net.bn1), mname
            continue
        kind = FC.conv_kind(m)
        assert kind is not None, "%s.%s is not covered: %s" % (name, mname, m)
        if 1 < m.groups < m.in_channels:
            gw = m.in_channels // m.groups
            widths.add(gw)
            kinds.add(kind)
            assert kind == ("g16" if gw == 16 else "gany"), (mname, kind)
    assert widths == WIDTHS[name], (name, widths)
    assert kinds <= {"g16", "gany"}


def test_kinds_that_existed_keep_their_names():
    import torch.nn as nn
    from ssds.modeling.layers.fused_conv import conv_kind

    assert conv_kind(nn.Conv2d(64, 64, 3, 1, 1, groups=4)) == "g16"
    assert conv_kind(nn.Conv2d(64, 64, 3, 1, 1, groups=64)) == "dw"
    assert conv_kind(nn.Conv2d(64, 128, 3, 1, 1)) == "dense"
    assert conv_kind(nn.Conv2d(3, 32, 3, 2, 1)) == "stem"
    assert conv_kind(nn.Conv2d(72, 72, 3, 2, 1, groups=3)) == "gany"
    assert conv_kind(nn.Conv2d(128, 128, 3, 1, 1, groups=32)) == "gany"   # 4 wide, an even number of groups
    assert conv_kind(nn.Conv2d(12, 12, 3, 1, 1, groups=3)) is None        # 4 wide, odd number of groups: no pairs
    assert conv_kind(nn.Conv2d(60, 60, 3, 1, 1, groups=5)) is None        # 12 wide: no multiple of 8
    assert conv_kind(nn.Conv2d(72, 144, 3, 1, 1, groups=3)) is None       # Cin != Cout
    assert conv_kind(nn.Conv2d(72, 72, 1, 1, 0, groups=3)) is None        # grouped 1x1
    assert conv_kind(nn.Conv2d(528, 528, 3, 1, 1, groups=2)) is None      # 264 wide: above the kernel's 256


def _unpack(img, groups, gw):
    """The layout comment of include/ssdk.h, read backwards, in numpy: image [groups * RB][KS][4][16][8] of uint16 ->
    (weights [groups][gw][9][gw], every padding element)."""
    rb, ks = (gw + 15) // 16, (9 * gw + 31) // 32
    assert img.shape == (groups * rb, ks, 4, 16, 8), img.shape
    # element (row, k) lives at [row // 16][k // 32][(k % 32) // 8][row % 16][k % 8]
    mat = img.transpose(0, 3, 1, 2, 4).reshape(groups, rb * 16, ks * 32)
    w = mat[:, :gw, :9 * gw].reshape(groups, gw, 9, gw)  # k = tap * gw + ci
    pad = np.concatenate([mat[:, gw:, :].ravel(), mat[:, :gw, 9 * gw:].ravel()])
    return w, pad


@pytest.mark.parametrize("dtype_name", ["bf16", "f16"])
@pytest.mark.parametrize("gw,groups", [(8, 7), (24, 3), (56, 2), (168, 2)])
def test_grouped_image_is_the_layout_the_header_defines(gw, groups, dtype_name):
    import torch
    import torch.nn as nn
    from ssds import _native as N
    from ssds.modeling.layers import fused_conv as FC

    dtype = torch.bfloat16 if dtype_name == "bf16" else torch.float16
    torch.manual_seed(gw)
    c = gw * groups
    conv = nn.Conv2d(c, c, 3, 1, 1, groups=groups, bias=False)
    pack = FC.ConvPack(conv, nn.BatchNorm2d(c), "relu", dtype)
    assert pack.kind == "gany" and pack.groups == groups
    img = pack.gfrag()
    assert img is pack.gfrag(), "the image is built once per weight tensor"
    assert img.dtype == dtype and img.is_contiguous()
    rb, ks = (gw + 15) // 16, (9 * gw + 31) // 32
    assert img.numel() * 2 == N.lib.ssdk_weight_frag_bytes(groups * rb * 16, ks * 32)
    w, pad = _unpack(img.view(torch.int16).numpy().view(np.uint16), groups, gw)
    want = conv.weight.detach().to(dtype).view(torch.int16).numpy().view(np.uint16)  # [C][gw][3][3]
    want = want.reshape(groups, gw, gw, 9).transpose(0, 1, 3, 2)                      # [g][co][tap][ci]
    assert np.array_equal(w, want)
    assert pad.size == groups * (rb * 16 * ks * 32 - gw * 9 * gw) and not pad.any(), "padding slots must be exact zeros"


def test_four_wide_groups_merge_into_block_diagonal_pairs():
    """gw = 4 (ResNeXt50 layer1): two neighbouring groups become one group of 8 whose off-diagonal 4 x 4 blocks are exact
    zeros and whose diagonal blocks are the original weights -- the added products are zeros, no result changes."""
    import torch
    from ssds.modeling.layers import fused_conv as FC

    torch.manual_seed(1)
    groups, c = 32, 128
    w = torch.randn(c, 3, 3, 4).to(torch.bfloat16)  # KRSC
    img, g2, gw2 = FC.pack_grouped_frag(w, groups)
    assert (g2, gw2) == (16, 8)
    got, pad = _unpack(img.view(torch.int16).numpy().view(np.uint16), g2, gw2)  # [16][8 co][9][8 ci]
    assert not pad.any()
    src = w.view(torch.int16).numpy().view(np.uint16).reshape(16, 2, 4, 9, 4)   # [pair][half][co][tap][ci]
    for half in (0, 1):
        rows = got[:, 4 * half:4 * half + 4]
        assert np.array_equal(rows[..., 4 * half:4 * half + 4], src[:, half]), "diagonal block"
        assert not rows[..., 4 * (1 - half):4 * (1 - half) + 4].any(), "off-diagonal block must be exact zeros"


def test_the_op_has_no_cpu_fallback():
    import torch
    import torch.nn as nn
    from ssds import _native as N
    from ssds.modeling.layers import fused_conv as FC

    conv = nn.Conv2d(48, 48, 3, 1, 1, groups=2, bias=False)
    pack = FC.ConvPack(conv, nn.BatchNorm2d(48), "relu", torch.bfloat16)
    with pytest.raises(N.SsdkError, match="no CPU fallback"):
        FC.conv_native(torch.zeros(1, 48, 8, 8, dtype=torch.bfloat16), pack)
