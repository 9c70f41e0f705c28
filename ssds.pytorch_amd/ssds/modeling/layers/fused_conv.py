"""Host side of the fused conv + folded-BN + activation kernels (C-ABI ``ssdk_conv`` /
``ssdk_conv_sequence``, csrc/ssdk_conv.hip).

* ``pack_conv(conv, bn, dtype)`` folds the BatchNorm running statistics into a per-channel fp32
  (scale, bias) pair and re-packs the weight once into the KRSC layout the kernels read.
* ``conv_native(x, pack, ...)`` launches one layer (activations are NHWC = torch ``channels_last``).
* ``ConvPlan`` records a whole network as an array of descriptors with pre-assigned activation buffers and
  replays it with ONE host call per forward (``ssdk_conv_sequence``): ~2 us of host time per layer instead
  of a Python round trip per layer, and trivially hipGraph-capturable.
* ``FusedSequentialMixin`` lets the reference-shaped nn.Sequential blocks (basic_layers.py) use the fused
  kernels in eval mode without changing their state_dict layout.

Switch: ``SSDK_FUSED_CONV`` = "1" (default: HIP kernels in eval mode on a HIP device) or "0" (torch/MIOpen
everywhere; for A/B measurements only, never chosen silently).
"""
import collections
import ctypes
import contextlib
import os
import threading

import torch
import torch.nn as nn
import torch.nn.functional as F

from ssds import _native as N

_ACT_OF = {nn.ReLU: "relu", nn.ReLU6: "relu6", nn.SiLU: "silu", nn.Sigmoid: "sigmoid"}


def _act_name(m):
    """Activation name of module ``m`` or None.  Looked up along the MRO: the training Solver swaps the classes of
    activations behind a kernel-backed BatchNorm to subclasses (batchnorm.FusedAwayReLU6 / FusedAwayReLU), and a model
    that went through it must still record its eval plan."""
    for klass in type(m).__mro__:
        if klass in _ACT_OF:
            return _ACT_OF[klass]
    return None

STATS = {"native_layers": 0, "plan_runs": 0, "torch_fallback_layers": 0}


def fused_enabled():
    return os.environ.get("SSDK_FUSED_CONV", "1") != "0"


def fold_bn(conv, bn):
    """-> (scale[Cout], bias[Cout]) fp32 such that bn(conv(x)) == conv_nobias(x) * scale + bias."""
    cout = conv.out_channels
    dev = conv.weight.device
    if bn is None:
        scale = torch.ones(cout, device=dev, dtype=torch.float32)
        bias = conv.bias.detach().float() if conv.bias is not None else torch.zeros(cout, device=dev)
        return scale, bias.contiguous()
    var = bn.running_var.detach().float()
    mean = bn.running_mean.detach().float()
    gamma = bn.weight.detach().float() if bn.affine else torch.ones_like(var)
    beta = bn.bias.detach().float() if bn.affine else torch.zeros_like(var)
    scale = gamma / torch.sqrt(var + bn.eps)
    b0 = conv.bias.detach().float() if conv.bias is not None else torch.zeros_like(mean)
    bias = (b0 - mean) * scale + beta
    return scale.contiguous(), bias.contiguous()


# SSDK_GCONV_ANY=0: grouped 3x3 layers whose width is not 16 are "not covered" again, so their backbone runs on
# PyTorch-ROCm as it did before csrc/ssdk_gconv_any.hip existed (A/B measurements only; docs/SWITCHES.md).
USE_GCONV_ANY = os.environ.get("SSDK_GCONV_ANY", "1") != "0"
GCONV_ANY_MAX_WIDTH = 256  # channels per group (csrc/ssdk_gconv_any.hip launch_gconv3x3_any)


class _PaddedMaps(threading.local):
    on = False
    depth = 0


_PADDED_MAPS = _PaddedMaps()


@contextlib.contextmanager
def padded_maps_scope():
    """The recording of ONE plan.  Inside it ``allow_padded_maps()`` -- called by a backbone recorder that produced a map whose
    channel count is no multiple of 8 (ShuffleNetV2: 116 -> 120, 244 -> 248 channels per pixel, zeros in the padding) -- lets
    ``conv_kind`` take the dense convolutions that read such a map: their packs zero-pad their input channels (``ConvPack.in_segs``).
    Outside a scope nothing changes: a module-path layer on a real 116-channel tensor stays 'not covered'."""
    before = _PADDED_MAPS.on
    _PADDED_MAPS.on = False
    _PADDED_MAPS.depth += 1
    try:
        yield
    finally:
        _PADDED_MAPS.depth -= 1
        _PADDED_MAPS.on = before


def allow_padded_maps():
    """For the rest of the enclosing ``padded_maps_scope`` (an error outside one: the switch would never be turned off)."""
    if _PADDED_MAPS.depth == 0:
        raise N.SsdkError("allow_padded_maps() outside padded_maps_scope()")
    _PADDED_MAPS.on = True


def in_padded_maps_scope():
    return _PADDED_MAPS.depth > 0


def pad8(c):
    return (c + 7) // 8 * 8


class PaddedValue(tuple):
    """A plan value ``(buffer, n, c, h, w)`` whose ``c`` PHYSICAL channels per pixel hold fewer real ones: ``segs`` = ((real,
    physical), ...) in channel order, zeros in every gap (one segment for a backbone map, several behind a concatenation)."""

    def __new__(cls, val, segs):
        self = super(PaddedValue, cls).__new__(cls, val)
        self.segs = tuple((int(r), int(q)) for r, q in segs)
        assert sum(q for _, q in self.segs) == val[2], (self.segs, val[2])
        return self

    @property
    def real_channels(self):
        return sum(r for r, _ in self.segs)


def value_segs(val):
    """((real, physical), ...) of a plan value; a plain value is one segment without padding."""
    return getattr(val, "segs", ((val[2], val[2]),))


def _pad_cols(w, segs):
    """[..., sum real] -> [..., sum physical]: zero columns behind every segment's real ones."""
    parts, at = [], 0
    for real, phys in segs:
        parts.append(w[..., at:at + real])
        at += real
        if phys > real:
            parts.append(w.new_zeros(tuple(w.shape[:-1]) + (phys - real,)))
    assert at == w.shape[-1], (segs, tuple(w.shape))
    return torch.cat(parts, -1).contiguous()


def _strip_cols(w, segs):
    parts, at = [], 0
    for real, phys in segs:
        parts.append(w[..., at:at + real])
        at += phys
    assert at == w.shape[-1], (segs, tuple(w.shape))
    return torch.cat(parts, -1).contiguous()


def conv_kind(conv):
    """'dense' | 'dw' | 'g16' | 'gany' | 'stem' | 'dilated' | None (None: not covered by the HIP kernels -> torch, reported).
    'dilated': a 3x3 / stride-1 convolution with padding == dilation == (d, d) that csrc/ssdk_dconv.hip takes (the BasicRFB extras);
    never 'dense' -- the heads, towers, xpair and the training swaps that ask for 'dense' keep ignoring such a layer."""
    k = conv.kernel_size
    if conv.dilation != (1, 1):
        d = conv.dilation[0]
        # (H and W are the planner's to check: the predicate's rule on the map is 1 <= H, W <= DCONV_MAX_SIDE)
        if (k == (3, 3) and conv.stride == (1, 1) and conv.dilation == (d, d) and conv.padding == (d, d) and conv.groups == 1
                and conv.padding_mode == "zeros"
                and N.lib.ssdk_dconv3x3_supported(conv.in_channels, conv.out_channels, 1, 1, d, N.BF16)):
            return "dilated"
        return None
    if not (k[0] == k[1] and k[0] in (1, 3) and conv.stride[0] == conv.stride[1] and conv.stride[0] in (1, 2)
            and conv.padding == (k[0] // 2, k[0] // 2) and conv.dilation == (1, 1)
            and conv.padding_mode == "zeros"):
        return None
    if conv.groups == 1:
        if conv.in_channels <= 4:
            # (24, inside padded_maps_scope: ShuffleNetV2's conv1, packed with its output rows zero-padded to 32 -- the stem kernel's
            #  widths are 16, 32, 64)
            return "stem" if (k[0] == 3 and (conv.out_channels in (16, 32, 64) or (conv.out_channels == 24 and _PADDED_MAPS.on))) else None
        # a channel count that is no multiple of 8 only inside a plan whose backbone hands out zero-padded maps (padded_maps_scope)
        return "dense" if conv.in_channels % 8 == 0 or _PADDED_MAPS.on else None
    if conv.groups == conv.in_channels == conv.out_channels and k[0] == 3 and conv.in_channels % 8 == 0:
        return "dw"
    if conv.in_channels == conv.out_channels == conv.groups * 16 and k[0] == 3:
        return "g16"  # 16 channels per group (RegNetX bottlenecks): csrc/ssdk_gconv.hip
    if conv.in_channels == conv.out_channels and k[0] == 3 and conv.in_channels % conv.groups == 0 and USE_GCONV_ANY:
        gw = conv.in_channels // conv.groups
        if (gw % 8 == 0 and gw <= GCONV_ANY_MAX_WIDTH) or (gw == 4 and conv.groups % 2 == 0):
            return "gany"  # any other width (RegNetX, ResNeXt): csrc/ssdk_gconv_any.hip, reads the grouped image
    return None


def pack_grouped_frag(w, groups):
    """Fragment-major image of the weights of a grouped 3x3 convolution for csrc/ssdk_gconv_any.hip (include/ssdk.h, "grouped
    image").  ``w``: KRSC [C][3][3][gw], gw = C / groups channels per group.  Pure layout, on the tensor's own device (CPU
    tensors too) -> (image [groups' * RB][KS][4][16][8], groups', gw'):

    * gw == 4 (ResNeXt50 layer1): neighbouring pairs of groups are merged into block-diagonal groups of gw' = 8 -- output
      channel j of a pair reads input channels 4 (j // 4) .. + 3 of the pair's 8, the other 4 slots are zeros.  The added
      products are exact zeros in an fp32 accumulator, so for finite inputs no result changes.  Otherwise gw' = gw.
    * per group a [RB * 16][Kpad] matrix: row = output channel of the group, k = tap * gw' + ci (tap = 3 ky + kx),
      RB = ceil(gw' / 16), Kpad = 32 * ceil(9 gw' / 32) = 32 KS, zeros in the padding rows and columns;
    * the groups concatenated along the rows, and that [groups' * RB * 16][Kpad] matrix in fragment-major order:
      element (row, k) at [row // 16][k // 32][(k % 32) // 8][row % 16][k % 8]."""
    c, kh, kw, gw = (int(v) for v in w.shape)
    assert kh == 3 and kw == 3 and c == groups * gw, (tuple(w.shape), groups)
    if gw == 4:
        assert groups % 2 == 0, groups
        wide = w.new_zeros((c // 8, 2, 4, 3, 3, 2, 4))
        src = w.reshape(c // 8, 2, 4, 3, 3, 4)
        wide[:, 0, :, :, :, 0] = src[:, 0]
        wide[:, 1, :, :, :, 1] = src[:, 1]
        w, groups, gw = wide.reshape(c, 3, 3, 8), groups // 2, 8
    assert gw % 8 == 0, gw
    rb, ks = (gw + 15) // 16, (9 * gw + 31) // 32
    mat = w.new_zeros((groups, rb * 16, ks * 32))
    mat[:, :gw, :9 * gw] = w.reshape(groups, gw, 9 * gw)
    img = mat.view(groups * rb, 16, ks, 4, 8).permute(0, 2, 3, 1, 4).contiguous()
    return img, groups, gw


# Fragment-major weight images for the kernels that stream weights into operand registers (ConvPack.frag); False keeps
# those kernels on the KRSC tensor (A/B runs and the test of that path).
USE_WFRAG = os.environ.get("SSDK_WFRAG", "1") != "0"


class ConvPack(object):
    """Weights of one fused layer in kernel layout (built once per model/dtype)."""

    __slots__ = ("kind", "w", "scale", "bias", "cin", "cout", "k", "stride", "groups", "act", "_frag", "in_segs", "cout_real", "dilation")

    def with_input_segs(self, segs):
        """A copy of this dense pack for an input laid out as ``segs`` = ((real, physical), ...): zero weight columns at every
        padding channel, so whatever the padding holds contributes nothing (and a produced map's padding IS zeros)."""
        segs = tuple((int(r), int(q)) for r, q in segs)
        if self.kind != "dense":
            raise N.SsdkError("a {} layer cannot read a zero-padded map".format(self.kind))
        real = _strip_cols(self.w, self.in_segs) if self.in_segs is not None else self.w
        if sum(r for r, _ in segs) != real.shape[-1]:
            raise N.SsdkError("a layer of {} input channels cannot read a map of {} real channels".format(
                real.shape[-1], sum(r for r, _ in segs)))
        other = ConvPack.__new__(ConvPack)
        for name in ConvPack.__slots__:
            setattr(other, name, getattr(self, name))
        other._frag = None
        other.in_segs = segs if any(r != q for r, q in segs) else None
        other.w = _pad_cols(real, segs)
        other.cin = sum(q for _, q in segs)
        return other

    def with_padded_output(self):
        """A copy of this dense pack that writes pad8(cout) channels per pixel: zero weight rows, zero scale and bias behind the real
        ones, so the padding channels of the map it produces are act(0) = 0 (act none | relu | relu6 | silu)."""
        if self.kind != "dense":
            raise N.SsdkError("a {} layer cannot write a zero-padded map".format(self.kind))
        other = ConvPack.__new__(ConvPack)
        for name in ConvPack.__slots__:
            setattr(other, name, getattr(self, name))
        other._frag = None
        extra = pad8(self.cout) - self.cout
        other.w = torch.cat([self.w, self.w.new_zeros((extra,) + tuple(self.w.shape[1:]))], 0).contiguous()
        other.bias = torch.cat([self.bias, self.bias.new_zeros(extra)]).contiguous()
        if self.scale is not None:
            other.scale = torch.cat([self.scale, self.scale.new_zeros(extra)]).contiguous()
        other.cout = pad8(self.cout)
        return other

    def frag(self):
        """Fragment-major image of the dense weights (include/ssdk.h ``ssdk_weight_frag_bytes``) for the kernels that stream
        weights straight into MFMA operand registers (conv_smallmap, xpair); None where no such kernel applies.  Built once
        per weight tensor (pure layout: [rows][K] -> [rows/16][K/32][4][16][8], rows zero-padded to a multiple of 16)."""
        k_elems = self.k * self.k * self.cin
        if (not USE_WFRAG or self.kind != "dense" or self.w.dtype not in (torch.bfloat16, torch.float16) or k_elems % 32
                or self.cin % 32):
            return None
        cached = getattr(self, "_frag", None)
        if cached is not None and cached[0] == (self.w.data_ptr(), self.w._version):
            return cached[1]
        rows = self.cout
        g = (rows + 15) // 16
        w2d = self.w.reshape(rows, k_elems)
        if g * 16 != rows:
            w2d = torch.cat([w2d, w2d.new_zeros((g * 16 - rows, k_elems))], 0)
        img = w2d.view(g, 16, k_elems // 32, 4, 8).permute(0, 2, 3, 1, 4).contiguous()
        assert img.numel() * 2 == N.lib.ssdk_weight_frag_bytes(rows, k_elems)
        self._frag = ((self.w.data_ptr(), self.w._version), img)
        return img

    def gfrag(self):
        """Grouped image of a 'gany' layer (pack_grouped_frag): the ONLY weight tensor its kernel reads, so it is built whatever
        USE_WFRAG says.  Cached like frag(); the pack, which every plan keeps, keeps the image alive."""
        assert self.kind == "gany", self.kind
        cached = getattr(self, "_frag", None)
        if cached is not None and cached[0] == (self.w.data_ptr(), self.w._version):
            return cached[1]
        img, groups, gw = pack_grouped_frag(self.w, self.groups)
        assert img.numel() * 2 == N.lib.ssdk_weight_frag_bytes(groups * ((gw + 15) // 16) * 16, 32 * ((9 * gw + 31) // 32))
        self._frag = ((self.w.data_ptr(), self.w._version), img)
        return img

    def dfrag(self):
        """Weight image of a 'dilated' layer (csrc/ssdk_dconv.hip, include/ssdk_dconv.h): the fragment-major image of the matrix
        [Cout][Kpad], k = tap * Cin + ci (tap = 3 ky + kx), Kpad = 32 * ceil(9 Cin / 32), zero columns behind 9 Cin and zero rows behind
        Cout -- the k order of ``pack_grouped_frag`` for ONE group as wide as the layer.  The only weight tensor the kernel reads, so it
        is built whatever USE_WFRAG says.  Cached like frag()."""
        assert self.kind == "dilated", self.kind
        cached = getattr(self, "_frag", None)
        if cached is not None and cached[0] == (self.w.data_ptr(), self.w._version):
            return cached[1]
        rows, k_elems = self.cout, 9 * self.cin
        g, ks = (rows + 15) // 16, (k_elems + 31) // 32
        mat = self.w.new_zeros((g * 16, ks * 32))
        mat[:rows, :k_elems] = self.w.reshape(rows, k_elems)
        img = mat.view(g, 16, ks, 4, 8).permute(0, 2, 3, 1, 4).contiguous()
        assert img.numel() * 2 == N.lib.ssdk_weight_frag_bytes(rows, ks * 32)
        self._frag = ((self.w.data_ptr(), self.w._version), img)
        return img

    def __init__(self, conv, bn, act, dtype, extra_cout=None):
        self._frag = None
        self.dilation = int(conv.dilation[0])  # 1 for every kind but 'dilated'
        self.in_segs = None
        self.cout_real = conv.out_channels
        self.kind = conv_kind(conv)
        if self.kind is None:
            raise N.SsdkError("conv {} is not covered by the HIP kernels".format(conv))
        scale, bias = fold_bn(conv, bn)
        w = conv.weight.detach().float()
        self.cin, self.cout = conv.in_channels, conv.out_channels
        self.k, self.stride, self.groups, self.act = conv.kernel_size[0], conv.stride[0], conv.groups, act
        if self.kind == "stem":  # fp32 weights with the BN scale folded in, KRSC
            self.w = (w * scale.view(-1, 1, 1, 1)).permute(0, 2, 3, 1).contiguous()
            self.scale = None
            if self.cout not in (16, 32, 64):  # zero output rows up to the stem kernel's next width: relu(0) = 0 in the padding
                wide = min(c for c in (16, 32, 64) if c >= self.cout)
                self.w = torch.cat([self.w, self.w.new_zeros((wide - self.cout,) + tuple(self.w.shape[1:]))], 0).contiguous()
                bias = torch.cat([bias, bias.new_zeros(wide - self.cout)]).contiguous()
                self.cout = wide
        elif self.kind == "dw":  # [C,1,3,3] -> [3][3][C]
            self.w = w[:, 0].permute(1, 2, 0).contiguous().to(dtype)
            self.scale = scale
        else:  # [Cout,Cin,kh,kw] -> [Cout][kh][kw][Cin]
            self.w = w.permute(0, 2, 3, 1).contiguous().to(dtype)
            if self.kind == "dense" and self.cin % 8:  # reads a zero-padded map (conv_kind: only inside padded_maps_scope)
                self.in_segs = ((self.cin, pad8(self.cin)),)
                self.w = _pad_cols(self.w, self.in_segs)
                self.cin = pad8(self.cin)
            # (the grouped kernels have no scale-free form: a layer without BatchNorm passes fold_bn's vector of ones)
            self.scale = scale if bn is not None or self.kind in ("g16", "gany") else None
        self.bias = bias


class StemPack(object):
    """7x7 / stride 2 / pad 3 stem conv on a 3-channel image + BN + activation (ResNet conv1/bn1/relu) packed for
    csrc/ssdk_stem.hip: weights [Cout][ky 7][kx padded to 8][ci padded to 4], zeros in the padding slots."""

    __slots__ = ("w", "scale", "bias", "cin", "cout", "act")

    @staticmethod
    def supported(conv, bn):
        return (bn is not None and conv.kernel_size == (7, 7) and conv.stride == (2, 2) and conv.padding == (3, 3)
                and conv.groups == 1 and conv.in_channels == 3 and conv.out_channels in (32, 64))

    def __init__(self, conv, bn, act, dtype):
        self.scale, self.bias = fold_bn(conv, bn)
        w = conv.weight.detach().float().permute(0, 2, 3, 1)  # [Cout][ky][kx][ci]
        wp = torch.zeros((conv.out_channels, 7, 8, 4), device=w.device, dtype=torch.float32)
        wp[:, :, :7, :3] = w
        self.w = wp.to(dtype).contiguous()
        self.cin, self.cout, self.act = 3, conv.out_channels, act


def _out_tensor(y, shape, like, memory_format, what):
    """The output of a ``*_native`` call: a fresh ``torch.empty`` (``y`` None), or the caller's own buffer once it is what the
    call would have allocated -- shape, dtype, device and memory format -- since the kernel is handed its bare address."""
    shape = tuple(int(v) for v in shape)
    if y is None:
        return torch.empty(shape, device=like.device, dtype=like.dtype, memory_format=memory_format)
    if (tuple(y.shape) != shape or y.dtype != like.dtype or y.device != like.device
            or not y.is_contiguous(memory_format=memory_format)):
        raise N.SsdkError("{}: the output handed in is {} {} on {} with strides {}, expected {} {} on {} in {}".format(
            what, tuple(y.shape), y.dtype, y.device, tuple(y.stride()), shape, like.dtype, like.device,
            "channels_last" if memory_format == torch.channels_last else "contiguous"))
    return y


def _out_shape(kind, **L):
    """(c, ho, wo) of an op of ``kind`` on the layer-dict entries ``L``: the op table's geometry (``OP_KINDS[kind].out``), for the
    ``*_native`` wrappers, which have no layer dict."""
    return OP_KINDS[kind].out(L)


def fill_stem_desc(d, x_ptr, y_ptr, n, h, w, cin, pack, dtype_code, in_layout):
    d.x, d.w, d.scale, d.bias, d.y = x_ptr, pack.w.data_ptr(), pack.scale.data_ptr(), pack.bias.data_ptr(), y_ptr
    d.N, d.H, d.W, d.Cin, d.Cout, d.act, d.dtype, d.in_layout = n, h, w, cin, pack.cout, N.ACT[pack.act], dtype_code, in_layout
    return d


def stem7_native(x, pack, y=None):
    """[N,3,H,W] image (NCHW contiguous or channels_last) -> channels_last [N,Cout,H/2,W/2] (``y``: write there)."""
    N.require_device(x, "conv_stem7")
    n, c, h, w = (int(v) for v in x.shape)
    layout = N.NCHW
    if not x.is_contiguous():
        x = x.contiguous(memory_format=torch.channels_last)
        layout = N.NHWC
    y = _out_tensor(y, (n,) + _out_shape("stem7", pack=pack, h=h, w=w), x, torch.channels_last, "conv_stem7")
    d = fill_stem_desc(N.StemDesc(), x.data_ptr(), y.data_ptr(), n, h, w, c, pack, N.dtype_code(x), layout)
    with torch.cuda.device(x.device):
        rc = N.lib.ssdk_conv_stem7(ctypes.byref(d), N.stream_ptr(x.device))
    N.check(rc, "conv_stem7")
    return y


def fill_pool_desc(d, x_ptr, y_ptr, n, h, w, c, dtype_code):
    d.x, d.y = x_ptr, y_ptr
    d.N, d.H, d.W, d.C, d.dtype = n, h, w, c, dtype_code
    return d


def maxpool_native(x, y=None):
    """F.max_pool2d(x, 3, 2, 1) on a channels_last tensor (``y``: write there)."""
    N.require_device(x, "maxpool3x3s2")
    if not x.is_contiguous(memory_format=torch.channels_last):
        x = x.contiguous(memory_format=torch.channels_last)
    n, c, h, w = (int(v) for v in x.shape)
    y = _out_tensor(y, (n,) + _out_shape("pool", ch=c, h=h, w=w), x, torch.channels_last, "maxpool3x3s2")
    d = fill_pool_desc(N.PoolDesc(), x.data_ptr(), y.data_ptr(), n, h, w, c, N.dtype_code(x))
    with torch.cuda.device(x.device):
        rc = N.lib.ssdk_maxpool3x3s2(ctypes.byref(d), N.stream_ptr(x.device))
    N.check(rc, "maxpool3x3s2")
    return y


def pack_heads(loc_conv, conf_conv, dtype):
    """loc | conf of one SSD level as ONE GEMM with N = A*(4+C): concatenated KRSC weights + biases."""
    p = ConvPack(loc_conv, None, "none", dtype)
    q = ConvPack(conf_conv, None, "none", dtype)
    p.w = torch.cat([p.w, q.w], 0).contiguous()
    p.bias = torch.cat([p.bias, q.bias], 0).contiguous()
    p.cout = loc_conv.out_channels + conf_conv.out_channels
    return p


class MbPack(object):
    """One MobileNetV2 inverted-residual block (expand 1x1 -> depthwise 3x3 -> project 1x1) packed for the
    fused block kernel (csrc/ssdk_mbconv.hip).  ``groups`` = [(conv, bn, act)] x 3 as produced by
    ``sequential_groups`` on the flattened block."""

    __slots__ = ("e", "d", "p", "we", "wd", "bd", "wp", "cin", "chid", "cout", "stride", "residual", "stem", "_image")

    @staticmethod
    def supported(groups, residual):
        if len(groups) != 3:
            return False
        (ce, _, ae), (cd, _, ad), (cp, _, ap) = groups
        return (conv_kind(ce) == "dense" and ce.kernel_size == (1, 1) and ce.stride == (1, 1) and ae == "relu6"
                and conv_kind(cd) == "dw" and ad == "relu6"
                and conv_kind(cp) == "dense" and cp.kernel_size == (1, 1) and cp.stride == (1, 1) and ap == "none"
                and ce.in_channels <= 160 and cp.out_channels <= 320 and cp.out_channels % 8 == 0
                and ce.out_channels == cd.in_channels == cp.in_channels
                and all(bn is not None for _, bn, _ in groups)
                and (not residual or (cd.stride[0] == 1 and ce.in_channels == cp.out_channels)))

    @staticmethod
    def stem_supported(stem_groups, block_groups):
        """network stem (3x3/s2 conv on <=3 channels, BN, ReLU6) + an expand-free block (dw, pw-linear)."""
        if len(stem_groups) != 1 or len(block_groups) != 2:
            return False
        (cs, bs, a_s), (cd, bdn, ad), (cp, bpn, ap) = stem_groups[0], block_groups[0], block_groups[1]
        return (cs.kernel_size == (3, 3) and cs.stride == (2, 2) and cs.padding == (1, 1) and cs.groups == 1
                and 9 * cs.in_channels <= 32 and cs.out_channels % 8 == 0 and a_s == "relu6" and bs is not None
                and conv_kind(cd) == "dw" and ad == "relu6" and cd.in_channels == cs.out_channels
                and conv_kind(cp) == "dense" and cp.kernel_size == (1, 1) and cp.stride == (1, 1) and ap == "none"
                and cp.out_channels <= 64 and cp.out_channels % 8 == 0 and bdn is not None and bpn is not None)

    def __init__(self, groups, residual, dtype, stem_group=None):
        self.stem = 0
        self._image = None
        if stem_group is not None:  # the stem conv plays the role of the expand conv
            cs, bs, _ = stem_group
            (cd, bd, _), (cp, bp, _) = groups
            scale, bias = fold_bn(cs, bs)
            # K layout of the stem GEMM = (ky, kx padded 3 -> 8, ci padded -> 4): a k-step is one kernel row and a
            # lane's 8 k-values are 2 neighbouring patch pixels x 4 channels (csrc/ssdk_mbconv.hip stem mode)
            w = cs.weight.detach().float().permute(0, 2, 3, 1)  # [Cout][ky][kx][ci]
            wpad = torch.zeros((cs.out_channels, 3, 8, 4), device=w.device, dtype=torch.float32)
            wpad[:, :, :3, : w.shape[3]] = w
            self.e = ConvPack.__new__(ConvPack)
            # the BN scale goes into the weights BEFORE they are rounded (the block kernels then apply a scale of exactly 1:
            # csrc/ssdk_mbflow.hip starts its expand MFMA from the BN bias and has no BN arithmetic left in the row loop)
            wpad = wpad * scale.view(-1, 1, 1, 1)
            self.e.w, self.e.scale, self.e.bias = wpad.reshape(cs.out_channels, 96).to(dtype).contiguous(), torch.ones_like(scale), bias
            self.d = ConvPack(cd, bd, "relu6", dtype)
            self.p = ConvPack(cp, bp, "none", dtype)
            self.cin, self.chid, self.cout = cs.in_channels, cs.out_channels, cp.out_channels
            self.stride, self.residual, self.stem = cd.stride[0], False, 1
            self._fold_tail(cd, bd, cp)
            return
        (ce, be, _), (cd, bd, _), (cp, bp, _) = groups
        self.e = ConvPack(ce, be, "relu6", dtype)
        # expand BN scale folded into the weights before rounding (see the stem case above); KRSC [Chid][1][1][Cin]
        w_e = ce.weight.detach().float().permute(0, 2, 3, 1) * self.e.scale.view(-1, 1, 1, 1)
        self.e.w, self.e.scale = w_e.contiguous().to(dtype), torch.ones_like(self.e.scale)
        self.d = ConvPack(cd, bd, "relu6", dtype)
        self.p = ConvPack(cp, bp, "none", dtype)
        self.cin, self.chid, self.cout = ce.in_channels, ce.out_channels, cp.out_channels
        self.stride, self.residual = cd.stride[0], bool(residual)
        self._fold_tail(cd, bd, cp)

    def _fold_tail(self, cd, bd, cp):
        # internal tensors are fp16: depthwise weights with the BN scale folded in, fp16 bias, fp16 projection
        sd, bdv = fold_bn(cd, bd)
        wdw = cd.weight.detach().float()[:, 0] * sd.view(-1, 1, 1)  # [C,3,3]
        self.wd = wdw.permute(1, 2, 0).contiguous().to(torch.float16)
        self.bd = bdv.to(torch.float16).contiguous()
        self.wp = cp.weight.detach().float().permute(0, 2, 3, 1).contiguous().to(torch.float16)


    def image(self, w_in, nw=None):
        """(nw, tensor) -- the image of the two 1x1 weight matrices and the per-channel constants for csrc/ssdk_mbk.hip
        (layout: include/ssdk.h ``ssdk_mbconv_desc.w_image``) on a map ``w_in`` pixels wide, or None where no instance of that
        kernel takes the block.  Built once per pack and output width: pure permutations of ``e.w`` (activation dtype, BN
        scale folded in), ``wp`` / ``wd`` (fp16) and the folded biases, carried as 16-bit words.  ``nw``: slices of the hidden
        channels = waves per work item (4)."""
        if self.stem or self.stride not in (1, 2):
            return None
        nw = 4 if nw is None else int(nw)
        wo = (w_in + 2 - 3) // self.stride + 1
        if w_in != wo * self.stride:
            return None
        key = (nw, wo)
        if self._image is not None and self._image[0] == key:
            return self._image[1]
        nfo_c = ctypes.c_int(0)
        need = int(N.lib.ssdk_mbk_image_bytes(self.cin, self.chid, self.cout, self.stride, wo, nw, ctypes.byref(nfo_c)))
        if need == 0:
            self._image = (key, None)
            return None
        ks, nch, nfo = self.cin // 32, self.chid // 16, int(nfo_c.value)
        nchw = (nch + nw - 1) // nw
        npair = (nchw + 1) // 2
        halves = self.cout // (16 * nfo)
        dev = self.wp.device
        we = self.e.w.reshape(self.chid, self.cin).view(torch.int16)
        wp = self.wp.reshape(self.cout, self.chid).view(torch.int16)
        we = torch.cat([we, we.new_zeros((1, self.cin))], 0)      # row chid = the zero row of a chunk beyond the slice / Chid
        wp = torch.cat([wp, wp.new_zeros((self.cout, 1))], 1)     # column chid likewise
        ar = lambda n: torch.arange(n, device=dev)  # noqa: E731
        lane = ar(64)
        fr, fg = lane & 15, lane >> 4
        # expand fragments [slice w][pair t][chunk cc][k-step][lane][8]
        w_, t_, cc_, ks_, j_ = ar(nw).view(-1, 1, 1, 1, 1, 1), ar(npair).view(1, -1, 1, 1, 1, 1), ar(2).view(1, 1, -1, 1, 1, 1), \
            ar(ks).view(1, 1, 1, -1, 1, 1), ar(8).view(1, 1, 1, 1, 1, -1)
        loc = 2 * t_ + cc_
        chunk = w_ * nchw + loc
        ok = (loc < nchw) & (chunk < nch)
        row = torch.where(ok, chunk * 16 + fr.view(1, 1, 1, 1, -1, 1), torch.full_like(chunk, self.chid))
        col = (32 * ks_ + 8 * fg.view(1, 1, 1, 1, -1, 1) + j_).expand(nw, npair, 2, ks, 64, 8)
        exp = we[row.expand(nw, npair, 2, ks, 64, 8), col]                                  # [nw, np, 2, ks, 64, 8]
        # projection fragments [half h][slice w][pair t][fragment f][lane][8]
        h_, w2, t2, f_, j2 = ar(halves).view(-1, 1, 1, 1, 1, 1), ar(nw).view(1, -1, 1, 1, 1, 1), ar(npair).view(1, 1, -1, 1, 1, 1), \
            ar(nfo).view(1, 1, 1, -1, 1, 1), ar(8).view(1, 1, 1, 1, 1, -1)
        loc2 = 2 * t2 + j2 // 4
        chunk2 = w2 * nchw + loc2
        ok2 = (loc2 < nchw) & (chunk2 < nch)
        hid = torch.where(ok2, chunk2 * 16 + 4 * fg.view(1, 1, 1, 1, -1, 1) + j2 % 4, torch.full_like(chunk2 + fg.view(1, 1, 1, 1, -1, 1), self.chid))
        co = (h_ * (16 * nfo) + 16 * f_ + fr.view(1, 1, 1, 1, -1, 1)).expand(halves, nw, npair, nfo, 64, 8)
        prj = wp[co, hid.expand(halves, nw, npair, nfo, 64, 8)]                               # [halves, nw, np, nfo, 64, 8]
        wts = torch.cat([exp.reshape(1, nw, npair, 2 * ks * 512).expand(halves, -1, -1, -1),
                         prj.reshape(halves, nw, npair, nfo * 512)], 3).reshape(-1)
        # per-slice constants, laid out as the kernel reads them: bias_expand fp32 | taps fp16 | bias_dw / 6 fp16
        c_, g_, q_ = ar(nchw).view(1, -1, 1, 1), ar(4).view(1, 1, -1, 1), ar(4).view(1, 1, 1, -1)
        gc = ar(nw).view(-1, 1, 1, 1) * nchw + c_
        ch = torch.where(gc < nch, gc * 16 + 4 * g_ + q_, torch.full_like(gc + g_ + q_, self.chid))   # [nw, nchw, 4, 4]
        zf = lambda t: torch.cat([t, t.new_zeros((1,) + tuple(t.shape[1:]))], 0)  # noqa: E731 -- index chid = zeros
        be = zf(self.e.bias.float())[ch]                                                           # fp32 [nw, nchw, 4, 4]
        wd = zf(self.wd.reshape(9, self.chid).t().contiguous())[ch]                                # fp16 [nw, nchw, 4, 4, 9]
        wd = wd.permute(0, 1, 4, 2, 3).contiguous()                                                # [nw, nchw, 9, 4, 4]
        bd6 = zf((self.bd.float() * torch.tensor(1.0 / 6.0, dtype=torch.float32, device=dev)).to(torch.float16))[ch]
        misc_kb = (nchw * 384 + 1023) // 1024
        misc = torch.cat([be.contiguous().view(torch.int16).reshape(nw, -1), wd.view(torch.int16).reshape(nw, -1),
                          bd6.contiguous().view(torch.int16).reshape(nw, -1)], 1)
        misc = torch.cat([misc, misc.new_zeros((nw, misc_kb * 512 - misc.shape[1]))], 1).reshape(-1)
        # projection BN per half: [nfo][4 g][scale * 6 (4 q) | bias (4 q)] fp32
        cof = (ar(halves).view(-1, 1, 1, 1) * (16 * nfo) + 16 * ar(nfo).view(1, -1, 1, 1) + 4 * ar(4).view(1, 1, -1, 1)
               + ar(4).view(1, 1, 1, -1))
        spb = torch.cat([(self.p.scale.float() * 6.0)[cof], self.p.bias.float()[cof]], 3).contiguous()  # [halves, nfo, 4, 8]
        spb = spb.view(torch.int16).reshape(halves, -1)
        spb = torch.cat([spb, spb.new_zeros((halves, 1024 - spb.shape[1]))], 1).reshape(-1)
        img = torch.cat([wts, misc, spb]).contiguous()
        assert img.numel() * 2 == need, (img.numel() * 2, need)
        self._image = (key, (nw, img))
        return self._image[1]

    def fp16_safe(self):
        """The block kernel keeps the expanded tensor, the depthwise weights / bias / output and the projection weights
        in fp16 (11-bit mantissa: more precise than bf16 inside its range, but the range is 65504).  Everything the
        kernel rounds to fp16 is bounded here from the folded weights: the expanded tensor is clamped to [0, 6], so a
        depthwise output is at most 6 * sum|w| + |b| before its own clamp.  False -> the planner records the block as
        three layer launches (bf16 / fp32 accumulators) instead."""
        if not (torch.isfinite(self.wd).all() and torch.isfinite(self.bd).all() and torch.isfinite(self.wp).all()):
            return False
        bound = 6.0 * self.wd.float().abs().sum((0, 1)) + self.bd.float().abs()  # per channel
        return bool(bound.max() < 3.0e4)


# ---- EfficientNet MBConv tail (csrc/ssdk_mbse.hip): depthwise k x k + SiLU, squeeze-excite gate, gated projection ----------
# SSDK_MBSE=0 (read when a plan is recorded): planner.record_efficientnet raises PlanUnsupported, so an EfficientNet backbone
# runs module by module on PyTorch-ROCm (A/B measurements only; docs/SWITCHES.md).
def mbse_enabled():
    return os.environ.get("SSDK_MBSE", "1") != "0"


MBSE_TILE = 16  # output pixels per tile side of mbse_dw_kernel (ssdk_mbse_pool_tiles)


def mbse_pool_tiles(h, w, k, stride):
    """T of pool_partial [N][T][C] -- the Python mirror of ssdk_mbse_pool_tiles (the CPU-side plan walk has no library call
    to make for it; tests compare the two)."""
    ho, wo = _out_hw(h, w, k, stride)
    return ((ho + MBSE_TILE - 1) // MBSE_TILE) * ((wo + MBSE_TILE - 1) // MBSE_TILE)


# Summation depths of the three mbse kernels = the longest chain of fp32 additions an input term passes through (what the
# error bars of tests/mbseaudit.py are derived from, as dwconv.DW_SUM_DEPTH is for the depthwise training kernels):
#   pool:  a lane of mbse_dw_kernel adds the pixels of its slot in index order -- a workgroup has 256 // cgb slots with cgb <= 32
#          channel octets, so >= 8 slots share the 256 pixels of a tile: <= 32 additions; the slots are added as a binary tree
#          over <= 256 slots: 8 levels; mbse_gate_kernel adds the T tiles in four contiguous quarters (ceil(T / 4) additions each),
#          the four quarters in order (3) and divides once (1).
#   FC1:   a lane adds channels l, l + 64, ... (ceil(C / 64) fused multiply-adds), a 6-level butterfly, the bias (1).
#   FC2:   R fused multiply-adds in index order, the bias (1).
def MBSE_POOL_DEPTH(tiles):
    return 32 + 8 + (int(tiles) + 3) // 4 + 3 + 1


def MBSE_FC1_DEPTH(c):
    return (int(c) + 63) // 64 + 6 + 1


def MBSE_FC2_DEPTH(r):
    return int(r) + 1


MBSE_MAX_C, MBSE_MAX_R = 4096, 1024  # csrc/ssdk_mbse.hip kMbseMaxC / kMbseMaxR (LDS of the gate kernel)


class MbSePack(object):
    """Everything behind the expand 1x1 of one EfficientNet ``MBConvBlock`` (nets/efficientnet.py) packed for
    ``ssdk_mbse``: depthwise weights [k][k][C] and projection weights [Cout][C] in the activation dtype, their folded
    BatchNorms and the two squeeze-excite layers ([R][C], [C][R] + biases) in fp32."""

    __slots__ = ("w_dw", "scale_dw", "bias_dw", "w_se1", "b_se1", "w_se2", "b_se2", "w_proj", "scale_proj", "bias_proj",
                 "cin", "cout", "r", "k", "stride", "residual")

    @staticmethod
    def _modules(block):
        _, dw, se, proj, bn = block.parts()
        se_mods = list(se.se.children())
        return dw[0], dw[1], dw[2], se_mods, proj, bn

    @staticmethod
    def supported(block):
        """The host-side mirror of ssdk_mbse's argument checks (plus the module pattern the pack is built from)."""
        try:
            cd, bd, ad, se_mods, cp, bp = MbSePack._modules(block)
        except (AttributeError, ValueError, IndexError, TypeError):
            return False
        if len(se_mods) != 5 or not isinstance(se_mods[0], nn.AdaptiveAvgPool2d) or se_mods[0].output_size not in (1, (1, 1)):
            return False
        f1, a1, f2, a2 = se_mods[1:]
        k, c = cd.kernel_size[0], cd.in_channels
        return (isinstance(cd, nn.Conv2d) and isinstance(bd, nn.BatchNorm2d) and _act_name(ad) == "silu"
                and cd.kernel_size in ((3, 3), (5, 5)) and cd.stride in ((1, 1), (2, 2)) and cd.padding == (k // 2, k // 2)
                and cd.dilation == (1, 1) and cd.padding_mode == "zeros" and cd.bias is None
                and cd.groups == c == cd.out_channels and c % 8 == 0 and c <= MBSE_MAX_C
                and all(isinstance(f, nn.Conv2d) and f.kernel_size == (1, 1) and f.stride == (1, 1) and f.padding == (0, 0)
                        and f.groups == 1 and f.bias is not None for f in (f1, f2))
                and f1.in_channels == c == f2.out_channels and f1.out_channels == f2.in_channels
                and 1 <= f1.out_channels <= MBSE_MAX_R and _act_name(a1) == "silu" and _act_name(a2) == "sigmoid"
                and isinstance(cp, nn.Conv2d) and cp.kernel_size == (1, 1) and cp.stride == (1, 1) and cp.padding == (0, 0)
                and cp.groups == 1 and cp.in_channels == c and cp.out_channels % 8 == 0 and cp.bias is None
                and isinstance(bp, nn.BatchNorm2d) and bd.affine and bp.affine)

    def __init__(self, block, dtype):
        """``dtype``: bfloat16 | float16 for the kernels (folded BN and SE layers then fp32, as ssdk_mbse reads them); float64 keeps
        every tensor in fp64 (the CPU tests compare the pack with the module at that precision).  The BatchNorms are folded in
        fp64 either way and rounded once."""
        cd, bd, _, se_mods, cp, bp = MbSePack._modules(block)
        f1, f2 = se_mods[1], se_mods[3]
        aux = torch.float64 if dtype == torch.float64 else torch.float32
        self.cin, self.cout, self.r = cd.in_channels, cp.out_channels, f1.out_channels
        self.k, self.stride, self.residual = cd.kernel_size[0], cd.stride[0], bool(block.use_residual)

        def fold(bn):
            scale = bn.weight.detach().double() / torch.sqrt(bn.running_var.detach().double() + bn.eps)
            bias = bn.bias.detach().double() - bn.running_mean.detach().double() * scale
            return scale.to(aux).contiguous(), bias.to(aux).contiguous()

        self.scale_dw, self.bias_dw = fold(bd)
        self.w_dw = cd.weight.detach()[:, 0].permute(1, 2, 0).contiguous().to(dtype)  # [C,1,k,k] -> [k][k][C]
        self.w_se1 = f1.weight.detach().reshape(self.r, self.cin).to(aux).contiguous()
        self.b_se1 = f1.bias.detach().to(aux).contiguous()
        self.w_se2 = f2.weight.detach().reshape(self.cin, self.r).to(aux).contiguous()
        self.b_se2 = f2.bias.detach().to(aux).contiguous()
        self.scale_proj, self.bias_proj = fold(bp)
        self.w_proj = cp.weight.detach().reshape(self.cout, self.cin).contiguous().to(dtype)


def fill_mbse_desc(d, pk, n, h, w, dtype_code, x=None, t=None, pool_partial=None, gate=None, y=None, residual=None, stages=0):
    d.x, d.t, d.pool_partial, d.gate, d.y, d.residual = x, t, pool_partial, gate, y, residual
    d.w_dw, d.scale_dw, d.bias_dw = pk.w_dw.data_ptr(), pk.scale_dw.data_ptr(), pk.bias_dw.data_ptr()
    d.w_se1, d.b_se1, d.w_se2, d.b_se2 = pk.w_se1.data_ptr(), pk.b_se1.data_ptr(), pk.w_se2.data_ptr(), pk.b_se2.data_ptr()
    d.w_proj, d.scale_proj, d.bias_proj = pk.w_proj.data_ptr(), pk.scale_proj.data_ptr(), pk.bias_proj.data_ptr()
    d.N, d.H, d.W, d.C, d.R, d.Cout, d.k, d.stride = n, h, w, pk.cin, pk.r, pk.cout, pk.k, pk.stride
    d.dtype, d.stages = dtype_code, stages
    return d


def mbse_native(x, pk, residual=None, stages=0, t=None, pool_partial=None, gate=None, y=None):
    """One ``ssdk_mbse`` call on channels_last tensors.  ``stages`` = 0 runs the whole tail; a mask (N.MBSE_DW | MBSE_GATE |
    MBSE_PROJ) runs those stages on the buffers handed in (the others are allocated).  -> dict(t, pool_partial, gate, y)."""
    N.require_device(x, "mbse")
    if not x.is_contiguous(memory_format=torch.channels_last):
        x = x.contiguous(memory_format=torch.channels_last)
    n, c, h, w = (int(v) for v in x.shape)
    _, ho, wo = _out_shape("mbse", pack=pk, h=h, w=w)
    tiles = mbse_pool_tiles(h, w, pk.k, pk.stride)
    dev = x.device
    t = torch.empty((n, c, ho, wo), device=dev, dtype=x.dtype, memory_format=torch.channels_last) if t is None else t
    pool_partial = torch.empty((n, tiles, c), device=dev, dtype=torch.float32) if pool_partial is None else pool_partial
    gate = torch.empty((n, c), device=dev, dtype=torch.float32) if gate is None else gate
    y = torch.empty((n, pk.cout, ho, wo), device=dev, dtype=x.dtype, memory_format=torch.channels_last) if y is None else y
    if residual is not None and not residual.is_contiguous(memory_format=torch.channels_last):
        residual = residual.contiguous(memory_format=torch.channels_last)
    d = fill_mbse_desc(N.MbSeDesc(), pk, n, h, w, N.dtype_code(x), x.data_ptr(), t.data_ptr(), pool_partial.data_ptr(),
                       gate.data_ptr(), y.data_ptr(), residual.data_ptr() if residual is not None else None, stages)
    with torch.cuda.device(dev):
        rc = N.lib.ssdk_mbse(ctypes.byref(d), N.stream_ptr(dev))
    N.check(rc, "mbse")
    STATS["native_layers"] += 1
    return dict(t=t, pool_partial=pool_partial, gate=gate, y=y)


# ---- transposed 3x3 / stride 2 / pad 1 convolution (csrc/ssdk_convt.hip): the decoder step of the Shelf neck ----------------
def convt_class_taps(py, px):
    """Taps of output parity class (py, px) = (oy & 1, ox & 1) in image order: [(dy, dx, ky, kx)] -- tap dy * (1 + px) + dx reads
    input pixel (iy + dy, ix + dx) of output pixel (2 iy + py, 2 ix + px) through weight element [ky][kx] (oy = 2 iy - 1 + ky:
    an even row takes ky = 1; an odd row ky = 2 from iy and ky = 0 from iy + 1; columns alike)."""
    return [(dy, dx, 2 - 2 * dy if py else 1, 2 - 2 * dx if px else 1) for dy in range(1 + py) for dx in range(1 + px)]


def convt_parity_images(w):
    """``w``: ConvTranspose2d weight [Cin][Cout][3][3] -> the four parity images of include/ssdk_convt.h ``ssdk_convt_desc.w_pack``
    (class 2 py + px), each the fragment-major image [ceil(Cout / 16)][Kc / 32][4][16][8] of the matrix [Cout][Kc] with
    k = tap * Cin + ci and Kc = taps * Cin rounded up to 32 by zeros.  Pure layout, on the tensor's own device and dtype."""
    cin, cout, kh, kw = (int(v) for v in w.shape)
    assert kh == 3 and kw == 3, tuple(w.shape)
    g = (cout + 15) // 16
    images = []
    for py in (0, 1):
        for px in (0, 1):
            taps = convt_class_taps(py, px)
            kc = 32 * ((len(taps) * cin + 31) // 32)
            mat = w.new_zeros((g * 16, kc))
            for t, (_, _, ky, kx) in enumerate(taps):
                mat[:cout, t * cin:(t + 1) * cin] = w[:, :, ky, kx].t()
            images.append(mat.view(g, 16, kc // 32, 4, 8).permute(0, 2, 3, 1, 4).contiguous())
    return images


class ConvTPack(object):
    """``nn.ConvTranspose2d(Cin, Cout, 3, stride=2, padding=1)`` packed for ``ssdk_convt3x3s2``: the four parity images of the
    weight in the activation dtype, one behind the other, and the fp32 bias (None without one)."""

    __slots__ = ("w", "bias", "cin", "cout")

    @staticmethod
    def supported(m):
        """The host-side mirror of ssdk_convt3x3s2's argument checks (plus the module it is built from)."""
        return (isinstance(m, nn.ConvTranspose2d) and m.kernel_size == (3, 3) and m.stride == (2, 2) and m.padding == (1, 1)
                and m.output_padding == (0, 0) and m.dilation == (1, 1) and m.groups == 1
                and m.in_channels % 8 == 0 and m.out_channels % 8 == 0)

    def __init__(self, convt, dtype):
        if not ConvTPack.supported(convt):
            raise N.SsdkError("{} is not covered by ssdk_convt3x3s2".format(convt))
        self.cin, self.cout = convt.in_channels, convt.out_channels
        self.w = torch.cat([im.reshape(-1) for im in convt_parity_images(convt.weight.detach().to(dtype))]).contiguous()
        assert self.w.numel() * self.w.element_size() == N.lib.ssdk_convt_pack_bytes(self.cin, self.cout)
        self.bias = convt.bias.detach().float().contiguous() if convt.bias is not None else None


def fill_convt_desc(d, pk, n, h, w, dtype_code, x=None, y=None, skip=None, act="none"):
    d.x, d.w_pack, d.skip, d.y = x, pk.w.data_ptr(), skip, y
    d.bias = pk.bias.data_ptr() if pk.bias is not None else None
    d.N, d.Cin, d.H, d.W, d.Cout, d.act, d.dtype = n, pk.cin, h, w, pk.cout, N.ACT[act], dtype_code
    return d


def convt_native(x, pk, skip=None, act="none", y=None):
    """One ``ssdk_convt3x3s2`` call: channels_last x [N, Cin, H, W] -> channels_last [N, Cout, 2H - 1, 2W - 1] =
    act(conv_transpose2d(x) + bias) (+ skip)."""
    N.require_device(x, "convt3x3s2")
    if not x.is_contiguous(memory_format=torch.channels_last):
        x = x.contiguous(memory_format=torch.channels_last)
    n, c, h, w = (int(v) for v in x.shape)
    assert c == pk.cin, (c, pk.cin)
    if y is None:
        y = torch.empty((n,) + _out_shape("convt", pack=pk, h=h, w=w), device=x.device, dtype=x.dtype, memory_format=torch.channels_last)
    if skip is not None:
        assert tuple(skip.shape) == tuple(y.shape) and skip.dtype == x.dtype, (tuple(skip.shape), tuple(y.shape))
        if not skip.is_contiguous(memory_format=torch.channels_last):
            skip = skip.contiguous(memory_format=torch.channels_last)
    d = fill_convt_desc(N.ConvTDesc(), pk, n, h, w, N.dtype_code(x), x.data_ptr(), y.data_ptr(),
                        skip.data_ptr() if skip is not None else None, act)
    with torch.cuda.device(x.device):
        rc = N.lib.ssdk_convt3x3s2(ctypes.byref(d), N.stream_ptr(x.device))
    N.check(rc, "convt3x3s2")
    STATS["native_layers"] += 1
    return y


# ---- channel concatenation and SPP block (csrc/ssdk_cat.hip): the YOLO necks' two operations that are no convolution --------
def cat_supported(c1, c2, h, w, up2):
    """The host-side mirror of ssdk_cat2's argument checks -> None, or the reason it refuses."""
    if c1 < 8 or c2 < 8 or c1 % 8 or c2 % 8:
        return "channel counts {} + {} are not multiples of 8".format(c1, c2)
    if up2 and (h % 2 or w % 2):
        return "an upsampled source needs an even {}x{} output".format(h, w)
    return None


def _channels_last(t):
    return t if t.is_contiguous(memory_format=torch.channels_last) else t.contiguous(memory_format=torch.channels_last)


def cat_native(a, b, up2=False, y=None):
    """One ``ssdk_cat2`` call on channels_last tensors: ``torch.cat((a, b), 1)``, or with ``up2``
    ``torch.cat((a, F.interpolate(b, scale_factor=2)), 1)`` for ``b`` at half the size of ``a`` -- the same bits."""
    N.require_device(a, "cat2")
    a, b = _channels_last(a), _channels_last(b)
    n, c1, h, w = (int(v) for v in a.shape)
    c2 = int(b.shape[1])
    want = (n, c2, h // 2, w // 2) if up2 else (n, c2, h, w)
    if tuple(b.shape) != want or b.dtype != a.dtype or (up2 and (h % 2 or w % 2)):
        raise N.SsdkError("cat2: b is {} {}, expected {} {} next to a {}".format(tuple(b.shape), b.dtype, want, a.dtype, tuple(a.shape)))
    if y is None:
        y = torch.empty((n, c1 + c2, h, w), device=a.device, dtype=a.dtype, memory_format=torch.channels_last)
    d = N.CatDesc()
    d.a, d.b, d.y = a.data_ptr(), b.data_ptr(), y.data_ptr()
    d.N, d.H, d.W, d.C1, d.C2, d.mode, d.dtype = n, h, w, c1, c2, N.FUSE_UP2 if up2 else N.FUSE_SAME, N.dtype_code(a)
    with torch.cuda.device(a.device):
        rc = N.lib.ssdk_cat2(ctypes.byref(d), N.stream_ptr(a.device))
    N.check(rc, "cat2")
    STATS["native_layers"] += 1
    return y


def spp_native(x, y=None):
    """One ``ssdk_spp`` call on a channels_last tensor: ``torch.cat([x] + [F.max_pool2d(x, k, 1, k // 2) for k in (5, 9, 13)], 1)``
    -- the same bits."""
    N.require_device(x, "spp")
    x = _channels_last(x)
    n, c, h, w = (int(v) for v in x.shape)
    if y is None:
        y = torch.empty((n, 4 * c, h, w), device=x.device, dtype=x.dtype, memory_format=torch.channels_last)
    d = N.SppDesc()
    d.x, d.y = x.data_ptr(), y.data_ptr()
    d.N, d.H, d.W, d.C, d.dtype = n, h, w, c, N.dtype_code(x)
    with torch.cuda.device(x.device):
        rc = N.lib.ssdk_spp(ctypes.byref(d), N.stream_ptr(x.device))
    N.check(rc, "spp")
    STATS["native_layers"] += 1
    return y


def fill_mb_desc(d, x_ptr, y_ptr, n, h, w, pk, dtype_code):
    d.x, d.y = x_ptr, y_ptr
    d.w_expand, d.scale_expand, d.bias_expand = pk.e.w.data_ptr(), pk.e.scale.data_ptr(), pk.e.bias.data_ptr()
    d.w_dw, d.bias_dw = pk.wd.data_ptr(), pk.bd.data_ptr()
    d.w_project, d.scale_project, d.bias_project = pk.wp.data_ptr(), pk.p.scale.data_ptr(), pk.p.bias.data_ptr()
    d.N, d.H, d.W, d.Cin, d.Chid, d.Cout = n, h, w, pk.cin, pk.chid, pk.cout
    d.stride, d.residual, d.dtype, d.stem = pk.stride, int(pk.residual), dtype_code, pk.stem
    d.image_nw, d.w_image, d.w_image_bytes = 0, None, 0
    if w in (16, 32, 64) and not pk.stem:  # ssdk_mbk.hip: the blocks on 16- to 64-pixel-wide maps
        im = pk.image(w)
        if im is not None:
            d.image_nw, d.w_image, d.w_image_bytes = im[0], im[1].data_ptr(), im[1].numel() * 2
    return d


def xpair_supported(p1, p2, h, w):
    """An SSD extra layer (1x1 + BN + act, then 3x3 / stride 2 / pad 1 + BN + act) that csrc/ssdk_xpair.hip runs as one
    launch: small map, channel counts of its instances."""
    return (p1.kind == "dense" and p2.kind == "dense" and p1.k == 1 and p1.stride == 1 and p2.k == 3 and p2.stride == 2
            and p1.cout == p2.cin
            # exactly what ssdk_xpair() accepts: maps of <= 16 pixels (one fragment) or exactly 64 (four full fragments)
            and (h * w <= 16 or h * w == 64)
            and ((h * w + 15) // 16, p1.cin, p1.cout, p2.cout) in ((4, 512, 128, 256), (1, 256, 128, 256), (1, 256, 64, 128),
                                                                   (1, 128, 64, 128))
            and p1.act in ("none", "relu", "relu6") and p2.act in ("none", "relu", "relu6")
            and p1.scale is not None and p2.scale is not None and os.environ.get("SSDK_XPAIR", "1") != "0")


def fill_xpair_desc(d, x_ptr, y_ptr, n, h, w, p1, p2, dtype_code):
    d.x, d.y = x_ptr, y_ptr
    d.w1, d.scale1, d.bias1 = p1.w.data_ptr(), p1.scale.data_ptr(), p1.bias.data_ptr()
    d.w2, d.scale2, d.bias2 = p2.w.data_ptr(), p2.scale.data_ptr(), p2.bias.data_ptr()
    f1, f2 = p1.frag(), p2.frag()
    d.w1_frag, d.w2_frag = (f1.data_ptr(), f2.data_ptr()) if f1 is not None and f2 is not None else (None, None)
    d.N, d.H, d.W, d.Cin, d.Cmid, d.Cout = n, h, w, p1.cin, p1.cout, p2.cout
    d.act1, d.act2, d.dtype = N.ACT[p1.act], N.ACT[p2.act], dtype_code
    return d


def xpair_native(x, p1, p2, y=None):
    """Conv 1x1 + BN + act -> Conv 3x3 / stride 2 + BN + act on a small map in one launch; x channels_last (``y``: write
    there)."""
    N.require_device(x, "xpair")
    if not x.is_contiguous(memory_format=torch.channels_last):
        x = x.contiguous(memory_format=torch.channels_last)
    n, c, h, w = (int(v) for v in x.shape)
    y = _out_tensor(y, (n,) + _out_shape("xpair", pack2=p2, h=h, w=w), x, torch.channels_last, "xpair")
    d = fill_xpair_desc(N.XpairDesc(), x.data_ptr(), y.data_ptr(), n, h, w, p1, p2, N.dtype_code(x))
    with torch.cuda.device(x.device):
        rc = N.lib.ssdk_xpair(ctypes.byref(d), N.stream_ptr(x.device))
    N.check(rc, "xpair")
    STATS["native_layers"] += 2
    return y


# ---- DarkNet residual block (csrc/ssdk_dkres.hip): 1x1 + BN + act -> 3x3 + BN + act -> + x as one launch, the middle map in LDS ----
# Widths routed to the fused kernel when SSDK_DKRES is unset: those the probe (tools/dkres_probe.py) measured not slower
# than the two ssdk_conv launches at the shipped configs' batch-32 shapes.  SSDK_DKRES=1: every width ssdk_dkres_supported takes;
# SSDK_DKRES=0: none (every block is two launches).
DKRES_DEFAULT_WIDTHS = (64, 128, 256)


def dkres_supported(p1, p2, h, w, dtype_code=None):
    """A residual block (``p1``: 1x1, C -> C/2; ``p2``: 3x3 / stride 1, C/2 -> C; both dense with a folded BatchNorm and none / relu
    / relu6) that csrc/ssdk_dkres.hip runs as one launch.  The shapes are the C predicate's to decide (``ssdk_dkres_supported``);
    ``SSDK_DKRES`` (read at every call) narrows or widens the widths that are routed to it."""
    if not (p1.kind == "dense" and p2.kind == "dense" and p1.k == 1 and p1.stride == 1 and p2.k == 3 and p2.stride == 1
            and p1.cout == p2.cin and p2.cout == p1.cin and p1.cin == 2 * p1.cout
            and p1.act in ("none", "relu", "relu6") and p2.act in ("none", "relu", "relu6")
            and p1.scale is not None and p2.scale is not None and p1.w.dtype == p2.w.dtype):
        return False
    if dtype_code is None:
        dtype_code = N._DTYPES.get(p1.w.dtype, -1)
    if not N.lib.ssdk_dkres_supported(p1.cin, h, w, dtype_code):
        return False
    env = os.environ.get("SSDK_DKRES")
    if env is None:
        return p1.cin in DKRES_DEFAULT_WIDTHS
    return env != "0"


def fill_dkres_desc(d, x_ptr, y_ptr, n, h, w, p1, p2, dtype_code):
    """Fills an ``ssdk_dkres_desc`` -- or the ``ssdk_xpair_desc`` of an SSDK_OP_DKRES op (include/ssdk.h: Cin = Cout = C,
    Cmid = C / 2), whose other fields carry the same names."""
    d.x, d.y = x_ptr, y_ptr
    d.w1, d.scale1, d.bias1 = p1.w.data_ptr(), p1.scale.data_ptr(), p1.bias.data_ptr()
    d.w2, d.scale2, d.bias2 = p2.w.data_ptr(), p2.scale.data_ptr(), p2.bias.data_ptr()
    f1, f2 = p1.frag(), p2.frag()
    d.w1_frag, d.w2_frag = (f1.data_ptr(), f2.data_ptr()) if f1 is not None and f2 is not None else (None, None)
    d.N, d.H, d.W = n, h, w
    if isinstance(d, N.XpairDesc):
        d.Cin, d.Cmid, d.Cout = p1.cin, p1.cout, p2.cout
    else:
        d.C = p1.cin
    d.act1, d.act2, d.dtype = N.ACT[p1.act], N.ACT[p2.act], dtype_code
    return d


def dkres_native(x, p1, p2, y=None):
    """``x + act2(bn2(conv3x3(act1(bn1(conv1x1(x))))))`` in one launch; x channels_last (``y``: write there; never ``x`` itself --
    a workgroup reads its neighbours' ``x``)."""
    N.require_device(x, "dkres")
    x = _channels_last(x)
    n, c, h, w = (int(v) for v in x.shape)
    y = _out_tensor(y, (n, c, h, w), x, torch.channels_last, "dkres")
    d = fill_dkres_desc(N.DkresDesc(), x.data_ptr(), y.data_ptr(), n, h, w, p1, p2, N.dtype_code(x))
    with torch.cuda.device(x.device):
        rc = N.lib.ssdk_dkres(ctypes.byref(d), N.stream_ptr(x.device))
    N.check(rc, "dkres")
    STATS["native_layers"] += 2
    return y


# ---- DenseNet dense layer (csrc/ssdk_denselayer.hip): BN + ReLU -> 1x1 -> BN + ReLU -> 3x3 as one launch that reads channels [0, Cin)
# of its block's buffer and writes [Cin, Cin + 32) -- no concatenation, the 128-channel middle map in LDS.
def denselayer_enabled():
    """SSDK_DENSELAYER (read whenever a plan is recorded): 0 sends a DenseNet backbone back to PyTorch-ROCm (docs/SWITCHES.md)."""
    return os.environ.get("SSDK_DENSELAYER", "1") != "0"


def fold_norm(bn):
    """-> (a[C], b[C]) fp32 such that bn(x) == a * x + b in eval mode."""
    var, mean = bn.running_var.detach().float(), bn.running_mean.detach().float()
    gamma = bn.weight.detach().float() if bn.affine else torch.ones_like(var)
    beta = bn.bias.detach().float() if bn.affine else torch.zeros_like(var)
    a = gamma / torch.sqrt(var + bn.eps)
    return a.contiguous(), (beta - mean * a).contiguous()


class DenseLayerPack(object):
    """One ``_DenseLayer`` (nets/densenet.py) packed for ``ssdk_dense_layer``: norm1 folded into the fp32 pair (a, b) that the
    kernel applies to x on its way into the MFMA operand, norm2 folded into (scale1, bias1) behind the 1x1, both weight tensors
    KRSC in 16 bits with their fragment-major images (``ssdk_weight_frag_bytes``; None with SSDK_WFRAG=0)."""

    __slots__ = ("a", "b", "w1", "scale1", "bias1", "w2", "w1_frag", "w2_frag", "cin", "cmid", "cout")

    @staticmethod
    def unsupported(layer):
        """None, or why ``layer`` is not the layer the kernel computes."""
        c1, c2 = getattr(layer, "conv1", None), getattr(layer, "conv2", None)
        n1, n2 = getattr(layer, "norm1", None), getattr(layer, "norm2", None)
        if not (isinstance(c1, nn.Conv2d) and isinstance(c2, nn.Conv2d) and isinstance(n1, nn.BatchNorm2d) and isinstance(n2, nn.BatchNorm2d)
                and isinstance(getattr(layer, "relu1", None), nn.ReLU) and isinstance(getattr(layer, "relu2", None), nn.ReLU)):
            return "norm1, relu1, conv1, norm2, relu2, conv2 (BatchNorm2d, ReLU, Conv2d) expected"
        if (c1.kernel_size != (1, 1) or c1.stride != (1, 1) or c1.padding != (0, 0) or c1.groups != 1 or c1.bias is not None
                or c2.kernel_size != (3, 3) or c2.stride != (1, 1) or c2.padding != (1, 1) or c2.dilation != (1, 1) or c2.groups != 1
                or c2.bias is not None or c2.in_channels != c1.out_channels or n1.num_features != c1.in_channels
                or n2.num_features != c1.out_channels):
            return "a bias-free 1x1 then a bias-free 3x3 / stride 1 / pad 1 expected"
        if c1.out_channels != N.DENSE_CMID or c2.out_channels != N.DENSE_COUT:
            return "bn_size * growth = {} middle and growth = {} output channels (the kernel has {} and {})".format(
                c1.out_channels, c2.out_channels, N.DENSE_CMID, N.DENSE_COUT)
        return None

    def __init__(self, layer, dtype):
        why = DenseLayerPack.unsupported(layer)
        if why is not None:
            raise N.SsdkError("dense layer: " + why)
        self.cin, self.cmid, self.cout = layer.conv1.in_channels, layer.conv1.out_channels, layer.conv2.out_channels
        self.a, self.b = fold_norm(layer.norm1)
        self.scale1, self.bias1 = fold_norm(layer.norm2)
        self.w1 = layer.conv1.weight.detach().float().reshape(self.cmid, self.cin).contiguous().to(dtype)
        self.w2 = layer.conv2.weight.detach().float().permute(0, 2, 3, 1).contiguous().to(dtype)  # [32][3][3][128]
        self.w1_frag = self.w2_frag = None
        if USE_WFRAG:
            self.w1_frag = _frag_image(self.w1, self.cmid, self.cin)
            self.w2_frag = _frag_image(self.w2.reshape(self.cout, 9 * self.cmid), self.cout, 9 * self.cmid)


def _frag_image(w2d, rows, k_elems):
    """Fragment-major image of a [rows][K] matrix (ConvPack.frag's layout): [rows / 16][K / 32][4][16][8]."""
    assert rows % 16 == 0 and k_elems % 32 == 0, (rows, k_elems)
    img = w2d.view(rows // 16, 16, k_elems // 32, 4, 8).permute(0, 2, 3, 1, 4).contiguous()
    assert img.numel() * 2 == N.lib.ssdk_weight_frag_bytes(rows, k_elems)
    return img


def fill_dense_desc(d, x_ptr, n, h, w, cin, ld, pk, dtype_code, es=2):
    """Fills an ``ssdk_dense_layer_desc`` -- or the ``ssdk_xpair_desc`` of an SSDK_OP_DENSE op (include/ssdk.h: scale2 / bias2 carry
    (a, b), pad carries ld).  ``x_ptr``: channel 0 of pixel 0 of the block's buffer; y is ``cin`` channels behind it."""
    assert cin == pk.cin, (cin, pk.cin)
    d.x, d.y = x_ptr, x_ptr + cin * es
    d.w1, d.scale1, d.bias1, d.w2 = pk.w1.data_ptr(), pk.scale1.data_ptr(), pk.bias1.data_ptr(), pk.w2.data_ptr()
    d.w1_frag, d.w2_frag = (pk.w1_frag.data_ptr(), pk.w2_frag.data_ptr()) if pk.w1_frag is not None else (None, None)
    d.N, d.H, d.W, d.Cin, d.dtype = n, h, w, cin, dtype_code
    if isinstance(d, N.XpairDesc):
        d.scale2, d.bias2, d.pad = pk.a.data_ptr(), pk.b.data_ptr(), ld
        d.Cmid, d.Cout, d.act1, d.act2 = pk.cmid, pk.cout, N.ACT["relu"], N.ACT["none"]
    else:
        d.a, d.b, d.ld = pk.a.data_ptr(), pk.b.data_ptr(), ld
    return d


def _dense_buffer(buf, what):
    """(n, h, w, ld) of a block buffer: a contiguous [N][H][W][ld] tensor in 16 bits on a HIP device."""
    N.require_device(buf, what)
    if buf.dim() != 4 or not buf.is_contiguous():
        raise N.SsdkError("{}: the block buffer is a contiguous [N][H][W][ld] tensor, got {} with strides {}".format(
            what, tuple(buf.shape), tuple(buf.stride())))
    return tuple(int(v) for v in buf.shape)


def dense_layer_native(buf, pk):
    """One dense layer in place: reads ``buf[..., :pk.cin]`` and writes ``buf[..., pk.cin : pk.cin + 32]`` (``buf``: [N][H][W][ld])."""
    n, h, w, ld = _dense_buffer(buf, "dense_layer")
    d = fill_dense_desc(N.DenseLayerDesc(), buf.data_ptr(), n, h, w, pk.cin, ld, pk, N.dtype_code(buf))
    with torch.cuda.device(buf.device):
        rc = N.lib.ssdk_dense_layer(ctypes.byref(d), N.stream_ptr(buf.device))
    N.check(rc, "dense_layer")
    STATS["native_layers"] += 2
    return buf


def dense_pool_native(buf, c, a, b, y=None):
    """avgpool2x2(relu(a * buf[..., :c] + b)) -> channels_last [N, c, H/2, W/2] (``y``: write there)."""
    n, h, w, ld = _dense_buffer(buf, "dense_pool")
    y = _out_tensor(y, (n,) + _out_shape("densepool", ch=c, h=h, w=w), buf, torch.channels_last, "dense_pool")
    d = N.DensePoolDesc()
    d.x, d.y, d.a, d.b = buf.data_ptr(), y.data_ptr(), a.data_ptr(), b.data_ptr()
    d.N, d.H, d.W, d.C, d.ld, d.dtype = n, h, w, c, ld, N.dtype_code(buf)
    with torch.cuda.device(buf.device):
        rc = N.lib.ssdk_dense_pool(ctypes.byref(d), N.stream_ptr(buf.device))
    N.check(rc, "dense_pool")
    STATS["native_layers"] += 1
    return y


def dense_place_native(x, buf):
    """Copies channels_last ``x`` [N, C, H, W] into ``buf[..., :C]`` (``buf``: [N][H][W][ld]); the other channels stay."""
    n, h, w, ld = _dense_buffer(buf, "dense_place")
    x = _channels_last(x)
    if tuple(x.shape) != (n, x.shape[1], h, w) or x.dtype != buf.dtype:
        raise N.SsdkError("dense_place: x is {} {}, the buffer {} {}".format(tuple(x.shape), x.dtype, tuple(buf.shape), buf.dtype))
    d = N.DensePlaceDesc()
    d.x, d.y = x.data_ptr(), buf.data_ptr()
    d.N, d.H, d.W, d.C, d.ld, d.dtype = n, h, w, int(x.shape[1]), ld, N.dtype_code(buf)
    with torch.cuda.device(buf.device):
        rc = N.lib.ssdk_dense_place(ctypes.byref(d), N.stream_ptr(buf.device))
    N.check(rc, "dense_place")
    STATS["native_layers"] += 1
    return buf


# ---- ShuffleNetV2 unit (csrc/ssdk_shuffle.hip): chunk / branch2 (/ branch1) / cat / channel shuffle as one launch that reads x once
# and writes the interleaved y once.  Tensors are dense NHWC [N][H][W][Cp], Cp = pad8(C): padding channels are never read and are
# written as zeros.
def shuffleunit_enabled():
    """SSDK_SHUFFLEUNIT (read whenever a plan is recorded): 0 sends a ShuffleNetV2 backbone back to PyTorch-ROCm (docs/SWITCHES.md)."""
    return os.environ.get("SSDK_SHUFFLEUNIT", SHUFFLEUNIT_DEFAULT) != "0"


SHUFFLEUNIT_DEFAULT = "1"  # the plan's slowest forward beats the module path's fastest on both configs


def shuffle_pad(cb):
    """Width the weight images and vectors of a branch of ``cb`` channels are zero-padded to (include/ssdk_shuffle.h)."""
    return (cb + N.SHUFFLE_CHUNK - 1) // N.SHUFFLE_CHUNK * N.SHUFFLE_CHUNK


def _zero_padded(t, shape):
    out = t.new_zeros(shape)
    out[tuple(slice(0, d) for d in t.shape)] = t
    return out.contiguous()


def _shuffle_pw(conv, rows, cols, dtype):
    """1x1 conv -> (zero-padded [rows][cols] matrix in ``dtype``, its fragment-major image)."""
    w = conv.weight.detach().float().reshape(conv.out_channels, conv.in_channels).to(dtype)
    w = _zero_padded(w, (rows, cols))
    return w, _frag_image(w, rows, cols)


def _shuffle_dw(conv, cols, dtype):
    """depthwise 3x3 [C, 1, 3, 3] -> [9 taps][cols] in ``dtype``, zeros behind the C real channels."""
    w = conv.weight.detach().float()[:, 0].permute(1, 2, 0).reshape(9, conv.out_channels).to(dtype)
    return _zero_padded(w, (9, cols))


def _shuffle_affine(bn, cols):
    """-> fp32 [2][cols]: the folded scale, then the folded bias, zeros in the padding (one tensor: an executor op has ONE member
    for the depthwise's constants, include/ssdk.h SSDK_OP_SHUFFLE)."""
    a, b = fold_norm(bn)
    return _zero_padded(torch.stack([a, b]), (2, cols))


def _branch_why(seq, kinds, what):
    mods = list(seq.children())
    if len(mods) != len(kinds) or not all(isinstance(m, k) for m, k in zip(mods, kinds)):
        return "{}: {} expected, got {}".format(what, ", ".join(k.__name__ for k in kinds), ", ".join(type(m).__name__ for m in mods))
    return None


def _pw_why(conv, cin, cout, what):
    if (conv.kernel_size != (1, 1) or conv.stride != (1, 1) or conv.padding != (0, 0) or conv.groups != 1 or conv.bias is not None
            or conv.in_channels != cin or conv.out_channels != cout):
        return "{}: a bias-free 1x1 {} -> {} expected, got {}".format(what, cin, cout, conv)
    return None


def _dw_why(conv, c, stride, what):
    if (conv.kernel_size != (3, 3) or conv.stride != (stride, stride) or conv.padding != (1, 1) or conv.dilation != (1, 1)
            or conv.groups != c or conv.in_channels != c or conv.out_channels != c or conv.bias is not None
            or conv.padding_mode != "zeros"):
        return "{}: a bias-free depthwise 3x3 / stride {} / pad 1 on {} channels expected, got {}".format(what, stride, c, conv)
    return None


_BRANCH2 = (nn.Conv2d, nn.BatchNorm2d, nn.ReLU, nn.Conv2d, nn.BatchNorm2d, nn.Conv2d, nn.BatchNorm2d, nn.ReLU)
_BRANCH1 = (nn.Conv2d, nn.BatchNorm2d, nn.Conv2d, nn.BatchNorm2d, nn.ReLU)


def _shuffle_unit_why(unit, stride):
    b1, b2 = getattr(unit, "branch1", None), getattr(unit, "branch2", None)
    if not isinstance(b1, nn.Sequential) or not isinstance(b2, nn.Sequential) or getattr(unit, "stride", None) != stride:
        return "a stride-{} unit with branch1 and branch2 (Sequential) expected, got {}".format(stride, type(unit).__name__)
    why = _branch_why(b2, _BRANCH2, "branch2")
    if why:
        return why
    cb = b2[5].out_channels
    cin = b2[0].in_channels
    if stride == 1:
        if len(b1) != 0:
            return "branch1 of a stride-1 unit is empty"
        if cin != cb:
            return "branch2 of a stride-1 unit maps Cb -> Cb, got {} -> {}".format(cin, cb)
    else:
        why = (_branch_why(b1, _BRANCH1, "branch1") or _dw_why(b1[0], cin, 2, "branch1.0") or _pw_why(b1[2], cin, cb, "branch1.2"))
        if why:
            return why
        if b1[1].num_features != cin or b1[3].num_features != cb:
            return "branch1: BatchNorm widths {} / {} for {} -> {} channels".format(b1[1].num_features, b1[3].num_features, cin, cb)
    why = _pw_why(b2[0], cin, cb, "branch2.0") or _dw_why(b2[3], cb, stride, "branch2.3") or _pw_why(b2[5], cb, cb, "branch2.5")
    if why:
        return why
    if any(b2[i].num_features != cb for i in (1, 4, 6)):
        return "branch2: a BatchNorm that is not {} wide".format(cb)
    return None


class ShuffleUnitPack(object):
    """One stride-1 ``InvertedResidual`` (nets/shufflenet.py) packed for ``ssdk_shuffle_unit``: branch2's three weight sets, every
    BatchNorm folded into an fp32 (scale, bias) pair that the kernel applies in fp32; 16-bit weights, zero-padded to
    ``p = shuffle_pad(cb)`` rows and K columns (``w1`` / ``w3``: the padded matrices, ``w1_img`` / ``w3_img``: their fragment-major
    images, which are what the kernel reads); ``affine2`` = fp32 [2][p], ``scale2`` / ``bias2`` its rows."""

    __slots__ = ("cb", "p", "w1", "w1_img", "scale1", "bias1", "wd", "affine2", "scale2", "bias2", "w3", "w3_img", "scale3", "bias3")
    stride = 1

    @staticmethod
    def unsupported(unit):
        """None, or why ``unit`` is not the unit the kernel computes."""
        why = _shuffle_unit_why(unit, 1)
        if why is None and not N.lib.ssdk_shuffle_unit_supported(unit.branch2[5].out_channels, 1, 1, N.BF16):
            why = "ssdk_shuffle_unit_supported refuses Cb = {}".format(unit.branch2[5].out_channels)
        return why

    def __init__(self, unit, dtype):
        why = type(self).unsupported(unit)
        if why is not None:
            raise N.SsdkError("shuffle unit: " + why)
        self._pack_branch2(unit.branch2, dtype)

    def _pack_branch2(self, b2, dtype, kp=None):
        self.cb = b2[5].out_channels
        self.p = shuffle_pad(self.cb)
        self.w1, self.w1_img = _shuffle_pw(b2[0], self.p, self.p if kp is None else kp, dtype)
        self.scale1, self.bias1 = _shuffle_affine(b2[1], self.p)
        self.wd = _shuffle_dw(b2[3], self.p, dtype)
        self.affine2 = _shuffle_affine(b2[4], self.p)
        self.scale2, self.bias2 = self.affine2[0], self.affine2[1]
        self.w3, self.w3_img = _shuffle_pw(b2[5], self.p, self.p, dtype)
        self.scale3, self.bias3 = _shuffle_affine(b2[6], self.p)


class ShuffleDownPack(ShuffleUnitPack):
    """One stride-2 ``InvertedResidual`` packed for ``ssdk_shuffle_down``: branch2 as in ``ShuffleUnitPack`` (its first 1x1 reads
    all ``cin`` input channels: K padded to ``kp`` = 32 ceil(cin / 32)) plus branch1's depthwise (``b1_wd`` [9][kp], ``b1_scale1`` /
    ``b1_bias1`` fp32 [kp]) and 1x1 (``b1_w2`` [p][kp] with its image, ``b1_scale2`` / ``b1_bias2`` fp32 [p])."""

    __slots__ = ("cin", "kp", "b1_wd", "b1_scale1", "b1_bias1", "b1_w2", "b1_w2_img", "b1_scale2", "b1_bias2")
    stride = 2

    @staticmethod
    def unsupported(unit):
        why = _shuffle_unit_why(unit, 2)
        if why is None and not N.lib.ssdk_shuffle_down_supported(unit.branch2[0].in_channels, unit.branch2[5].out_channels, 1, 1, N.BF16):
            why = "ssdk_shuffle_down_supported refuses Cin = {}, Cb = {}".format(unit.branch2[0].in_channels,
                                                                                unit.branch2[5].out_channels)
        return why

    def __init__(self, unit, dtype):
        why = type(self).unsupported(unit)
        if why is not None:
            raise N.SsdkError("shuffle unit: " + why)
        self.cin = unit.branch2[0].in_channels
        self.kp = (self.cin + 31) // 32 * 32
        self._pack_branch2(unit.branch2, dtype, kp=self.kp)
        b1 = unit.branch1
        self.b1_wd = _shuffle_dw(b1[0], self.kp, dtype)
        self.b1_scale1, self.b1_bias1 = _shuffle_affine(b1[1], self.kp)
        self.b1_w2, self.b1_w2_img = _shuffle_pw(b1[2], self.p, self.kp, dtype)
        self.b1_scale2, self.b1_bias2 = _shuffle_affine(b1[3], self.p)


def fill_shuffle_desc(d, x_ptr, y_ptr, n, h, w, pk, dtype_code, ld_in=0):
    """Fills an ``ssdk_shuffle_unit_desc`` / ``ssdk_shuffle_down_desc`` -- or the ``mb`` (+ ``xpair``) members of an executor op
    (include/ssdk.h SSDK_OP_SHUFFLE / SSDK_OP_SHUFFLEDOWN) -- from a ``ShuffleUnitPack`` / ``ShuffleDownPack``."""
    down = pk.stride == 2
    if isinstance(d, N.Op):
        m = d.mb
        m.x, m.y = x_ptr, y_ptr
        m.w_expand, m.scale_expand, m.bias_expand = pk.w1_img.data_ptr(), pk.scale1.data_ptr(), pk.bias1.data_ptr()
        m.w_dw, m.bias_dw = pk.wd.data_ptr(), pk.affine2.data_ptr()
        m.w_project, m.scale_project, m.bias_project = pk.w3_img.data_ptr(), pk.scale3.data_ptr(), pk.bias3.data_ptr()
        m.N, m.H, m.W, m.Chid, m.Cout, m.stride, m.dtype = n, h, w, pk.cb, 2 * pk.cb, pk.stride, dtype_code
        m.Cin = pk.cin if down else 2 * pk.cb
        if down:
            b = d.xpair
            b.w1, b.scale1, b.bias1 = pk.b1_wd.data_ptr(), pk.b1_scale1.data_ptr(), pk.b1_bias1.data_ptr()
            b.w2_frag, b.scale2, b.bias2 = pk.b1_w2_img.data_ptr(), pk.b1_scale2.data_ptr(), pk.b1_bias2.data_ptr()
            b.Cin, b.Cmid, b.Cout, b.act1, b.act2, b.pad, b.dtype = pk.cin, pk.cin, pk.cb, N.ACT["none"], N.ACT["relu"], ld_in, dtype_code
            b.N, b.H, b.W = n, h, w
        return d
    d.x, d.y = x_ptr, y_ptr
    d.w1, d.scale1, d.bias1 = pk.w1_img.data_ptr(), pk.scale1.data_ptr(), pk.bias1.data_ptr()
    d.wd, d.scale2, d.bias2 = pk.wd.data_ptr(), pk.scale2.data_ptr(), pk.bias2.data_ptr()
    d.w3, d.scale3, d.bias3 = pk.w3_img.data_ptr(), pk.scale3.data_ptr(), pk.bias3.data_ptr()
    d.N, d.H, d.W, d.Cb, d.dtype = n, h, w, pk.cb, dtype_code
    if down:
        d.b1_wd, d.b1_scale1, d.b1_bias1 = pk.b1_wd.data_ptr(), pk.b1_scale1.data_ptr(), pk.b1_bias1.data_ptr()
        d.b1_w2, d.b1_scale2, d.b1_bias2 = pk.b1_w2_img.data_ptr(), pk.b1_scale2.data_ptr(), pk.b1_bias2.data_ptr()
        d.Cin, d.ld_in = pk.cin, ld_in
    return d


def _nhwc(x, what):
    """(n, h, w, c) of a dense NHWC tensor [N][H][W][C] in 16 bits on a HIP device."""
    N.require_device(x, what)
    if x.dim() != 4 or not x.is_contiguous():
        raise N.SsdkError("{}: a contiguous [N][H][W][C] tensor expected, got {} with strides {}".format(
            what, tuple(x.shape), tuple(x.stride())))
    return tuple(int(v) for v in x.shape)


def shuffle_unit_native(x, pk, y=None):
    """One stride-1 unit: ``x`` [N][H][W][Cp], Cp = pad8(2 cb), of which channels [0, 2 cb) are read -> ``y`` of the same shape, zeros
    in [2 cb, Cp) (``y``: write there)."""
    n, h, w, c = _nhwc(x, "shuffle_unit")
    if c != pad8(2 * pk.cb):
        raise N.SsdkError("shuffle_unit: x has {} channels per pixel, a unit of Cb = {} reads {}".format(c, pk.cb, pad8(2 * pk.cb)))
    y = _out_tensor(y, (n, h, w, c), x, torch.contiguous_format, "shuffle_unit")
    d = fill_shuffle_desc(N.ShuffleUnitDesc(), x.data_ptr(), y.data_ptr(), n, h, w, pk, N.dtype_code(x))
    with torch.cuda.device(x.device):
        rc = N.lib.ssdk_shuffle_unit(ctypes.byref(d), N.stream_ptr(x.device))
    N.check(rc, "shuffle_unit")
    STATS["native_layers"] += 3
    return y


def shuffle_down_native(x, pk, y=None):
    """One stride-2 unit: ``x`` [N][H][W][ld], ld a multiple of 8 and >= cin, of which channels [0, cin) are read -> ``y``
    [N][Ho][Wo][pad8(2 cb)], Ho = (H - 1) / 2 + 1 (``y``: write there)."""
    n, h, w, ld = _nhwc(x, "shuffle_down")
    if ld < pk.cin or ld % 8:
        raise N.SsdkError("shuffle_down: x has {} channels per pixel, a unit of Cin = {} needs a multiple of 8 >= Cin".format(ld, pk.cin))
    cp, ho, wo = _out_shape("shuffledown", pack=pk, h=h, w=w)
    y = _out_tensor(y, (n, ho, wo, cp), x, torch.contiguous_format, "shuffle_down")
    d = fill_shuffle_desc(N.ShuffleDownDesc(), x.data_ptr(), y.data_ptr(), n, h, w, pk, N.dtype_code(x), ld_in=ld)
    with torch.cuda.device(x.device):
        rc = N.lib.ssdk_shuffle_down(ctypes.byref(d), N.stream_ptr(x.device))
    N.check(rc, "shuffle_down")
    STATS["native_layers"] += 5
    return y


def fill_fuse_desc(d, a_ptr, b_ptr, c_ptr, y_ptr, n, h, w, ch, weights, mode_b, mode_c, hw_b, hw_c, dtype_code):
    """``hw_b`` / ``hw_c``: (height, width) of the sources b and c (``hw_c`` None without a third source)."""
    d.a, d.b, d.c, d.y = a_ptr, b_ptr, c_ptr, y_ptr
    d.w0, d.w1, d.w2 = (float(v) for v in weights)
    d.mode_b, d.mode_c = mode_b, mode_c
    d.N, d.H, d.W, d.C = n, h, w, ch
    d.hb, d.wb = (int(v) for v in hw_b)
    if hw_c is not None:
        d.hc, d.wc = (int(v) for v in hw_c)
    d.dtype = dtype_code
    return d


def fuse_native(a, b, c=None, weights=(1.0, 1.0, 0.0), mode_b=N.FUSE_SAME, mode_c=N.FUSE_SAME, y=None):
    """y = w0*a + w1*R_b(b) [+ w2*R_c(c)] (BiFPN weighted fusion, csrc/ssdk_fuse.hip); channels_last tensors (``y``: write
    there)."""
    N.require_device(a, "fuse")
    ts = [t if t is None or t.is_contiguous(memory_format=torch.channels_last) else
          t.contiguous(memory_format=torch.channels_last) for t in (a, b, c)]
    a, b, c = ts
    n, ch, h, w = (int(v) for v in a.shape)
    y = _out_tensor(y, (n, ch, h, w), a, torch.channels_last, "fuse")
    d = fill_fuse_desc(N.FuseDesc(), a.data_ptr(), b.data_ptr(), c.data_ptr() if c is not None else None, y.data_ptr(), n, h, w, ch,
                       weights, mode_b, mode_c, tuple(b.shape[2:]), tuple(c.shape[2:]) if c is not None else None, N.dtype_code(a))
    with torch.cuda.device(a.device):
        rc = N.lib.ssdk_fuse(ctypes.byref(d), N.stream_ptr(a.device))
    N.check(rc, "fuse")
    return y


def mbconv_native(x, pk, variant=0, y=None):
    """One fused inverted-residual block; x channels_last [N,Cin,H,W] -> channels_last [N,Cout,Ho,Wo] (``y``: write there).
    ``variant``: 0 automatic, 1 register-flow kernel wherever it exists, -1 LDS-tiled kernel only (ssdk_mbconv_desc)."""
    N.require_device(x, "mbconv")
    stem = pk.stem
    if stem and x.is_contiguous():
        stem = 1  # NCHW image
    else:
        if not x.is_contiguous(memory_format=torch.channels_last):
            x = x.contiguous(memory_format=torch.channels_last)
        stem = 2 if stem else 0
    n, c, h, w = (int(v) for v in x.shape)
    y = _out_tensor(y, (n,) + _out_shape("mb", pack=pk, h=h, w=w), x, torch.channels_last, "mbconv")
    d = fill_mb_desc(N.MbConvDesc(), x.data_ptr(), y.data_ptr(), n, h, w, pk, N.dtype_code(x))
    d.stem = stem
    d.variant = int(variant)
    with torch.cuda.device(x.device):
        rc = N.lib.ssdk_mbconv(ctypes.byref(d), N.stream_ptr(x.device))
    N.check(rc, "mbconv")
    STATS["native_layers"] += 1
    return y


def conv_res_mode(pack, res_mode=0):
    """ssdk_conv_desc.res_mode of a layer: the caller's two bits, and bits 8-11 = dilation - 1 (include/ssdk_dconv.h)."""
    return (res_mode & 3) | (((getattr(pack, "dilation", 1) - 1) << N.CONV_DILATION_SHIFT) & N.CONV_DILATION_MASK)


def _out_hw(h, w, k, stride):  # (a 'dilated' layer is k 3 / stride 1 with padding = dilation: the map keeps its size, as here)
    pad = k // 2
    return (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1


def wants_frag(pack, h, w, has_residual, in_layout=N.NHWC):
    """Whether one of the kernels that read the fragment-major weight image can take this layer -- the host-side mirror of the
    C dispatch (csrc/ssdk_smallmap.hip launch_conv_smallmap: 3x3 on maps of <= 64 output pixels, stride 1 | 2;
    csrc/ssdk_conv3x3s.hip launch_conv3x3_short: 3x3 / stride 1, NHWC input, Cin a multiple of 32 up to 128 -- or 256 on maps
    of <= 2500 pixels --, Cout >= 96, no residual, a map of >= 128 pixels and >= 8 columns).  Everything else (the ResNet /
    RegNet backbone 3x3s, the 80x80 tower layers) stays on kernels that read the KRSC tensor and carries no second copy."""
    if pack.kind != "dense" or pack.k != 3:
        return False
    ho, wo = _out_hw(h, w, pack.k, pack.stride)
    if ho * wo <= 64:  # conv_smallmap_kernel (stride 2: the first SSD extra, 16x16 -> 8x8)
        return True
    if pack.stride != 1 or has_residual or in_layout != N.NHWC:
        return False
    short_k = pack.cin % 32 == 0 and (pack.cin <= 128 or (pack.cin == 256 and h * w <= 2500))
    return short_k and pack.cout >= 96 and h * w >= 128 and w >= 8


def fill_desc(d, x_ptr, n, h, w, pack, dtype_code, act, y_ptr, in_layout=N.NHWC, out_layout=N.NHWC,
              residual_ptr=None, y2_ptr=None, split=None, act2=None):
    d.x, d.w = x_ptr, pack.w.data_ptr()
    if pack.kind == "gany":  # not optional: gconv3x3_any_kernel reads nothing else
        frag = pack.gfrag()
    elif pack.kind == "dilated":  # not optional either: dconv3x3_kernel
        frag = pack.dfrag()
    else:
        frag = pack.frag() if wants_frag(pack, h, w, residual_ptr is not None, in_layout) else None
    d.w_frag = frag.data_ptr() if frag is not None else None
    d.scale = pack.scale.data_ptr() if pack.scale is not None else None
    d.bias = pack.bias.data_ptr()
    d.residual, d.y, d.y2 = residual_ptr, y_ptr, y2_ptr
    d.N, d.Cin, d.H, d.W, d.Cout = n, pack.cin, h, w, pack.cout
    d.k, d.stride, d.groups = pack.k, pack.stride, pack.groups
    d.act = N.ACT[act]
    d.act2 = N.ACT[act2 if act2 is not None else act]
    d.split = split if split is not None else pack.cout
    d.dtype, d.in_layout, d.out_layout = dtype_code, in_layout, out_layout
    d.res_mode = conv_res_mode(pack)
    return d


def conv_native(x, pack, act=None, residual=None, nchw_out=False, split=None, act2=None, res_mode=0, y=None, y2=None):
    """One fused layer.  x: [N,C,H,W] tensor in channels_last memory (converted if not; the stem also takes
    plain NCHW).  Returns a channels_last tensor, or NCHW tensor(s) when ``nchw_out`` (heads).  ``y`` (and ``y2`` for the
    second part of a ``split`` head): the caller's own output buffers instead of fresh ones."""
    N.require_device(x, "conv")
    act = pack.act if act is None else act
    n, c, h, w = (int(v) for v in x.shape)
    in_layout = N.NHWC
    if pack.kind == "stem" and x.is_contiguous():
        in_layout = N.NCHW
    elif not x.is_contiguous(memory_format=torch.channels_last):
        x = x.contiguous(memory_format=torch.channels_last)
    _, ho, wo = _out_shape(None, pack=pack, h=h, w=w)
    if y2 is not None and not (nchw_out and split is not None):
        raise N.SsdkError("conv: y2 is the second output of a split NCHW head; this call has none")
    if nchw_out:
        if split is not None:
            y = _out_tensor(y, (n, split, ho, wo), x, torch.contiguous_format, "conv")
            y2 = _out_tensor(y2, (n, pack.cout - split, ho, wo), x, torch.contiguous_format, "conv (y2)")
        else:
            y = _out_tensor(y, (n, pack.cout, ho, wo), x, torch.contiguous_format, "conv")
    else:
        y = _out_tensor(y, (n, pack.cout, ho, wo), x, torch.channels_last, "conv")
    if residual is not None and not residual.is_contiguous(memory_format=torch.channels_last):
        residual = residual.contiguous(memory_format=torch.channels_last)
    d = fill_desc(N.ConvDesc(), x.data_ptr(), n, h, w, pack, N.dtype_code(x), act, y.data_ptr(), in_layout,
                  N.NCHW if nchw_out else N.NHWC, residual.data_ptr() if residual is not None else None,
                  y2.data_ptr() if y2 is not None else None, split, act2)
    d.res_mode = conv_res_mode(pack, res_mode)
    with torch.cuda.device(x.device):
        need = int(N.lib.ssdk_conv_workspace_bytes(n, pack.cin, h, w, pack.cout, pack.k, pack.stride, N.dtype_code(x)))
        if need:
            ws = N.scratch(x.device, "splitk", need + 256)  # (+ 256: the kernels take it 256-byte aligned)
            wptr = (ws.data_ptr() + 255) & ~255
            rc = N.lib.ssdk_conv(ctypes.byref(d), wptr, ws.numel() - (wptr - ws.data_ptr()), N.stream_ptr(x.device))
        else:
            rc = N.lib.ssdk_conv(ctypes.byref(d), None, 0, N.stream_ptr(x.device))
    N.check(rc, "conv")
    STATS["native_layers"] += 1
    return (y, y2) if y2 is not None else y


# ---- the plan's op kinds: ONE definition each of the executor's op code, the output geometry, the descriptor fill and the table row.
# ``out(L)`` -> (c, ho, wo), the output's shape from the layer dict alone (what the record methods allocate and the ``*_native``
# wrappers return); ``fill(plan, i, L, op)`` fills ``plan.ops[i]`` (a source that is an external input goes through ``plan._ptr``,
# which notes the patch); ``row(L, es)`` -> dict(name, flops = 2 * MAC, bytes = algorithmic HBM traffic, kind) of ``layer_table()``.
# A new plan op = a record method of ConvPlan + one entry of OP_KINDS + one dispatch line in ssdk_run_ops (csrc/ssdk_conv.hip).
OpKind = collections.namedtuple("OpKind", "code out fill row")


def _pnhw(L):
    return L["pack"], L["n"], L["h"], L["w"]


def _conv_out(L):
    pk = L["pack"]
    return (pk.cout,) + _out_hw(L["h"], L["w"], pk.k, pk.stride)


def _conv_fill(plan, i, L, op):
    y_ptr = plan.arena.ptr(L["y"]) if L["y"] is not None else 0
    res_ptr = plan._ptr(L["res"], plan.patches, i, "conv.residual") if L["res"] is not None else None
    fill_desc(op.conv, plan._ptr(L["x"], plan.patches, i, "conv.x"), L["n"], L["h"], L["w"], L["pack"],
              plan.dtype_code, L["act"], y_ptr, N.NHWC, N.NCHW if L["nchw"] else N.NHWC, res_ptr, None,
              L.get("split"), L.get("act2"))
    op.conv.res_mode = conv_res_mode(L["pack"], L.get("res_mode", 0))  # (L["res_mode"] stays the 2-bit value)


def _conv_row(L, es):
    pk, n, h, w = _pnhw(L)
    _, ho, wo = _conv_out(L)
    macs = n * ho * wo * pk.cout * (pk.cin // pk.groups) * pk.k * pk.k
    byt = es * (n * (h * w * pk.cin + ho * wo * pk.cout) + pk.cout * (pk.cin // pk.groups) * pk.k * pk.k)
    kind = "head" if L["nchw"] else ("tower" if L.get("role") == "tower" else
                                     ("dw" if pk.kind == "dw" else ("gconv" if pk.groups > 1 else "conv")))
    dil = " d%d" % pk.dilation if getattr(pk, "dilation", 1) > 1 else ""
    return dict(name="%s %d>%d k%d s%d%s @%dx%d" % (kind, pk.cin, pk.cout, pk.k, pk.stride, dil, h, w),
                flops=2.0 * macs, bytes=float(byt), kind=kind)


def _mb_out(L):
    pk = L["pack"]
    hs, ws = _out_hw(L["h"], L["w"], 3, 2) if pk.stem else (L["h"], L["w"])
    return (pk.cout,) + _out_hw(hs, ws, 3, pk.stride)


def _mb_fill(plan, i, L, op):
    fill_mb_desc(op.mb, plan._ptr(L["x"], plan.patches, i, "mb.x"), plan.arena.ptr(L["y"]), L["n"], L["h"],
                 L["w"], L["pack"], plan.dtype_code)


def _mb_row(L, es):
    pk, n, h, w = _pnhw(L)
    _, ho, wo = _mb_out(L)
    if pk.stem:  # stem 3x3/s2 (cin -> chid) + depthwise + projection
        hs, ws = _out_hw(h, w, 3, 2)
        macs = n * (hs * ws * 9 * pk.cin * pk.chid + ho * wo * 9 * pk.chid + ho * wo * pk.chid * pk.cout)
    else:
        macs = n * (h * w * pk.cin * pk.chid + ho * wo * 9 * pk.chid + ho * wo * pk.chid * pk.cout)
    byt = es * n * (h * w * pk.cin + ho * wo * pk.cout)
    name = "mbconv%s %d>%d>%d s%d @%dx%d" % ("+stem" if pk.stem else "", pk.cin, pk.chid, pk.cout, pk.stride, h, w)
    return dict(name=name, flops=2.0 * macs, bytes=float(byt), kind="mbconv")


def _mbse_fill(plan, i, L, op):
    fill_mbse_desc(op.mbse, L["pack"], L["n"], L["h"], L["w"], plan.dtype_code,
                   plan._ptr(L["x"], plan.patches, i, "mbse.x"), plan.arena.ptr(L["t"]), plan.arena.ptr(L["partial"]),
                   plan.arena.ptr(L["gate"]), plan.arena.ptr(L["y"]),
                   plan._ptr(L["res"], plan.patches, i, "mbse.residual") if L["res"] is not None else None)


def _mbse_row(L, es):  # depthwise + SE + gated projection: x in, y out, t written and read once, the weights
    pk, n, h, w = _pnhw(L)
    _, ho, wo = _conv_out(L)
    macs = n * (ho * wo * pk.k * pk.k * pk.cin + 2 * pk.cin * pk.r + ho * wo * pk.cin * pk.cout)
    byt = (es * (n * (h * w * pk.cin + 2 * ho * wo * pk.cin + ho * wo * pk.cout) + pk.k * pk.k * pk.cin
                 + pk.cin * pk.cout) + 4 * (2 * pk.cin * pk.r + pk.r + pk.cin))
    return dict(name="mbse %d>%d k%d s%d @%dx%d" % (pk.cin, pk.cout, pk.k, pk.stride, h, w), flops=2.0 * macs,
                bytes=float(byt), kind="mbconv")


def _convt_out(L):
    return (L["pack"].cout, 2 * L["h"] - 1, 2 * L["w"] - 1)


def _carried(plan, i, L, op, cin, cout, k, stride, split, act="none"):
    """What the kinds carried by the op's ssdk_conv_desc under other field names (include/ssdk.h SSDK_OP_CONVT, _CAT, _SPP,
    _DENSEPOOL, _DENSEPLACE) fill alike; -> the descriptor for the kind's own fields."""
    c = op.conv
    c.x, c.y = plan._ptr(L["x"], plan.patches, i, "conv.x"), plan.arena.ptr(L["y"])
    c.N, c.Cin, c.H, c.W, c.Cout, c.k, c.stride, c.groups = L["n"], cin, L["h"], L["w"], cout, k, stride, 1
    c.act, c.act2 = N.ACT[act], N.ACT["none"]
    c.split, c.dtype, c.in_layout, c.out_layout = split, plan.dtype_code, N.NHWC, N.NHWC
    return c


def _convt_fill(plan, i, L, op):  # w = the parity images
    pk = L["pack"]
    c = _carried(plan, i, L, op, pk.cin, pk.cout, 3, 2, pk.cout)
    c.w = pk.w.data_ptr()
    c.bias = pk.bias.data_ptr() if pk.bias is not None else None
    c.residual = plan._ptr(L["res"], plan.patches, i, "conv.residual") if L["res"] is not None else None


def _convt_row(L, es):  # 9 taps per 2 x 2 output quad, less the last row / column's; x, skip, y and the weights once
    pk, n, h, w = _pnhw(L)
    _, ho, wo = _convt_out(L)
    macs = n * pk.cin * pk.cout * (h * w + 2 * h * (w - 1) + 2 * (h - 1) * w + 4 * (h - 1) * (w - 1))
    byt = es * (n * (h * w * pk.cin + (2 if L["res"] is not None else 1) * ho * wo * pk.cout) + 9 * pk.cin * pk.cout)
    return dict(name="convt %d>%d k3 s2 @%dx%d" % (pk.cin, pk.cout, h, w), flops=2.0 * macs, bytes=float(byt), kind="conv")


def _cat_fill(plan, i, L, op):
    c = _carried(plan, i, L, op, L["c1"], L["c1"] + L["c2"], 1, 1, L["c1"] + L["c2"])
    c.residual, c.res_mode = plan._ptr(L["b"], plan.patches, i, "conv.residual"), 1 if L["up2"] else 0


def _cat_row(L, es):  # data movement: both sources and the output once
    n, h, w, c1, c2 = L["n"], L["h"], L["w"], L["c1"], L["c2"]
    src_b = (h // 2) * (w // 2) if L["up2"] else h * w
    return dict(name="cat %d+%d%s @%dx%d" % (c1, c2, " up2" if L["up2"] else "", h, w), flops=0.0,
                bytes=float(es * n * (h * w * c1 + src_b * c2 + h * w * (c1 + c2))), kind="fuse")


def _spp_fill(plan, i, L, op):
    _carried(plan, i, L, op, L["ch"], 4 * L["ch"], 5, 1, 4 * L["ch"])


def _spp_row(L, es):  # comparisons only: x once, the four slices once
    n, h, w, ch = L["n"], L["h"], L["w"], L["ch"]
    return dict(name="spp %d k5,9,13 @%dx%d" % (ch, h, w), flops=0.0, bytes=float(es * n * h * w * 5 * ch), kind="fuse")


def _xpair_out(L):
    return (L["pack2"].cout,) + _out_hw(L["h"], L["w"], 3, 2)


def _xpair_fill(plan, i, L, op):
    fill_xpair_desc(op.xpair, plan._ptr(L["x"], plan.patches, i, "xpair.x"), plan.arena.ptr(L["y"]), L["n"], L["h"],
                    L["w"], L["pack"], L["pack2"], plan.dtype_code)


def _xpair_row(L, es):
    pk, n, h, w = _pnhw(L)
    p2 = L["pack2"]
    _, ho, wo = _xpair_out(L)
    macs = n * (h * w * pk.cin * pk.cout + ho * wo * 9 * p2.cin * p2.cout)
    byt = es * (n * (h * w * pk.cin + ho * wo * p2.cout) + pk.cin * pk.cout + 9 * p2.cin * p2.cout)
    return dict(name="extra %d>%d>%d k1,k3s2 @%dx%d" % (pk.cin, pk.cout, p2.cout, h, w), flops=2.0 * macs,
                bytes=float(byt), kind="conv")


def _dkres_fill(plan, i, L, op):  # carried by the op's ssdk_xpair_desc (include/ssdk.h SSDK_OP_DKRES)
    fill_dkres_desc(op.xpair, plan._ptr(L["x"], plan.patches, i, "xpair.x"), plan.arena.ptr(L["y"]), L["n"], L["h"],
                    L["w"], L["pack"], L["pack2"], plan.dtype_code)


def _dkres_row(L, es):  # both convolutions' MACs; x in and y out once (mid never leaves the CU), the weights
    pk, n, h, w = _pnhw(L)
    p2 = L["pack2"]
    macs = n * h * w * (pk.cin * pk.cout + 9 * p2.cin * p2.cout)
    byt = es * (n * h * w * (pk.cin + p2.cout) + pk.cin * pk.cout + 9 * p2.cin * p2.cout)
    return dict(name="dkres %d>%d>%d k1,k3 @%dx%d" % (pk.cin, pk.cout, p2.cout, h, w), flops=2.0 * macs,
                bytes=float(byt), kind="conv")


def _dense_fill(plan, i, L, op):  # carried by the op's ssdk_xpair_desc (include/ssdk.h SSDK_OP_DENSE)
    fill_dense_desc(op.xpair, plan.arena.ptr(L["x"]), L["n"], L["h"], L["w"], L["cin"], L["ld"], L["pack"], plan.dtype_code,
                    plan.es)


def _dense_row(L, es):  # both convolutions' MACs; Cin channels in, 32 out (m never leaves the CU), the weights
    pk, n, h, w = _pnhw(L)
    macs = n * h * w * (pk.cin * pk.cmid + 9 * pk.cmid * pk.cout)
    byt = es * (n * h * w * (pk.cin + pk.cout) + pk.cin * pk.cmid + 9 * pk.cmid * pk.cout)
    return dict(name="dense %d>%d>%d k1,k3 @%dx%d" % (pk.cin, pk.cmid, pk.cout, h, w), flops=2.0 * macs,
                bytes=float(byt), kind="conv")


def _densepool_fill(plan, i, L, op):
    c = _carried(plan, i, L, op, L["ch"], L["ch"], 2, 2, L["ld"], act="relu")
    c.scale, c.bias = L["a"].data_ptr(), L["b"].data_ptr()


def _densepool_out(L):
    return (L["ch"], L["h"] // 2, L["w"] // 2)


def _densepool_row(L, es):  # the block's c channels in, a quarter of the pixels out
    n, h, w, ch = L["n"], L["h"], L["w"], L["ch"]
    _, ho, wo = _densepool_out(L)
    return dict(name="densepool %d @%dx%d" % (ch, h, w), flops=16.0 * n * ch * ho * wo,
                bytes=float(es * n * ch * (h * w + ho * wo) + 8 * ch), kind="pool")


def _denseplace_fill(plan, i, L, op):
    _carried(plan, i, L, op, L["ch"], L["ch"], 1, 1, L["ld"])


def _denseplace_row(L, es):  # data movement: the map in and out once
    n, h, w, ch = L["n"], L["h"], L["w"], L["ch"]
    return dict(name="denseplace %d>%d @%dx%d" % (ch, L["ld"], h, w), flops=0.0, bytes=float(es * 2 * n * ch * h * w), kind="fuse")


def _shuffle_fill(plan, i, L, op):  # carried by the op's mb (+ xpair) members (include/ssdk.h SSDK_OP_SHUFFLE)
    fill_shuffle_desc(op, plan._ptr(L["x"], plan.patches, i, "mb.x"), plan.arena.ptr(L["y"]), L["n"], L["h"], L["w"],
                      L["pack"], plan.dtype_code, ld_in=L.get("ld", 0))


def _shuffle_row(L, es):  # branch2's MACs; x in and y out once (neither intermediate leaves the CU), the weights
    pk, n, h, w = _pnhw(L)
    cb = pk.cb
    return dict(name="shuffle %d k1,dw3,k1 @%dx%d" % (2 * cb, h, w), flops=2.0 * n * h * w * (2 * cb * cb + 9 * cb),
                bytes=float(es * (n * h * w * 4 * cb + 2 * cb * cb + 9 * cb)), kind="conv")


def _shuffledown_out(L):
    return (pad8(2 * L["pack"].cb),) + _out_hw(L["h"], L["w"], 3, 2)


def _shuffledown_row(L, es):  # both branches' MACs; x in once, y out once, the weights
    pk, n, h, w = _pnhw(L)
    cb, cin = pk.cb, pk.cin
    _, ho, wo = _shuffledown_out(L)
    macs = n * (h * w * cin * cb + ho * wo * (9 * cb + cb * cb + 9 * cin + cin * cb))
    return dict(name="shuffledown %d>%d k1,dw3s2,k1 @%dx%d" % (cin, 2 * cb, h, w), flops=2.0 * macs,
                bytes=float(es * (n * (h * w * cin + ho * wo * 2 * cb) + 2 * cin * cb + cb * cb + 9 * (cin + cb))), kind="conv")


def _stem7_out(L):
    return (L["pack"].cout,) + _out_hw(L["h"], L["w"], 7, 2)


def _stem7_fill(plan, i, L, op):
    fill_stem_desc(op.stem, plan._ptr(L["x"], plan.patches, i, "stem.x"), plan.arena.ptr(L["y"]), L["n"], L["h"], L["w"], 3,
                   L["pack"], plan.dtype_code, N.NCHW)


def _stem7_row(L, es):
    pk, n, h, w = _pnhw(L)
    _, ho, wo = _stem7_out(L)
    return dict(name="stem7 3>%d @%dx%d" % (pk.cout, h, w), flops=2.0 * n * ho * wo * 147 * pk.cout,
                bytes=float(es * n * (3 * h * w + pk.cout * ho * wo)), kind="stem")


def _pool_out(L):
    return (L["ch"],) + _out_hw(L["h"], L["w"], 3, 2)


def _pool_fill(plan, i, L, op):
    fill_pool_desc(op.pool, plan._ptr(L["x"], plan.patches, i, "pool.x"), plan.arena.ptr(L["y"]), L["n"], L["h"], L["w"], L["ch"],
                   plan.dtype_code)


def _pool_row(L, es):
    n, h, w, ch = L["n"], L["h"], L["w"], L["ch"]
    _, ho, wo = _pool_out(L)
    return dict(name="maxpool %d @%dx%d" % (ch, h, w), flops=9.0 * n * ch * ho * wo,
                bytes=float(es * n * ch * (h * w + ho * wo)), kind="pool")


def _fuse_fill(plan, i, L, op):
    a = plan._ptr(L["a"][0], plan.patches, i, "fuse.a")
    b = plan._ptr(L["b"][0], plan.patches, i, "fuse.b")
    c = plan._ptr(L["c"][0], plan.patches, i, "fuse.c") if L["c"] is not None else None
    fill_fuse_desc(op.fuse, a, b, c, plan.arena.ptr(L["y"]), L["n"], L["h"], L["w_"], L["ch"], L["w"], L["mode_b"], L["mode_c"],
                   L["b"][3:], L["c"][3:] if L["c"] is not None else None, plan.dtype_code)


def _fuse_row(L, es):
    n, h, w, ch = L["n"], L["h"], L["w_"], L["ch"]
    srcs = [L["a"], L["b"]] + ([L["c"]] if L["c"] is not None else [])
    byt = es * (sum(v[1] * v[2] * v[3] * v[4] for v in srcs) + n * ch * h * w)
    return dict(name="fuse x%d %d @%dx%d" % (len(srcs), ch, h, w), flops=2.0 * len(srcs) * n * ch * h * w,
                bytes=float(byt), kind="fuse")


OP_KINDS = {
    None: OpKind(N.OP_CONV, _conv_out, _conv_fill, _conv_row),  # a convolution or a head
    "mb": OpKind(N.OP_MBCONV, _mb_out, _mb_fill, _mb_row),
    "mbse": OpKind(N.OP_MBSE, _conv_out, _mbse_fill, _mbse_row),
    "convt": OpKind(N.OP_CONVT, _convt_out, _convt_fill, _convt_row),
    "cat": OpKind(N.OP_CAT, lambda L: (L["c1"] + L["c2"], L["h"], L["w"]), _cat_fill, _cat_row),
    "spp": OpKind(N.OP_SPP, lambda L: (4 * L["ch"], L["h"], L["w"]), _spp_fill, _spp_row),
    "xpair": OpKind(N.OP_XPAIR, _xpair_out, _xpair_fill, _xpair_row),
    "dkres": OpKind(N.OP_DKRES, lambda L: (L["pack2"].cout, L["h"], L["w"]), _dkres_fill, _dkres_row),
    "dense": OpKind(N.OP_DENSE, lambda L: (L["cin"] + L["pack"].cout, L["h"], L["w"]), _dense_fill, _dense_row),
    "densepool": OpKind(N.OP_DENSEPOOL, _densepool_out, _densepool_fill, _densepool_row),
    "denseplace": OpKind(N.OP_DENSEPLACE, lambda L: (L["ch"], L["h"], L["w"]), _denseplace_fill, _denseplace_row),
    "shuffle": OpKind(N.OP_SHUFFLE, lambda L: (pad8(2 * L["pack"].cb), L["h"], L["w"]), _shuffle_fill, _shuffle_row),
    "shuffledown": OpKind(N.OP_SHUFFLEDOWN, _shuffledown_out, _shuffle_fill, _shuffledown_row),
    "stem7": OpKind(N.OP_STEM7, _stem7_out, _stem7_fill, _stem7_row),
    "pool": OpKind(N.OP_POOL, _pool_out, _pool_fill, _pool_row),
    "fuse": OpKind(N.OP_FUSE, lambda L: (L["ch"], L["h"], L["w_"]), _fuse_fill, _fuse_row),
}


class _Arena(object):
    """Greedy re-use of activation buffers inside one plan (the network is a chain: a buffer is free again
    once its last reader has been recorded)."""

    def __init__(self, device):
        self.device = device
        self.bufs = []  # [tensor(uint8), free]

    def get(self, nbytes):
        best = None
        for i, (t, free) in enumerate(self.bufs):
            if free and t.numel() >= nbytes and (best is None or t.numel() < self.bufs[best][0].numel()):
                best = i
        if best is None:
            self.bufs.append([torch.empty(max(nbytes, 256), dtype=torch.uint8, device=self.device), False])
            return len(self.bufs) - 1
        self.bufs[best][1] = False
        return best

    def release(self, i):
        if i is not None:
            self.bufs[i][1] = True

    def ptr(self, i):
        return self.bufs[i][0].data_ptr()

    def total_bytes(self):
        return sum(t.numel() for t, _ in self.bufs)


class ExtBuf(object):
    """An external input of a plan (the image, or a backbone feature map computed outside the plan): the
    descriptors that read it are patched with the tensor's address on every run."""

    def __init__(self, index, shape):
        self.index, self.shape = index, tuple(shape)


class ConvPlan(object):
    """A recorded forward: ops (fused convs, fused MobileNet blocks, BiFPN fusions) on arena buffers.
    ``record`` by walking the model once for given input shapes; ``run(*inputs)`` replays it with ONE C call.
    Head outputs are allocated per call (they are returned to the caller); all other activations live in the
    plan's arena.  A "value" is ``(buffer index | ExtBuf, n, c, h, w)``."""

    def __init__(self, device, dtype, in_shape=None):
        self.device, self.dtype = device, dtype
        self.dtype_code = N._DTYPES[dtype]
        self.es = 2
        self.arena = _Arena(device)
        self.pinned = set()  # arena buffers read by side-lane ops: never re-used (see head())
        self.layers = []   # dicts with everything the descriptor fillers need
        self.heads = []    # (layer index, n, split | None, cout, ho, wo, tag)
        self.keep = []     # packs kept alive
        self.inputs = []   # ExtBuf
        self.ops = None
        self.report = []
        self.in_shape = tuple(in_shape) if in_shape is not None else None
        self._ctx = None  # this plan's side stream / events / op-profiling ring (include/ssdk.h "Contexts"): lazy
        self.side_chain = False  # tower chains recorded for the side stream: the plan turns its context's side lane on
        self.head_order = []     # per head: the level it belongs to (None: recording order)
        if in_shape is not None:
            self.add_input(in_shape)

    @property
    def ctx(self):
        if self._ctx is None:
            self._ctx = N.Context(self.device)
        return self._ctx

    def add_input(self, shape):
        """Declare an external [N,C,H,W] input (channels_last memory at run time); returns its value."""
        e = ExtBuf(len(self.inputs), shape)
        self.inputs.append(e)
        n, c, h, w = e.shape
        return (e, n, c, h, w)

    def input_value(self):
        e = self.inputs[0]
        n, c, h, w = e.shape
        return (e, n, c, h, w)

    def conv(self, val, pack, act=None, residual=None, res_mode=0, role=None, lane=0):
        """res_mode bit 0: the residual value is half resolution (nearest x2 upsample, FPN top-down);
        bit 1: the activation follows the add (ResNet blocks).  ``role='tower'`` marks the 3x3 convs of the shared
        head towers (fpn.py:10-18) for the per-layer table: they are head convolutions, not neck.
        ``lane=2`` records the op for the executor's side stream (a chain of small-level tower layers next to the big
        levels, planner._record_extras_and_towers; include/ssdk.h: lane 2 = the in-line kernel choice): its input and
        output buffers are pinned like a side-lane head's."""
        buf, n, c, h, w = val
        pack = self._fit(val, pack)
        assert c == pack.cin, (c, pack.cin)
        if pack.cout % 8 and _PADDED_MAPS.on:  # (behind a backbone of zero-padded maps) an NHWC map of e.g. 244 channels: written as 248
            # per pixel, zeros in the padding
            if (pack.act if act is None else act) not in ("none", "relu", "relu6", "silu"):
                raise N.SsdkError("a zero-padded map behind the activation {}".format(pack.act if act is None else act))
            pack = pack.with_padded_output()
        if residual is not None:
            assert value_segs(residual) == ((getattr(pack, "cout_real", pack.cout), pack.cout),), (value_segs(residual), pack.cout)
        out = self._record(dict(x=buf, n=n, h=h, w=w, pack=pack, act=pack.act if act is None else act,
                                res=residual[0] if residual is not None else None, res_mode=res_mode, nchw=False,
                                role=role, lane=lane))
        if lane:
            self._pin_side(buf, out[0])
        self.keep.append(pack)
        return self._padded(out, getattr(pack, "cout_real", pack.cout))

    def _record(self, L):
        """Appends the layer dict ``L`` with a fresh arena buffer ``y`` of the shape its kind's ``out`` gives; -> the output value."""
        c, ho, wo = OP_KINDS[L.get("kind")].out(L)
        L["y"] = self.arena.get(L["n"] * c * ho * wo * self.es)
        self.layers.append(L)
        return (L["y"], L["n"], c, ho, wo)

    def _pin_side(self, buf, out):
        """A lane != 0 op runs on the executor's side stream next to the main chain: its output and its input (unless external) are
        never handed out again inside this plan (see head())."""
        self.side_chain = True
        self.pinned.add(out)
        if not isinstance(buf, ExtBuf):
            self.pinned.add(buf)

    def mbconv(self, val, pk):
        buf, n, c, h, w = val
        assert c == pk.cin, (c, pk.cin)
        self.keep.append(pk)
        return self._record(dict(kind="mb", x=buf, n=n, h=h, w=w, pack=pk))

    def mbse(self, val, pack, residual=None):
        """The tail of an EfficientNet MBConv block (``MbSePack``) on ``val`` = the expanded tensor (or the block input of an
        expand-free block); ``residual``: the block input, added in the projection's epilogue.  t, pool_partial and gate are
        arena scratch, handed back as soon as the op is recorded (lane 0 ops run in order)."""
        buf, n, c, h, w = val
        assert c == pack.cin, (c, pack.cin)
        L = dict(kind="mbse", x=buf, n=n, h=h, w=w, pack=pack, res=residual[0] if residual is not None else None)
        out = self._record(L)
        ho, wo = out[3:]
        if residual is not None:
            assert tuple(residual[1:]) == out[1:], (residual[1:], out[1:])
        tiles = mbse_pool_tiles(h, w, pack.k, pack.stride)
        scratch = [self.arena.get(n * c * ho * wo * self.es), self.arena.get(n * tiles * c * 4), self.arena.get(n * c * 4)]
        L.update(t=scratch[0], partial=scratch[1], gate=scratch[2])
        for b in scratch:
            self.arena.release(b)
        self.keep.append(pack)
        return out

    def convt(self, val, pack, skip=None):
        """Transposed 3x3 / stride 2 / pad 1 convolution (``ConvTPack``) + bias (+ ``skip``, a value at the output's size): the
        decoder step of the Shelf neck as one op, [n, c, h, w] -> [n, cout, 2h - 1, 2w - 1]."""
        buf, n, c, h, w = val
        assert c == pack.cin, (c, pack.cin)
        out = self._record(dict(kind="convt", x=buf, n=n, h=h, w=w, pack=pack, res=skip[0] if skip is not None else None))
        if skip is not None:
            assert tuple(skip[1:]) == out[1:], (skip[1:], out[1:])
        self.keep.append(pack)
        return out

    def cat(self, a, b, up2=False):
        """Channel concatenation ``a || b`` (``up2``: ``b`` at half the size of ``a``, nearest x2 on the way) as one op
        (csrc/ssdk_cat.hip): [n, c1, h, w], [n, c2, ...] -> [n, c1 + c2, h, w]."""
        buf, n, c1, h, w = a
        bbuf, nb, c2, hb, wb = b
        assert nb == n and (hb, wb) == ((h // 2, w // 2) if up2 else (h, w)) and not (up2 and (h % 2 or w % 2)), (a[1:], b[1:], up2)
        assert cat_supported(c1, c2, h, w, up2) is None, cat_supported(c1, c2, h, w, up2)
        val = self._record(dict(kind="cat", x=buf, b=bbuf, n=n, h=h, w=w, c1=c1, c2=c2, up2=bool(up2)))
        if hasattr(a, "segs") or hasattr(b, "segs"):  # zero-padded maps keep their padding where it is: the readers' packs follow
            val = PaddedValue(val, value_segs(a) + value_segs(b))
        return val

    def spp(self, val):
        """The SPP block ``x || maxpool5(x) || maxpool9(x) || maxpool13(x)`` as one op (csrc/ssdk_cat.hip):
        [n, c, h, w] -> [n, 4 c, h, w]."""
        buf, n, c, h, w = val
        assert c >= 8 and c % 8 == 0, c
        out = self._record(dict(kind="spp", x=buf, n=n, h=h, w=w, ch=c))
        if hasattr(val, "segs"):  # (max-pooling keeps the zeros of a padded map where they are, in each of the four slices)
            return PaddedValue(out, val.segs * 4)
        return out

    def xpair(self, val, p1, p2, lane=0):
        buf, n, c, h, w = val
        p1 = self._fit(val, p1)
        assert c == p1.cin, (c, p1.cin)
        out = self._record(dict(kind="xpair", x=buf, n=n, h=h, w=w, pack=p1, pack2=p2, lane=lane))
        if lane:
            self._pin_side(buf, out[0])
        self.keep.extend([p1, p2])
        return out

    def dkres(self, val, p1, p2):
        """A DarkNet residual block as one op (csrc/ssdk_dkres.hip): [n, c, h, w] -> [n, c, h, w].  The output is a buffer of its
        own -- the arena never hands out ``val``'s while ``val`` is unreleased, and the kernel refuses y == x."""
        buf, n, c, h, w = val
        assert c == p1.cin == p2.cout and p1.cout == p2.cin, (c, p1.cin, p1.cout, p2.cin, p2.cout)
        self.keep.extend([p1, p2])
        return self._record(dict(kind="dkres", x=buf, n=n, h=h, w=w, pack=p1, pack2=p2))

    def dense_block(self, n, ctot, h, w):
        """The ONE buffer [n][h][w][ctot] of a dense block (csrc/ssdk_denselayer.hip): ``dense_place`` fills its first channels,
        every ``dense`` op appends 32, and once the last layer is recorded ``(buffer, n, ctot, h, w)`` is an ordinary dense value
        (pixel stride == channels).  It stays out of the arena's free list until that value is released."""
        return self.arena.get(n * ctot * h * w * self.es)

    def dense_place(self, val, block, ld):
        """Copies the dense value ``val`` into channels [0, c) of ``block`` (pixel stride ``ld``); returns the channel count."""
        buf, n, c, h, w = val
        assert c % 8 == 0 and c <= ld and ld % 8 == 0, (c, ld)
        self.layers.append(dict(kind="denseplace", x=buf, n=n, h=h, w=w, ch=c, ld=ld, y=block))
        return c

    def dense(self, block, n, cin, h, w, ld, pack):
        """One dense layer as one op: reads channels [0, cin) of ``block`` and writes [cin, cin + 32); returns the new count."""
        assert cin == pack.cin and cin + pack.cout <= ld, (cin, pack.cin, pack.cout, ld)
        L = dict(kind="dense", x=block, n=n, h=h, w=w, cin=cin, ld=ld, pack=pack, y=block)
        self.layers.append(L)
        self.keep.append(pack)
        return OP_KINDS["dense"].out(L)[0]

    def dense_pool(self, val, a, b):
        """The front of a transition on a finished block (``val``, pixel stride == channels): avgpool2x2(relu(a x + b)) as one op,
        [n, c, h, w] -> [n, c, h / 2, w / 2] dense."""
        buf, n, c, h, w = val
        assert h >= 2 and w >= 2 and a.numel() == c == b.numel(), (c, h, w, a.numel())
        self.keep.extend([a, b])
        return self._record(dict(kind="densepool", x=buf, n=n, h=h, w=w, ch=c, ld=c, a=a, b=b))

    def shuffle_unit(self, val, pack):
        """A stride-1 ShuffleNetV2 unit as one op (csrc/ssdk_shuffle.hip): [n, Cp, h, w] -> [n, Cp, h, w], Cp = pad8(2 cb) physical
        channels of which 2 cb are real (a ``PaddedValue`` when they differ).  The output is a buffer of its own."""
        buf, n, c, h, w = val
        assert c == pad8(2 * pack.cb) and value_segs(val)[0][0] == 2 * pack.cb, (c, value_segs(val), pack.cb)
        self.keep.append(pack)
        return self._padded(self._record(dict(kind="shuffle", x=buf, n=n, h=h, w=w, pack=pack)), 2 * pack.cb)

    def shuffle_down(self, val, pack):
        """A stride-2 unit as one op: [n, ld, h, w] of which the first ``pack.cin`` channels are real -> [n, pad8(2 cb), ho, wo]."""
        buf, n, c, h, w = val
        assert c % 8 == 0 and c >= pack.cin and value_segs(val)[0][0] == pack.cin, (c, value_segs(val), pack.cin)
        self.keep.append(pack)
        return self._padded(self._record(dict(kind="shuffledown", x=buf, n=n, h=h, w=w, ld=c, pack=pack)), 2 * pack.cb)

    @staticmethod
    def _padded(val, real):
        return PaddedValue(val, ((real, val[2]),)) if real != val[2] else val

    def _fit(self, val, pack):
        """``pack`` for reading ``val``: as it is, or -- when ``val`` is a zero-padded map laid out differently from what the pack was
        built for (behind a concatenation) -- a copy with zero weight columns at ``val``'s padding channels."""
        segs = getattr(val, "segs", None)
        if segs is not None and getattr(pack, "in_segs", None) != segs:
            pack = pack.with_input_segs(segs)
        return pack

    def read(self, val):
        """The REAL channels of a recorded value after a run, as a channels_last view [n, c, h, w] of its arena buffer (a zero-padded
        map of one segment is sliced to its real channels)."""
        buf, n, c, h, w = val
        t = self.arena.bufs[buf][0][: n * c * h * w * self.es].view(self.dtype).view(n, h, w, c)
        segs = value_segs(val)
        assert len(segs) == 1, segs
        return t[..., :segs[0][0]].permute(0, 3, 1, 2)

    def stem7(self, val, pack):
        buf, n, c, h, w = val
        self.keep.append(pack)
        return self._record(dict(kind="stem7", x=buf, n=n, h=h, w=w, pack=pack))

    def pool(self, val):
        buf, n, c, h, w = val
        return self._record(dict(kind="pool", x=buf, n=n, h=h, w=w, ch=c))

    def fuse(self, a, b, c=None, weights=(1.0, 1.0, 0.0), mode_b=N.FUSE_SAME, mode_c=N.FUSE_SAME):
        """y = w0*a + w1*R_b(b) [+ w2*R_c(c)] at the resolution of ``a`` (BiFPN weighted fusion)."""
        _, n, ch, h, w = a
        out = self._record(dict(kind="fuse", a=a, b=b, c=c, w=tuple(float(v) for v in weights), mode_b=mode_b,
                                mode_c=mode_c, n=n, h=h, w_=w, ch=ch))
        if hasattr(a, "segs"):  # (a weighted sum of maps padded alike is padded alike)
            assert all(value_segs(v) == a.segs for v in (b, c) if v is not None), [value_segs(v) for v in (a, b, c) if v is not None]
            return PaddedValue(out, a.segs)
        return out

    def head(self, val, pack, split=None, act="none", act2=None, tag="both", lane=None, position=None, level=None):
        """An NCHW output of the plan: loc|conf of one SSD level as one split GEMM (``tag='both'``) or the last
        conv of one shared tower (``tag='loc' | 'conf'``).  ``level``: the pyramid level of the output when the heads are
        recorded out of level order (small levels first, on the side stream); the outputs are returned in level order."""
        buf, n, c, h, w = val
        pack = self._fit(val, pack)
        assert c == pack.cin, (c, pack.cin)
        _, ho, wo = OP_KINDS[None].out(dict(pack=pack, h=h, w=w))
        # small heads are leaves of latency-bound work: they run on the executor's side stream next to the main
        # chain (SSDK_SIDE_STREAM); the big levels fill the chip on their own and stay in line.  A side-lane op
        # reads its input while the main lane keeps going, so that buffer must never be handed out again inside
        # this plan (the arena re-uses a buffer as soon as its last reader is RECORDED, which orders nothing
        # across streams): it is pinned.
        if lane is None:
            lane = 1 if n * ho * wo <= 4096 else 0
        if lane and not isinstance(buf, ExtBuf):
            self.pinned.add(buf)
        self.layers.append(dict(x=buf, n=n, h=h, w=w, pack=pack, act=act, y=None, res=None, res_mode=0, nchw=True,
                                split=split, act2=act2, lane=lane))
        entry = (len(self.layers) - 1, n, split, pack.cout, ho, wo, tag)
        if position is None:
            self.heads.append(entry)
            self.head_order.append(level)
        else:  # recorded out of level order (lane balancing): the outputs keep the level order
            self.heads.insert(position, entry)
            self.head_order.insert(position, level)
        self.keep.append(pack)

    def release(self, val):
        if not isinstance(val[0], ExtBuf) and val[0] not in self.pinned:
            self.arena.release(val[0])

    def _ptr(self, buf, patches, op_index, field):
        if buf is None:
            return 0
        if isinstance(buf, ExtBuf):
            patches.append((op_index, field, buf.index))
            return 0
        return self.arena.ptr(buf)

    def finalize(self):
        if any(o is not None for o in self.head_order):  # heads recorded out of level order: back into level order
            assert all(o is not None for o in self.head_order)
            order = sorted(range(len(self.heads)), key=lambda i: self.head_order[i])
            self.heads = [self.heads[i] for i in order]
            self.head_order = [self.head_order[i] for i in order]
        need = 0
        for L in self.layers:
            if L.get("kind") is None:
                pk = L["pack"]
                need = max(need, int(N.lib.ssdk_conv_workspace_bytes(L["n"], pk.cin, L["h"], L["w"], pk.cout, pk.k,
                                                                      pk.stride, self.dtype_code)))
        # split-K scratch (fp32 slabs + arrival counters): zero-initialised once, re-armed by the kernels.  The heads
        # may run on the executor's side stream concurrently with the main chain and get their own half.
        need = (need + 255) & ~255
        self.ws = torch.zeros(2 * need + 512, dtype=torch.uint8, device=self.device) if need else None
        self.ops = (N.Op * len(self.layers))()
        self.patches = []  # (op index, field name, external input index)
        for i, (L, op) in enumerate(zip(self.layers, self.ops)):
            kind = OP_KINDS[L.get("kind")]
            op.kind = kind.code
            op.lane = L.get("lane", 0)  # side stream for the small heads and the small levels' chains (head(), _pin_side())
            kind.fill(self, i, L, op)
        return self

    def layer_table(self):
        """Geometry of every op of the plan: dicts with name, flops (2*MAC) and algorithmic HBM bytes
        (input + output + weights, each once) -- what the per-layer roofline numbers are computed from."""
        return [OP_KINDS[L.get("kind")].row(L, self.es) for L in self.layers]

    def _set_field(self, op_index, field, ptr):
        sub, name = field.split(".")
        setattr(getattr(self.ops[op_index], sub), name, ptr)

    def prepare(self, *inputs):
        """Points the recorded ops at this call's inputs and freshly allocated head outputs.  inputs: the tensors
        declared with ``add_input`` (the image: NCHW contiguous or channels_last; feature maps: converted to
        channels_last if needed).  Returns (loc tuple, conf tuple), NCHW -- filled once ``launch`` has run every op."""
        if len(inputs) != len(self.inputs):
            raise N.SsdkError("plan expects {} inputs, got {}".format(len(self.inputs), len(inputs)))
        held = []
        for e, x in zip(self.inputs, inputs):
            if tuple(x.shape) != e.shape or x.dtype != self.dtype:
                raise N.SsdkError("plan input {} was recorded as {} {}, got {} {}".format(
                    e.index, e.shape, self.dtype, tuple(x.shape), x.dtype))
        first_kind = self.ops[0].kind
        image_first = len(self.inputs) == 1 and self.inputs[0].shape[1] <= 4
        xs = list(inputs)
        if image_first:
            x = xs[0]
            if first_kind == N.OP_STEM7:  # ResNet stem reads the image in either layout
                first = self.ops[0].stem
                if x.is_contiguous():
                    first.in_layout = N.NCHW
                else:
                    x = x.contiguous(memory_format=torch.channels_last)
                    first.in_layout = N.NHWC
            elif first_kind == N.OP_MBCONV:  # stem + first block fused: the image is read by the block kernel
                first = self.ops[0].mb
                if x.is_contiguous():
                    first.stem = 1
                else:
                    x = x.contiguous(memory_format=torch.channels_last)
                    first.stem = 2
            else:
                first = self.ops[0].conv
                if x.is_contiguous():
                    first.in_layout = N.NCHW if self.layers[0]["pack"].kind == "stem" else N.NHWC
                    if first.in_layout == N.NHWC:
                        x = x.contiguous(memory_format=torch.channels_last)
                else:
                    x = x.contiguous(memory_format=torch.channels_last)
                    first.in_layout = N.NHWC
            xs[0] = x
        else:
            xs = [x if x.is_contiguous(memory_format=torch.channels_last) else
                  x.contiguous(memory_format=torch.channels_last) for x in xs]
        held.extend(xs)
        for (oi, field, ei) in self.patches:
            self._set_field(oi, field, xs[ei].data_ptr())
        loc, conf = [], []
        for (li, n, split, cout, ho, wo, tag) in self.heads:
            if tag == "both":
                l = torch.empty((n, split, ho, wo), device=self.device, dtype=self.dtype)
                c = torch.empty((n, cout - split, ho, wo), device=self.device, dtype=self.dtype)
                self.ops[li].conv.y, self.ops[li].conv.y2 = l.data_ptr(), c.data_ptr()
                loc.append(l)
                conf.append(c)
            else:
                t = torch.empty((n, cout, ho, wo), device=self.device, dtype=self.dtype)
                self.ops[li].conv.y = t.data_ptr()
                (loc if tag == "loc" else conf).append(t)
        if os.environ.get("SSDK_OPS_TRACE"):
            import sys
            for (li, n, split, cout, ho, wo, tag), t in zip(self.heads, [None] * len(self.heads)):
                sys.stderr.write("[plan] head op %d %s n=%d cout=%d %dx%d y=%#x\n" % (li, tag, n, cout, ho, wo, self.ops[li].conv.y or 0))
        self._held = held  # converted inputs stay alive until the next prepare()
        return tuple(loc), tuple(conf)

    def launch(self, lo=0, hi=None, stream=None):
        """Enqueue ops [lo, hi) of the plan on ``stream`` (default: the current stream) with ONE C call."""
        hi = len(self.layers) if hi is None else hi
        if hi <= lo:
            return
        ops = self.ops if lo == 0 else (N.Op * (hi - lo)).from_address(ctypes.addressof(self.ops) + lo * ctypes.sizeof(N.Op))
        sp = N.stream_ptr(self.device) if stream is None else ctypes.c_void_p(stream.cuda_stream)
        if self.side_chain:  # (SSDK_LEVEL_LANES=0 records no chains: planner._record_extras_and_towers)
            self.ctx.auto_side_lane()  # on by default; an explicit set_side_lane(False) / SSDK_SIDE_STREAM=0 is respected
        with torch.cuda.device(self.device):
            if self.ws is not None:
                wptr = (self.ws.data_ptr() + 255) & ~255
                rc = N.lib.ssdk_run_ops_ctx(self.ctx.ptr, ops, hi - lo, wptr,
                                            self.ws.numel() - (wptr - self.ws.data_ptr()), sp)
            else:
                rc = N.lib.ssdk_run_ops_ctx(self.ctx.ptr, ops, hi - lo, None, 0, sp)
        N.check(rc, "run_ops")
        STATS["native_layers"] += hi - lo

    def run(self, *inputs):
        """prepare + launch of the whole plan on the current stream.  Returns (loc tuple, conf tuple), NCHW."""
        out = self.prepare(*inputs)
        self.launch()
        STATS["plan_runs"] += 1
        return out


def sequential_groups(seq):
    """[Conv2d, (BatchNorm2d), (activation)]* -> [(conv, bn, act)], or None if the pattern does not match."""
    mods = list(seq.children())
    i, out = 0, []
    while i < len(mods):
        conv = mods[i]
        if not isinstance(conv, nn.Conv2d):
            return None
        bn, act, j = None, "none", i + 1
        if j < len(mods) and isinstance(mods[j], nn.BatchNorm2d):
            bn, j = mods[j], j + 1
        a = _act_name(mods[j]) if j < len(mods) else None
        if a is not None:
            act, j = a, j + 1
        out.append((conv, bn, act))
        i = j
    return out


class FusedSequentialMixin(object):
    """nn.Sequential of [Conv2d, (BatchNorm2d), (activation)]* groups: in eval mode on a HIP device each
    group is one fused launch; in training mode (or with SSDK_FUSED_CONV=0) the plain torch modules run."""

    def _packs(self, dtype):
        cache = getattr(self, "_ssdk_packs", None)
        if cache is None or cache[0] != dtype:
            groups = sequential_groups(self)
            packs = None
            if groups is not None and all(conv_kind(c) is not None for c, _, _ in groups):
                packs = [ConvPack(c, b, a, dtype) for c, b, a in groups]
            cache = (dtype, packs)
            object.__setattr__(self, "_ssdk_packs", cache)
        return cache[1]

    def train(self, mode=True):
        object.__setattr__(self, "_ssdk_packs", None)  # weights may change: re-fold on the next eval forward
        return nn.Sequential.train(self, mode)

    def _apply(self, fn, *a, **kw):
        object.__setattr__(self, "_ssdk_packs", None)
        return nn.Sequential._apply(self, fn, *a, **kw)

    def _load_from_state_dict(self, *a, **kw):
        # reached for EVERY module of the tree whichever ancestor's load_state_dict() was called (a parent's
        # load_state_dict never calls a child's): the folded weights of this block are stale from here on
        object.__setattr__(self, "_ssdk_packs", None)
        return nn.Sequential._load_from_state_dict(self, *a, **kw)

    def forward(self, x):
        if self.training or not fused_enabled() or not x.is_cuda or x.dtype not in (torch.bfloat16, torch.float16):
            return nn.Sequential.forward(self, x)
        packs = self._packs(x.dtype)
        if packs is None:
            STATS["torch_fallback_layers"] += 1
            return nn.Sequential.forward(self, x)
        for p in packs:
            x = conv_native(x, p)
        return x
