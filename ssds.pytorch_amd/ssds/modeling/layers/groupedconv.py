"""Grouped 3x3 convolutions of the training step on the NCHW tensors themselves (csrc/ssdk_gconvtrain.hip): the bottleneck
3x3 of RegNetX (nets/regnet.py) and ResNeXt (nets/resnet.py), forward, input gradient and weight gradient.

PyTorch-ROCm sends a grouped ``nn.Conv2d`` in bf16 to MIOpen's grouped convolution, through autocast's cast of the weight.
``GroupedConv3x3`` is an ``nn.Conv2d`` (same parameters, ``state_dict`` keys and initialisation) whose 16-bit HIP-device
forward / backward run on the ssdk kernels:

    prepare          ssdk_gconv3x3_train_prepare   fp32 master weight -> the 16-bit forward and input-gradient images
    forward          ssdk_gconv3x3_train_forward   y  = conv(x, W)
    input gradient   ssdk_gconv3x3_train_dgrad     dx = conv^T(dy, W)   (stride 2: by input-pixel parity, no zero-dilated dy)
    weight gradient  ssdk_gconv3x3_train_wgrad     dW fp32, pixel ranges added in index order: bit-reproducible

pad 1, stride 1 | 2, Cin == Cout == groups * gw with gw = 4 (an even number of groups) or a multiple of 8 up to 256.  CPU
tensors, fp32 tensors, non-contiguous tensors and every other layer shape take ``nn.Conv2d.forward``."""
import torch
import torch.nn as nn

from ssds import _native as N
from ssds.modeling.layers import kernel_conv as K
from ssds.modeling.layers.fused_conv import pack_grouped_frag

MAX_WIDTH = 256  # channels per group (csrc/ssdk_gconvtrain.hip gt_shape)
STATS = {"swapped": 0, "native_forward": 0, "native_dgrad": 0, "native_wgrad": 0}


def width_supported(channels, groups):
    """The widths csrc/ssdk_gconvtrain.hip takes: 4 channels per group with an even number of groups, or a multiple of 8 up
    to 256."""
    if groups < 1 or channels % groups:
        return False
    gw = channels // groups
    return (gw == 4 and groups % 2 == 0) or (gw % 8 == 0 and 8 <= gw <= MAX_WIDTH)


def supported(m):
    """``m`` is a grouped (neither dense nor depthwise) 3x3 / pad 1 / stride 1 | 2 convolution of a supported width."""
    return (isinstance(m, nn.Conv2d) and m.kernel_size == (3, 3) and m.padding == (1, 1) and m.dilation == (1, 1)
            and m.stride in ((1, 1), (2, 2)) and m.padding_mode == "zeros" and m.in_channels == m.out_channels
            and 1 < m.groups < m.in_channels and width_supported(m.in_channels, m.groups))


def image_shape(channels, groups):
    """-> (groups', gw', RB, KS) of the grouped image (include/ssdk.h): 4-wide groups merged into pairs."""
    gw = channels // groups
    if gw == 4:
        groups, gw = groups // 2, 8
    return groups, gw, (gw + 15) // 16, (9 * gw + 31) // 32


def pack_grouped_frag_dgrad(w, groups):
    """The grouped image of the INPUT-GRADIENT weights of a grouped 3x3 convolution: ``w`` KRSC [C][3][3][gw] as for
    fused_conv.pack_grouped_frag; per group the matrix is transposed (rows = input channels, k = tap' * gw + co) and the taps
    are flipped, W'[g][ci][ky][kx][co] = W[g][co][2 - ky][2 - kx][ci], so that at stride 1 dx = conv(dy, W'), pad 1.  Pure
    layout, on the tensor's own device (CPU tensors too) -> (image, groups', gw') as pack_grouped_frag (4-wide groups merged)."""
    c, kh, kw, gw = (int(v) for v in w.shape)
    assert kh == 3 and kw == 3 and c == groups * gw, (tuple(w.shape), groups)
    wt = w.reshape(groups, gw, 3, 3, gw).flip(2, 3).permute(0, 4, 2, 3, 1).reshape(c, 3, 3, gw)
    return pack_grouped_frag(wt.contiguous(), groups)


def unpack_grouped_frag(img, groups, gw):
    """The layout of include/ssdk.h read backwards: image [groups * RB][KS][4][16][8] -> OIHW weights [groups * gw][gw][3][3]
    of a convolution with ``groups`` groups (the merged groups of a 4-wide layer come back as block-diagonal groups of 8)."""
    rb, ks = (gw + 15) // 16, (9 * gw + 31) // 32
    assert tuple(img.shape) == (groups * rb, ks, 4, 16, 8), tuple(img.shape)
    mat = img.permute(0, 3, 1, 2, 4).reshape(groups, rb * 16, ks * 32)
    w = mat[:, :gw, :9 * gw].reshape(groups, gw, 3, 3, gw)  # k = tap * gw + ci
    return w.permute(0, 1, 4, 2, 3).reshape(groups * gw, gw, 3, 3).contiguous()


def prepare_images(weight, groups, dtype, want_dgrad=True):
    """fp32 (or 16-bit) weight [C, gw, 3, 3] on a HIP device -> (forward image, input-gradient image | None) in ``dtype``, one
    launch."""
    c = int(weight.shape[0])
    ge, gwe, rb, ks = image_shape(c, groups)
    dev = weight.device
    w32 = weight.detach().float().contiguous()  # (a 16-bit weight survives the round trip exactly)
    fwd = torch.empty((ge * rb, ks, 4, 16, 8), device=dev, dtype=dtype)
    dg = torch.empty_like(fwd) if want_dgrad else None
    with torch.cuda.device(dev):
        N.check(N.lib.ssdk_gconv3x3_train_prepare(w32.data_ptr(), fwd.data_ptr(), None if dg is None else dg.data_ptr(), c, groups,
                                                  N.dtype_code(fwd), N.stream_ptr(dev)), "gconv3x3_train_prepare")
    return fwd, dg


# (a bias is added and reduced on torch: no registered backbone has one)
FAMILY = K.ImageFamily(name="gconv3x3_train", stats=STATS, kernel_bias=False, prepare=prepare_images,
                       dims=lambda n, cin, cout, h, w, groups, stride: (n, cin, h, w, groups, stride),
                       forward=N.lib.ssdk_gconv3x3_train_forward, dgrad=N.lib.ssdk_gconv3x3_train_dgrad,
                       wgrad=N.lib.ssdk_gconv3x3_train_wgrad, wgrad_workspace_bytes=N.lib.ssdk_gconv3x3_train_wgrad_workspace_bytes)


def grouped_conv3x3(x, weight, bias=None, stride=1, groups=1):
    """The native path, called explicitly: x 16-bit contiguous NCHW on a HIP device; differentiable."""
    return K.ImageConv3x3.apply(x, weight, bias, stride, groups, FAMILY)


class GroupedConv3x3(K.KernelConv2d):
    """``nn.Conv2d(C, C, 3, stride 1 | 2, pad 1, groups)`` whose 16-bit HIP-device forward / backward run on
    csrc/ssdk_gconvtrain.hip (same parameters, ``state_dict`` keys and initialisation); everything else is ``nn.Conv2d.forward``."""

    matches = staticmethod(supported)
    half_weight = True

    def _run(self, x, w):
        return K.ImageConv3x3.apply(x, w, self.bias, self.stride[0], self.groups, FAMILY)


def use_native_gconv(model):
    """Switch every grouped 3x3 ``nn.Conv2d`` of ``model`` that ``supported`` accepts to the kernel-backed subclass (in place; no
    new parameters, same ``state_dict``).  -> model; STATS["swapped"] counts the layers."""
    STATS["swapped"] += K.swap_layers(model, GroupedConv3x3)
    return model
