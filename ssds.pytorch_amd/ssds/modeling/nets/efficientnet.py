"""EfficientNet-B0 ... B5 feature extractors returning the feature maps named by ``outputs`` -- the interface of the
reference's ``ssds/modeling/nets/efficientnet.py`` (``EfficientEx.forward`` :264-276, factories :289-352).  The stage
table, the width / depth multipliers and the filter / repeat rounding are the reference's (:133-166); parameter names
follow its layout (``conv1.{0,1}``, ``stage{1..7}.{i}.conv.{...}``, the squeeze-excite convolutions under ``.se.{1,3}``;
the Sequential indices inside ``conv`` are one lower in the expand-free first block) so reference checkpoints load.  The
classifier tail (``head_conv``, ``classifier``; reference :191-196) is not instantiated.

Eval on a HIP device runs as a recorded plan (planner.record_efficientnet): the expand 1x1 on the dense kernels, the rest
of every block -- depthwise k x k, squeeze-excite gate, gated projection -- on csrc/ssdk_mbse.hip.  In the training step
the 3x3 depthwise convolutions, the 1x1 convolutions and the BatchNorms run on their kernels through the Solver's class swaps;
the 5x5 depthwise convolution and SiLU + squeeze-excite run on csrc/ssdk_mbconvtrain.hip through a swap of the BLOCK's class
(layers/mbconvtrain.py), so these modules stay what they are."""
import math

import torch
import torch.nn as nn

from ssds.modeling.layers.dwconv import make_conv2d

from .rutils import register


class Swish(nn.SiLU):
    """x * sigmoid(x) (reference :28-33), as a parameter-free nn.SiLU so that fused_conv._act_name recognises it."""

    def __init__(self, *args, **kwargs):
        super(Swish, self).__init__()


class PlainConv2d(nn.Conv2d):
    """An ``nn.Conv2d`` that the training Solver's class swaps (``type(m) is nn.Conv2d``) pass over: the 5x5 depthwise
    convolutions and the squeeze-excite convolutions on 1x1 maps.  Their training kernels are reached through the block
    (layers/mbconvtrain.TrainMBConvBlock reads these modules' parameters); called as modules they run on PyTorch-ROCm."""


class ConvBNReLU(nn.Sequential):
    def __init__(self, in_planes, out_planes, kernel_size, stride=1, groups=1):
        padding = (kernel_size - 1) // 2
        if groups > 1 and kernel_size != 3:
            conv = PlainConv2d(in_planes, out_planes, kernel_size, stride, padding=padding, groups=groups, bias=False)
        else:
            conv = make_conv2d(in_planes, out_planes, kernel_size, stride, padding, groups=groups, bias=False)
        super(ConvBNReLU, self).__init__(conv, nn.BatchNorm2d(out_planes), Swish())


class SqueezeExcitation(nn.Module):
    def __init__(self, in_planes, reduced_dim):
        super(SqueezeExcitation, self).__init__()
        self.se = nn.Sequential(
            nn.AdaptiveAvgPool2d(1),
            PlainConv2d(in_planes, reduced_dim, 1),
            Swish(),
            PlainConv2d(reduced_dim, in_planes, 1),
            nn.Sigmoid(),
        )

    def forward(self, x):
        return x * self.se(x)


class MBConvBlock(nn.Module):
    """(1x1 expand + BN + SiLU) -> k x k depthwise + BN + SiLU -> squeeze-excite -> 1x1 linear projection + BN (+ x)."""

    def __init__(self, in_planes, out_planes, expand_ratio, kernel_size, stride, reduction_ratio=4, drop_connect_rate=0.2):
        super(MBConvBlock, self).__init__()
        assert stride in (1, 2) and kernel_size in (3, 5)
        self.drop_connect_rate = drop_connect_rate
        self.use_residual = in_planes == out_planes and stride == 1
        hidden_dim = in_planes * expand_ratio
        reduced_dim = max(1, int(in_planes / reduction_ratio))
        layers = []
        if in_planes != hidden_dim:
            layers.append(ConvBNReLU(in_planes, hidden_dim, 1))
        layers += [
            ConvBNReLU(hidden_dim, hidden_dim, kernel_size, stride=stride, groups=hidden_dim),
            SqueezeExcitation(hidden_dim, reduced_dim),
            nn.Conv2d(hidden_dim, out_planes, 1, bias=False),
            nn.BatchNorm2d(out_planes),
        ]
        self.conv = nn.Sequential(*layers)

    def parts(self):
        """-> (expand ConvBNReLU | None, depthwise ConvBNReLU, SqueezeExcitation, projection conv, projection BN)."""
        mods = list(self.conv.children())
        expand = mods[0] if len(mods) == 5 else None
        dw, se, proj, bn = mods[-4:]
        return expand, dw, se, proj, bn

    def _drop_connect(self, x):
        if not self.training:
            return x
        keep_prob = 1.0 - self.drop_connect_rate
        mask = (keep_prob + torch.rand(x.size(0), 1, 1, 1, device=x.device)).floor()  # per sample (reference :116-124)
        return x.div(keep_prob) * mask.to(x.dtype)

    def forward(self, x):
        if self.use_residual:
            return x + self._drop_connect(self.conv(x))
        return self.conv(x)


def _make_divisible(value, divisor=8):
    new_value = max(divisor, int(value + divisor / 2) // divisor * divisor)
    if new_value < 0.9 * value:
        new_value += divisor
    return new_value


def _round_filters(filters, width_mult):
    if width_mult == 1.0:
        return filters
    return int(_make_divisible(filters * width_mult))


def _round_repeats(repeats, depth_mult):
    if depth_mult == 1.0:
        return repeats
    return int(math.ceil(depth_mult * repeats))


# t (expand ratio), c (output channels), n (repeats), s (stride of the first block), k (depthwise kernel)
_SETTINGS = [[1, 16, 1, 1, 3], [6, 24, 2, 2, 3], [6, 40, 2, 2, 5], [6, 80, 3, 2, 3], [6, 112, 3, 1, 5], [6, 192, 4, 2, 5],
             [6, 320, 1, 1, 3]]
# name: (width multiplier, depth multiplier)
_VARIANTS = {"EfficientNetB0": (1.0, 1.0), "EfficientNetB1": (1.0, 1.1), "EfficientNetB2": (1.1, 1.2),
             "EfficientNetB3": (1.2, 1.4), "EfficientNetB4": (1.4, 1.8), "EfficientNetB5": (1.6, 2.2)}


class EfficientEx(nn.Module):
    """``forward(x)`` -> list of the feature maps of the levels in ``outputs`` (level j = ``stage{j}``, j = 1 ... 7),
    stopping after the deepest requested level."""

    def __init__(self, width_mult=1.0, depth_mult=1.0, outputs=[7]):
        super(EfficientEx, self).__init__()
        self.settings = _SETTINGS
        self.outputs = outputs
        self.depth_mult = depth_mult
        in_channels = _round_filters(32, width_mult)
        self.conv1 = ConvBNReLU(3, in_channels, 3, stride=2)
        self.out_channels = {}
        for j, (t, c, n, s, k) in enumerate(self.settings):
            out_channels = _round_filters(c, width_mult)
            stage = []
            for i in range(_round_repeats(n, depth_mult)):
                stage.append(MBConvBlock(in_channels, out_channels, expand_ratio=t, stride=s if i == 0 else 1, kernel_size=k))
                in_channels = out_channels
            self.add_module("stage{}".format(j + 1), nn.Sequential(*stage))
            self.out_channels[j + 1] = out_channels
        for m in self.modules():  # reference :198-212
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out")
                if m.bias is not None:
                    nn.init.zeros_(m.bias)
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.ones_(m.weight)
                nn.init.zeros_(m.bias)

    def initialize(self):
        """The reference downloads ImageNet weights here (:235-262).  There is no network on the target systems: pretrained
        weights are loaded explicitly through ``ssds.core.checkpoint.resume_checkpoint`` (cfg.RESUME_CHECKPOINT) instead."""
        return None

    def forward(self, x):
        x = self.conv1(x)
        outputs = []
        for j in range(len(self.settings)):
            level = j + 1
            if level > max(self.outputs):
                break
            x = getattr(self, "stage{}".format(level))(x)
            if level in self.outputs:
                outputs.append(x)
        return outputs


@register
def EfficientNetB0(outputs, **kwargs):
    return EfficientEx(*_VARIANTS["EfficientNetB0"], outputs=outputs)


@register
def EfficientNetB1(outputs, **kwargs):
    return EfficientEx(*_VARIANTS["EfficientNetB1"], outputs=outputs)


@register
def EfficientNetB2(outputs, **kwargs):
    return EfficientEx(*_VARIANTS["EfficientNetB2"], outputs=outputs)


@register
def EfficientNetB3(outputs, **kwargs):
    return EfficientEx(*_VARIANTS["EfficientNetB3"], outputs=outputs)


@register
def EfficientNetB4(outputs, **kwargs):
    return EfficientEx(*_VARIANTS["EfficientNetB4"], outputs=outputs)


@register
def EfficientNetB5(outputs, **kwargs):
    return EfficientEx(*_VARIANTS["EfficientNetB5"], outputs=outputs)
