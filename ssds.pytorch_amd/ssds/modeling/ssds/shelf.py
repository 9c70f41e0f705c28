"""SSDShelf (ShelfNet-style neck, https://arxiv.org/abs/1811.11254, + per-level heads) -- constructor, ``add_extras``
factory, module names (``transforms``, ``shelf_head.{decoder0,encoder0,decoder1}.{blockN,convN}``, ``loc``, ``conf``),
``state_dict`` key order and forward contract of the reference's ``ssds/modeling/ssds/shelf.py`` (SharedBlock :10-35,
ShelfPyramid :38-62, Head :65-70, SSDShelf :73-156).

The neck is three pyramids over the 1x1-transformed backbone maps: a decoder walks from the smallest map up
(``ConvTranspose2d(3, stride 2, padding 1)`` + the next map, then a ``SharedBlock``), an encoder walks back down
(``ConvBNReLU(3, stride 2)`` + the next map), a second decoder walks up again.  The transposed convolution has no output
padding, so an ``h x w`` map becomes ``(2h - 1) x (2w - 1)``: the model only runs on pyramids whose every level is exactly
``2h - 1`` of the next (image sides of the form ``2^k + 1``); anything else fails in the add, as in the reference.

MI355X execution (eval, 16-bit, HIP device): the whole neck and the heads are one recorded plan
(layers/planner.py ``build_shelf_plan``) -- the transposed convolution + bias + skip add is ONE launch of
csrc/ssdk_convt.hip, each ``SharedBlock`` two fused 3x3 launches from the same weight (BatchNorm 1 + ReLU; BatchNorm 2 +
skip + ReLU).  Training (utils/train_ddp.Solver): under ``SSDK_CONVT_TRAIN=1`` the transposed convolution + bias + skip add, its input
gradient and its weight + bias gradient run on csrc/ssdk_convttrain.hip (layers/convttrain.py ``ShelfConvT``, an in-place class swap);
the switch is off by default, because the step measured slower with it, and ``nn.ConvTranspose2d`` then runs on
PyTorch-ROCm.  ``Dropout2d`` stays torch's either way (one broadcast multiply by an [N, C, 1, 1] mask, drawn from torch's generator)."""
from collections import OrderedDict

import torch
import torch.nn as nn

from ssds.modeling.layers.basic_layers import ConvBNReLU
from ssds.modeling.layers.layers_parser import parse_feature_layer

from .ssdsbase import NeckPlanMixin, SSDSBase


class SharedBlock(nn.Module):
    """Residual block whose two 3x3 convolutions are the SAME ``conv1`` (reference shelf.py:10-35):
    relu2(bn2(conv1(drop(relu1(bn1(conv1(x)))))) + x)."""

    def __init__(self, planes):
        super(SharedBlock, self).__init__()
        self.planes = planes
        self.conv1 = nn.Conv2d(planes, planes, kernel_size=3, stride=1, padding=1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.relu1 = nn.ReLU(inplace=True)
        self.drop = nn.Dropout2d(p=0.25)
        self.bn2 = nn.BatchNorm2d(planes)
        self.relu2 = nn.ReLU(inplace=True)

    def forward(self, x):
        out = self.drop(self.relu1(self.bn1(self.conv1(x))))
        out = self.bn2(self.conv1(out))
        return self.relu2(out + x)


class ShelfPyramid(nn.Module):
    """One walk over the levels (reference shelf.py:38-62): ``block0`` on the first map, then per level
    ``block_i(conv_i(previous) + map_i)``.  ``conv`` is the resampling step between levels: ``nn.ConvTranspose2d`` (3 x 3,
    stride 2, padding 1, bias; decoder) or ``ConvBNReLU`` (3 x 3, stride 2; encoder).  Returns the levels in REVERSED order,
    i.e. ready to be the next pyramid's input."""

    def __init__(self, settings, conv=nn.ConvTranspose2d, block=SharedBlock):
        super(ShelfPyramid, self).__init__()
        extra = {"padding": 1, "bias": True} if conv is nn.ConvTranspose2d else {}
        for i, depth in enumerate(settings):
            self.add_module("block{}".format(i), block(depth))
            if i > 0:
                self.add_module("conv{}".format(i), conv(settings[i - 1], depth, kernel_size=3, stride=2, **extra))

    def forward(self, xx):
        out, x = [], xx[0]
        for i in range(len(xx)):
            if i > 0:
                conv = getattr(self, "conv{}".format(i))
                if getattr(conv, "takes_skip", False):  # layers/convttrain.ShelfConvT: the add rides on the forward kernel
                    x = conv(x, skip=xx[i])
                else:
                    x = conv(x) + xx[i]
            x = getattr(self, "block{}".format(i))(x)
            out.append(x)
        return out[::-1]


class Head(nn.Sequential):
    """ConvBNReLU(C, C, 3) + Conv2d(C, out_planes, 3) of one level (reference shelf.py:65-70)."""

    def __init__(self, in_channels, out_planes):
        super(Head, self).__init__(ConvBNReLU(in_channels, in_channels, 3), nn.Conv2d(in_channels, out_planes, 3, padding=1))

    # the output convolution's parameters under the names SSD's bare head convolutions have (``for m in model.conf: m.bias``:
    # bench.py's seeded score prior); plain aliases, not registered a second time
    @property
    def weight(self):
        return self[-1].weight

    @property
    def bias(self):
        return self[-1].bias


class SSDShelf(NeckPlanMixin, SSDSBase):
    def __init__(self, backbone, extras, head, num_classes):
        super(SSDShelf, self).__init__(backbone, num_classes)
        self.transforms = nn.ModuleList(extras[0])
        self.shelf_head = nn.Sequential(extras[1])
        self.loc = nn.ModuleList(head[0])
        self.conf = nn.ModuleList(head[1])
        self.initialize()

    def initialize(self):
        self.backbone.initialize()
        self.transforms.apply(self.initialize_extra)
        self.shelf_head.apply(self.initialize_extra)
        self.loc.apply(self.initialize_head)
        self.conf.apply(self.initialize_head)
        for c in self.conf:
            c[-1].apply(self.initialize_prior)

    def _build_neck_plan(self, features, image=None):
        from ssds.modeling.layers.planner import build_shelf_plan

        return build_shelf_plan(self, features, image=image)

    def forward(self, x):
        out = self._full_native(x)  # planned backbone: image -> heads is one plan
        if out is not None:
            return out
        features = self.backbone(x)
        out = self._neck_native(features)  # eval on a HIP device: transforms, the three pyramids, heads = one plan
        if out is not None:
            return out
        f0 = features[0]
        if not self.training and f0.is_cuda and f0.dtype in (torch.bfloat16, torch.float16):
            from ssds.modeling.layers import fused_conv as FC

            if FC.fused_enabled():  # the plan refused this model / these maps: said, not hidden
                FC.STATS["torch_fallback_layers"] += 1
        features = [self.transforms[i](f) for i, f in enumerate(features)]
        features = self.shelf_head(features[::-1])
        for i in range(len(features), len(self.transforms)):
            features.append(self.transforms[i](features[-1]))
        loc = [l(f) for f, l in zip(features, self.loc)]
        conf = [c(f) for f, c in zip(features, self.conf)]
        if not self.training:
            conf = [c.sigmoid() for c in conf]
        return tuple(loc), tuple(conf)

    @staticmethod
    def add_extras(feature_layer, mbox, num_classes):
        """ints -> backbone output + 1x1 transform (bias, no BN); strings -> ``parse_feature_layer`` on the previous map; a
        ``Head`` pair per level; the three pyramids at the BACKBONE widths (reference shelf.py:125-156: a two-element depth
        ``[in, out]`` with ``in != out`` therefore does not run there either)."""
        nets_outputs, transform_layers, loc_layers, conf_layers, shelf_depths = [], [], [], [], []
        in_channels = None
        for layer, depth, box in zip(feature_layer[0], feature_layer[1], mbox):
            if isinstance(layer, int):
                if isinstance(depth, list):
                    if len(depth) == 2:
                        in_channels, depth = depth
                else:
                    in_channels = depth
                nets_outputs.append(layer)
                shelf_depths.append(in_channels)
                transform_layers += [nn.Conv2d(in_channels, depth, 1)]
            else:
                transform_layers += parse_feature_layer(layer, in_channels, depth)
                in_channels = depth
            loc_layers += [Head(in_channels, box * 4)]
            conf_layers += [Head(in_channels, box * num_classes)]
        shelf_head = OrderedDict([
            ("decoder0", ShelfPyramid(shelf_depths[::-1])),
            ("encoder0", ShelfPyramid(shelf_depths, conv=ConvBNReLU)),
            ("decoder1", ShelfPyramid(shelf_depths[::-1])),
        ])
        return nets_outputs, (transform_layers, shelf_head), (loc_layers, conf_layers)
