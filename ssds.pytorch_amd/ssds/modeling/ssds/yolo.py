"""YOLOv3 (https://arxiv.org/abs/1804.02767) and YOLOv4 (https://arxiv.org/abs/2004.10934) detector heads -- constructor,
``add_extras`` factories, module names (``transforms``, ``extras``, ``fpn.{k}.top-down-*`` / ``bottom-up-*``, ``loc``, ``conf``),
``state_dict`` key order and forward contract of the reference's ``ssds/modeling/ssds/yolo.py`` (YOLOV3 :10-158, SPPModule
:161-184, PANModule :187-247, YOLOV4 :250-394).

YOLOv3 walks the backbone maps from the smallest up: a 3x3 ``transforms[i]`` on the coarser result, nearest x2, channel
concatenation BEHIND the backbone map, then ``extras[i]`` (1x1 to half width + 3x3).  YOLOv4 first narrows every backbone map with a
3x3 ``transforms[i]`` -- the last one through the SPP block ``cat(x, maxpool5(x), maxpool9(x), maxpool13(x))`` -- and then runs the
stacked PAN modules: the same top-down walk, and a bottom-up walk of stride-2 3x3 + concatenation at the same size.  Both only run
on maps that are exact halves of each other; anything else fails in ``torch.cat``, as in the reference.

MI355X execution (eval, 16-bit, HIP device): backbone, neck and heads are one recorded plan (layers/planner.py
``build_yolov3_plan`` / ``build_yolov4_plan``).  The two operations the plan had no op for are one launch each of
csrc/ssdk_cat.hip: ``ssdk_cat2`` writes ``a || nearest_x2(b)`` without ever storing the upsampled tensor, ``ssdk_spp`` computes
the three pools from one staging of ``x``.  Training is the module path around the convolution layers that
ssds/utils/train_ddp.py swaps for kernel-backed ones; with the ``native_cat`` flag (layers/cattrain.py ``use_native_cat``) the
concatenations and the SPP block run forward and backward on csrc/ssdk_cattrain.hip, and without it -- or for operands the kernels
do not take -- on torch's ``cat`` / ``interpolate`` / ``max_pool2d`` autograd."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from ssds.modeling.layers.basic_layers import ConvBNReLU, ConvBNReLUx2

from .shelf import Head
from .ssdsbase import NeckPlanMixin, SSDSBase


def _count_fallback(f0, training):
    """The plan refused this model / these maps in a setting where it would have run: said, not hidden."""
    if not training and f0.is_cuda and f0.dtype in (torch.bfloat16, torch.float16):
        from ssds.modeling.layers import fused_conv as FC

        if FC.fused_enabled():
            FC.STATS["torch_fallback_layers"] += 1


def _cat(native, a, b, up):
    """cat((a, nearest_x2(b) if up else b), 1): on csrc/ssdk_cattrain.hip when ``native`` and the operands meet its contract."""
    if native:
        from ssds.modeling.layers import cattrain

        y = cattrain.try_cat2(a, b, cattrain.UP2 if up else cattrain.SAME)
        if y is not None:
            return y
    return torch.cat((a, F.interpolate(b, scale_factor=2, mode="nearest") if up else b), dim=1)


def _refuse(layer):
    raise ValueError("{} does not support by YOLO".format(layer))


class YOLOV3(NeckPlanMixin, SSDSBase):
    native_cat = False  # layers/cattrain.py use_native_cat: the concatenations of the training step on csrc/ssdk_cattrain.hip

    def __init__(self, backbone, extras, head, num_classes):
        super(YOLOV3, self).__init__(backbone, num_classes)
        self.transforms = nn.ModuleList(extras[0])
        self.extras = nn.ModuleList(extras[1])
        self.loc = nn.ModuleList(head[0])
        self.conf = nn.ModuleList(head[1])
        self.initialize()

    def initialize(self):
        self.backbone.initialize()
        self.transforms.apply(self.initialize_extra)
        self.extras.apply(self.initialize_extra)
        self.loc.apply(self.initialize_head)
        self.conf.apply(self.initialize_head)
        for c in self.conf:
            c[-1].apply(self.initialize_prior)

    def _build_neck_plan(self, features, image=None):
        from ssds.modeling.layers.planner import build_yolov3_plan

        return build_yolov3_plan(self, features, image=image)

    def forward(self, x):
        out = self._full_native(x)  # planned backbone: image -> heads is one plan
        if out is not None:
            return out
        features = list(self.backbone(x))
        out = self._neck_native(features)  # eval on a HIP device: top-down chain, extras, heads = one plan
        if out is not None:
            return out
        _count_fallback(features[0], self.training)
        n = len(features)
        raw_last = xx = features[-1]
        for i in range(n - 1, -1, -1):
            if i != n - 1:
                xx = _cat(self.native_cat, features[i], self.transforms[i](xx), True)
            xx = self.extras[i](xx)
            features[i] = xx
        # the first string extra reads the RAW last backbone map, later ones the previous extra (reference yolo.py:75-81)
        for i in range(n, len(self.loc)):
            xx = self.extras[i](raw_last if i == n else xx)
            features.append(xx)
        loc = [l(f) for f, l in zip(features, self.loc)]
        conf = [c(f) for f, c in zip(features, self.conf)]
        if not self.training:
            conf = [c.sigmoid() for c in conf]
        return tuple(loc), tuple(conf)

    @staticmethod
    def add_extras(feature_layer, mbox, num_classes):
        """ints -> backbone output: ``ConvBNReLUx2`` at depth -> depth / 2 on the last one, on the others a 3x3 transform of the
        coarser level to depth / 2 and ``ConvBNReLUx2`` on the 1.5 depth wide concatenation; a two-element depth ``[in, out]``
        names both widths; ``"Conv:S"`` -> a stride-2 ``ConvBNReLU`` on the width before it; a ``Head`` pair per level."""
        nets_outputs, transform_layers, extra_layers, loc_layers, conf_layers = [], [], [], [], []
        last_int_layer = [layer for layer in feature_layer[0] if isinstance(layer, int)][-1]
        in_channels = None
        for layer, depth, box in zip(feature_layer[0], feature_layer[1], mbox):
            pair = isinstance(depth, list)
            if isinstance(layer, int):
                nets_outputs.append(layer)
                if layer == last_int_layer:
                    extra_layers += [ConvBNReLUx2(depth[0], depth[1], 3) if pair else ConvBNReLUx2(depth, depth // 2, 3)]
                else:
                    prev_depth = feature_layer[1][feature_layer[0].index(layer) + 1]
                    if pair:
                        transform_layers += [ConvBNReLU(prev_depth[1], depth[0] // 2, 3)]
                        extra_layers += [ConvBNReLUx2(int(depth[0] * 1.5), depth[1], 3)]
                    else:
                        transform_layers += [ConvBNReLU(prev_depth // 2, depth // 2, 3)]
                        extra_layers += [ConvBNReLUx2(int(depth * 1.5), depth // 2, 3)]
            elif layer == "Conv:S":
                extra_layers += [ConvBNReLU(in_channels, depth, 3, stride=2)]
            else:
                _refuse(layer)
            in_channels = depth[1] if pair else (depth // 2 if isinstance(layer, int) else depth)
            loc_layers += [Head(in_channels, box * 4)]
            conf_layers += [Head(in_channels, box * num_classes)]
            in_channels = depth[0] if pair else depth
        return nets_outputs, (transform_layers, extra_layers), (loc_layers, conf_layers)


class SPPModule(nn.Module):
    """cat(x, pool_5(x), pool_9(x), ... ) over ``num_levels`` stride-1 pools of windows 4 i + 5 with padding k // 2 (reference
    yolo.py:161-184); ``pool_type`` "max_pool" or anything else for average pooling.  No parameters."""

    native_cat = False  # layers/cattrain.py use_native_cat (three max-pool levels only)

    def __init__(self, num_levels, pool_type="max_pool"):
        super(SPPModule, self).__init__()
        self.num_levels = num_levels
        self.pool_type = pool_type

    def forward(self, x):
        if self.native_cat and self.num_levels == 3 and self.pool_type == "max_pool":
            from ssds.modeling.layers import cattrain

            y = cattrain.try_spp(x)
            if y is not None:
                return y
        pool = F.max_pool2d if self.pool_type == "max_pool" else F.avg_pool2d
        out = [x]
        for i in range(self.num_levels):
            k = 4 * (i + 1) + 1
            out.append(pool(x, kernel_size=k, stride=1, padding=(k - 1) // 2))
        return torch.cat(out, dim=1)


class PANModule(nn.Module):
    """One path-aggregation block over ``len(channels)`` levels, largest map first (reference yolo.py:187-247): top-down
    ``cat(x[i-1], up2(conv3x3(x[i])))`` + ``ConvBNReLUx2``, then bottom-up ``cat(x[i+1], conv3x3/s2(x[i]))`` + ``ConvBNReLUx2``."""

    native_cat = False  # layers/cattrain.py use_native_cat

    def __init__(self, channels):
        super(PANModule, self).__init__()
        self.levels = len(channels)
        for i in range(self.levels - 1, 0, -1):
            self.add_module("top-down-{}-to-{}".format(i, i - 1), ConvBNReLU(channels[i], channels[i - 1]))
            self.add_module("top-down-{}".format(i - 1), ConvBNReLUx2(channels[i - 1] * 2, channels[i - 1]))
        for i in range(0, self.levels - 1):
            self.add_module("bottom-up-{}-to-{}".format(i, i + 1), ConvBNReLU(channels[i], channels[i + 1], stride=2))
            self.add_module("bottom-up-{}".format(i + 1), ConvBNReLUx2(channels[i + 1] * 2, channels[i + 1]))
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.xavier_uniform_(m.weight)
                if m.bias is not None:
                    nn.init.constant_(m.bias, val=0)

    def forward(self, xx):
        assert len(xx) == self.levels
        xx = list(xx)
        for i in range(self.levels - 1, 0, -1):
            up = getattr(self, "top-down-{}-to-{}".format(i, i - 1))(xx[i])
            xx[i - 1] = getattr(self, "top-down-{}".format(i - 1))(_cat(self.native_cat, xx[i - 1], up, True))
        for i in range(0, self.levels - 1):
            down = getattr(self, "bottom-up-{}-to-{}".format(i, i + 1))(xx[i])
            xx[i + 1] = getattr(self, "bottom-up-{}".format(i + 1))(_cat(self.native_cat, xx[i + 1], down, False))
        return xx


class YOLOV4(NeckPlanMixin, SSDSBase):
    def __init__(self, backbone, extras, head, num_classes):
        super(YOLOV4, self).__init__(backbone, num_classes)
        self.transforms = nn.ModuleList(extras[0])
        self.extras = nn.ModuleList(extras[1])
        self.fpn = extras[2]
        self.loc = nn.ModuleList(head[0])
        self.conf = nn.ModuleList(head[1])
        self.initialize()

    def initialize(self):
        self.backbone.initialize()
        self.transforms.apply(self.initialize_extra)
        self.fpn.apply(self.initialize_extra)
        self.extras.apply(self.initialize_extra)
        self.loc.apply(self.initialize_head)
        self.conf.apply(self.initialize_head)
        for c in self.conf:
            c[-1].apply(self.initialize_prior)

    def _build_neck_plan(self, features, image=None):
        from ssds.modeling.layers.planner import build_yolov4_plan

        return build_yolov4_plan(self, features, image=image)

    def forward(self, x):
        out = self._full_native(x)  # planned backbone: image -> heads is one plan
        if out is not None:
            return out
        features = list(self.backbone(x))
        out = self._neck_native(features)  # eval on a HIP device: transforms + SPP, PAN stacks, extras, heads = one plan
        if out is not None:
            return out
        _count_fallback(features[0], self.training)
        for i, t in enumerate(self.transforms):
            features[i] = t(features[i])
        features = list(self.fpn(features))
        x = features[-1]
        for e in self.extras:
            x = e(x)
            features.append(x)
        loc = [l(f) for f, l in zip(features, self.loc)]
        conf = [c(f) for f, c in zip(features, self.conf)]
        if not self.training:
            conf = [c.sigmoid() for c in conf]
        return tuple(loc), tuple(conf)

    @staticmethod
    def add_extras(feature_layer, mbox, num_classes):
        """ints -> backbone output narrowed to depth / 2 by a 3x3 transform, the last one as ``ConvBNReLU, SPPModule(3),
        ConvBNReLU(2 depth -> depth / 2)``; ``"Conv:S"`` -> a stride-2 ``ConvBNReLU`` behind the last level; a ``Head`` pair per
        level; ``feature_layer[2]`` (default 1) stacked ``PANModule``s at the narrowed widths."""
        nets_outputs, transform_layers, extra_layers, loc_layers, conf_layers, fpn_channels = [], [], [], [], [], []
        last_int_layer = [layer for layer in feature_layer[0] if isinstance(layer, int)][-1]
        in_channels = None
        for layer, depth, box in zip(feature_layer[0], feature_layer[1], mbox):
            if isinstance(layer, int):
                nets_outputs.append(layer)
                fpn_channels.append(depth // 2)
                if layer == last_int_layer:
                    transform_layers += [nn.Sequential(ConvBNReLU(depth, depth // 2, 3), SPPModule(3),
                                                       ConvBNReLU(depth * 2, depth // 2, 3))]
                else:
                    transform_layers += [ConvBNReLU(depth, depth // 2, 3)]
            elif layer == "Conv:S":
                extra_layers += [ConvBNReLU(in_channels, depth, 3, stride=2)]
            else:
                _refuse(layer)
            in_channels = depth // 2 if isinstance(layer, int) else depth
            loc_layers += [Head(in_channels, box * 4)]
            conf_layers += [Head(in_channels, box * num_classes)]
        num_stack = 1 if len(feature_layer) == 2 else feature_layer[2]
        fpn = nn.Sequential(*[PANModule(fpn_channels) for _ in range(num_stack)])
        return nets_outputs, (transform_layers, extra_layers, fpn), (loc_layers, conf_layers)
