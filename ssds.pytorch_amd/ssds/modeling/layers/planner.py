"""Records the eval forward of a detector as a ``ConvPlan`` (fused_conv.py): every Conv-BN-activation
group becomes one descriptor of the fused HIP kernels, block-level residual adds ride in the epilogue of
the projecting 1x1 conv, and the loc | conf convs of each level become one split-output GEMM.

Covered: MobileNet v1/v2 backbones (nets/mobilenet.py), the SSD extras and heads (ssds/ssd.py) -- i.e. the
network of BASELINE configs 1, 2 and 4 -- and the FPN / BiFPN / Shelf / YOLOv3 / YOLOv4 necks with their towers or heads
(ssds/fpn.py, ssds/bifpn.py, ssds/shelf.py, ssds/yolo.py; configs 3 and 5) on top of backbone feature maps handed in as external inputs.  Anything else
raises ``PlanUnsupported`` and the caller runs the module-by-module path instead (and says so in
``fused_conv.STATS``)."""
import torch.nn as nn

import os

import functools

from .fused_conv import (ConvPack, ConvPlan, ConvTPack, DenseLayerPack, MbPack, MbSePack, ShuffleDownPack, ShuffleUnitPack, StemPack,
                         allow_padded_maps, cat_supported, conv_kind, denselayer_enabled, dkres_supported, fold_norm, in_padded_maps_scope, pack_heads,
                         padded_maps_scope, sequential_groups, shuffleunit_enabled, value_segs, xpair_supported)
from ssds import _native as N


class PlanUnsupported(Exception):
    pass


def _one_recording(build):
    """A plan builder runs inside ``fused_conv.padded_maps_scope``: a backbone that hands out zero-padded maps (ShuffleNetV2) lets the
    dense convolutions behind it read them, for this recording only."""
    @functools.wraps(build)
    def wrapped(*a, **kw):
        with padded_maps_scope():
            return build(*a, **kw)
    return wrapped


def flatten(module):
    """nn.Sequential tree -> flat list of leaf modules in execution order."""
    out = []
    for m in module.children():
        if isinstance(m, nn.Sequential):
            out.extend(flatten(m))
        else:
            out.append(m)
    return out


def groups_of(module):
    seq = nn.Sequential(*flatten(module))
    groups = sequential_groups(seq)
    if groups is None:
        raise PlanUnsupported("not a Conv-BN-act chain: {}".format(type(module).__name__))
    for conv, _, _ in groups:
        if conv_kind(conv) is None:
            raise PlanUnsupported("conv not covered by the HIP kernels: {}".format(conv))
    return groups


def record_chain(plan, val, module, residual=None, keep_input=False, lane=0):
    """Record the Conv-BN-act chain of ``module`` starting from value ``val``; the residual (if any, always
    the chain input) is added in the epilogue of the LAST conv.  Intermediate buffers are released as soon
    as they have been read; the chain input is released at the end unless ``keep_input``."""
    groups = groups_of(module)
    if residual is None and len(groups) == 2:  # an SSD extra layer on a small map: one launch (csrc/ssdk_xpair.hip)
        p1, p2 = (ConvPack(conv, bn, act, plan.dtype) for conv, bn, act in groups)
        if xpair_supported(p1, p2, val[3], val[4]):
            out = plan.xpair(val, p1, p2, lane=lane)
            if not keep_input:
                plan.release(val)
            return out
    cur = val
    for i, (conv, bn, act) in enumerate(groups):
        pack = ConvPack(conv, bn, act, plan.dtype)
        last = i == len(groups) - 1
        nxt = plan.conv(cur, pack, residual=residual if last else None, lane=lane)
        if cur is not val:
            plan.release(cur)
        cur = nxt
    if not keep_input:
        plan.release(val)
    return cur


def dconv_enabled():
    """SSDK_DCONV (default DCONV_DEFAULT): RFB extras on the recorded plan, their dilated 3x3 convolutions on csrc/ssdk_dconv.hip.
    Read at recording time."""
    return os.environ.get("SSDK_DCONV", DCONV_DEFAULT) != "0"


DCONV_DEFAULT = "1"


def _rfb_conv(plan, val, bc, what, residual=None, res_mode=0, scale=1.0):
    """One ``BasicConv`` of a BasicRFB block as one plan op; PlanUnsupported, naming the layer, for what no kernel takes."""
    conv, bn = bc.conv, bc.bn
    kind = conv_kind(conv)
    if kind == "dilated":
        d = conv.dilation[0]
        if not N.lib.ssdk_dconv3x3_supported(conv.in_channels, conv.out_channels, val[3], val[4], d, plan.dtype_code):
            raise PlanUnsupported("{}: ssdk_dconv3x3_supported refuses Cin={} Cout={} H={} W={} dilation={} dtype={}".format(
                what, conv.in_channels, conv.out_channels, val[3], val[4], d, plan.dtype_code))
    elif kind != "dense":
        raise PlanUnsupported("{}: conv not covered by the HIP kernels: {}".format(what, conv))
    if bn is not None and not isinstance(bn, nn.BatchNorm2d):
        raise PlanUnsupported("{}: BatchNorm2d expected behind the conv, found {}".format(what, type(bn).__name__))
    pack = ConvPack(conv, bn, "relu" if bc.relu is not None else "none", plan.dtype)
    if scale != 1.0:  # the block's ``out * scale`` rides in the folded BatchNorm
        ones = pack.scale if pack.scale is not None else pack.bias.new_ones(pack.bias.shape)
        pack.scale, pack.bias = ones * float(scale), pack.bias * float(scale)
    return plan.conv(val, pack, residual=residual, res_mode=res_mode, act="relu" if res_mode & 2 else None)


def record_rfb(plan, val, blk, keep_input=False):
    """One ``BasicRFB`` block (layers/rfb_layers.py) as ten ops, all in line: branch0 (1x1, 3x3 / stride s, dilated 3x3), branch1 (1x1,
    3x3, 3x3 / stride s, dilated 3x3), their concatenation (ssdk_cat2), the 1x1 / stride-s shortcut, and ConvLinear with the shortcut
    as its residual, the block's ``scale`` folded into its BatchNorm and the ReLU behind the add.  Intermediates are released as
    soon as they have been read; the input at the end unless ``keep_input``."""
    from .rfb_layers import BasicConv, BasicRFB

    name = type(blk).__name__
    if not isinstance(blk, BasicRFB):
        raise PlanUnsupported("block {} has no planner".format(name))
    if not dconv_enabled():
        raise PlanUnsupported("SSDK_DCONV=0: the RFB extras run on PyTorch-ROCm")
    cin = blk.shortcut.conv.in_channels
    if hasattr(val, "segs"):
        raise PlanUnsupported("{} behind a zero-padded map of {} channels".format(name, val[2]))
    if cin % 128:
        # i = in_planes // 8 -> 3 (i // 2) -> 2 i are all multiples of 8 exactly when in_planes is a multiple of 128
        raise PlanUnsupported("{} with in_planes = {}: the widths inside the block (in_planes // 8, 3 (in_planes // 16), in_planes // 4) "
                              "are multiples of 8 only when in_planes is a multiple of 128".format(name, cin))
    if val[2] != cin:
        raise PlanUnsupported("{} of {} input channels behind a map of {}".format(name, cin, val[2]))
    mods = list(blk.branch0) + list(blk.branch1) + [blk.ConvLinear, blk.shortcut]
    if len(blk.branch0) != 3 or len(blk.branch1) != 4 or not all(isinstance(m, BasicConv) for m in mods):
        raise PlanUnsupported("{}: branches of 3 and 4 BasicConv layers expected".format(name))
    ends = []
    for b, branch in enumerate((blk.branch0, blk.branch1)):
        cur = val
        for j, bc in enumerate(branch):
            nxt = _rfb_conv(plan, cur, bc, "{} branch{}.{}".format(name, b, j))
            if cur is not val:
                plan.release(cur)
            cur = nxt
        ends.append(cur)
    if tuple(ends[0][3:]) != tuple(ends[1][3:]):
        raise PlanUnsupported("{}: branches end on maps of different sizes: {} and {}".format(name, ends[0][3:], ends[1][3:]))
    why = cat_supported(ends[0][2], ends[1][2], ends[0][3], ends[0][4], False)
    if why:
        raise PlanUnsupported("{}: concatenation not covered by ssdk_cat2: {}".format(name, why))
    both = plan.cat(ends[0], ends[1])
    plan.release(ends[0])
    plan.release(ends[1])
    short = _rfb_conv(plan, val, blk.shortcut, name + " shortcut")
    out = _rfb_conv(plan, both, blk.ConvLinear, name + " ConvLinear", residual=short, res_mode=2, scale=blk.scale)
    plan.release(both)
    plan.release(short)
    if not keep_input:
        plan.release(val)
    return out


def record_extra(plan, val, module, keep_input=False):
    """One module made by ``layers_parser.parse_feature_layer``: a BasicRFB block on ``record_rfb``, everything else (the Conv-BN-ReLU
    chains) on ``record_chain``."""
    from .rfb_layers import BasicRFB

    if isinstance(module, BasicRFB):
        return record_rfb(plan, val, module, keep_input=keep_input)
    return record_chain(plan, val, module, keep_input=keep_input)


def record_mobilenet(plan, val, net, on_output=None):
    from ssds.modeling.nets.mobilenet import InvertedResidual, MobileNetEx

    if not isinstance(net, MobileNetEx):
        raise PlanUnsupported("backbone {} has no planner".format(type(net).__name__))
    fused_block = os.environ.get("SSDK_FUSED_BLOCK", "1") != "0"
    first_blk = net.layer1[0]
    stem_fused = False
    if fused_block and isinstance(first_blk, InvertedResidual) and not first_blk.use_res_connect:
        sg, bg = groups_of(net.conv1), groups_of(first_blk.conv)
        if MbPack.stem_supported(sg, bg):  # stem conv + expand-free first block: ONE launch from the image
            pk = MbPack(bg, False, plan.dtype, stem_group=sg[0])
            if pk.fp16_safe():  # (folded weights outside the fp16 range of the kernel's internals: layer by layer)
                cur = plan.mbconv(val, pk)
                stem_fused = True
    if not stem_fused:
        cur = record_chain(plan, val, net.conv1, keep_input=True)  # the image is not an arena buffer
    outputs = []
    for j in range(len(net.settings)):
        level = j + 1
        if level > max(net.outputs):
            break
        for bi, blk in enumerate(getattr(net, "layer{}".format(level))):
            if stem_fused and level == 1 and bi == 0:
                continue
            is_out_input = any(cur is o for o in outputs)
            if isinstance(blk, InvertedResidual):
                res = cur if blk.use_res_connect else None
                groups = groups_of(blk.conv)
                pk = MbPack(groups, blk.use_res_connect, plan.dtype) if fused_block and MbPack.supported(groups, blk.use_res_connect) else None
                if pk is not None and pk.fp16_safe():
                    nxt = plan.mbconv(cur, pk)  # whole block, 1 launch
                    if not is_out_input:
                        plan.release(cur)
                    cur = nxt
                else:
                    cur = record_chain(plan, cur, blk.conv, residual=res, keep_input=is_out_input)
            else:
                cur = record_chain(plan, cur, blk, keep_input=is_out_input)
        if level in net.outputs:
            outputs.append(cur)
            if on_output is not None:
                on_output(len(outputs) - 1, cur)
    return outputs


@_one_recording
def build_ssd_plan(model, x, features=None):
    """SSD (ssds/ssd.py) on a planned backbone (MobileNet, ResNet) -> finalized ConvPlan for inputs shaped like ``x``.  With
    ``features`` (and ``x`` None) the backbone's maps are the plan's external inputs, as for the necks (``_neck_inputs``): the extras
    and the heads alone."""
    if features is not None:
        plan, given = _neck_inputs(model, features, None)
    else:
        plan = ConvPlan(x.device, x.dtype, x.shape)

    def head(i, f, lane=None, position=None):
        # recorded right behind its feature map: the executor forks it onto the side stream, where it overlaps
        # the rest of the backbone / the extras chain (feature maps are never released, so that is safe)
        l, c = model.loc[i], model.conf[i]
        if conv_kind(l) != "dense" or conv_kind(c) != "dense":
            raise PlanUnsupported("head conv not covered")
        plan.head(f, pack_heads(l, c, plan.dtype), split=l.out_channels, act="none", act2="sigmoid", tag="both", lane=lane,
                  position=position)

    from ssds.modeling.nets.mobilenet import MobileNetEx

    # (Round 5 measured the mirror-image ordering -- extras chain + small heads as a side-stream run next to the two backbone-level
    #  heads -- at 60.9 / 62.4 k against 61.9 / 62.9 k img/s in line; the SSDK_SSD_TAIL_SIDE switch and its two recordings are
    #  gone in round 6: docs/HISTORY.md.)
    if features is not None:
        feats = list(given)
        for i, f in enumerate(feats):
            head(i, f)
    elif isinstance(model.backbone, MobileNetEx):
        feats = record_mobilenet(plan, plan.input_value(), model.backbone, on_output=head)
    else:
        feats = record_backbone(plan, plan.input_value(), model.backbone)
        for i, f in enumerate(feats):
            head(i, f)
    # The heads of the extras' levels are recorded BEHIND the extras chain, next to each other (outputs keep the level order):
    # they depend only on their feature maps, and the executor launches neighbouring small-map layers that do not read each
    # other's outputs as ONE kernel (ssdk_run_ops -> conv_smallmap_group_kernel: the 4x4 / 2x2 / 1x1 heads are chains of
    # dependent latencies with 128 / 32 / 8 workgroups each).  SSDK_HEAD_BALANCE=0: every head right behind its feature map.
    balance = os.environ.get("SSDK_HEAD_BALANCE", "1") != "0" and len(model.extras) > 1
    deferred = []
    for j, extra in enumerate(model.extras):
        feats.append(record_extra(plan, feats[-1], extra, keep_input=True))
        if balance:
            deferred.append((len(feats) - 1, feats[-1]))
        else:
            head(len(feats) - 1, feats[-1])
    for i, f in deferred:
        head(i, f, lane=0, position=i)
    return plan.finalize()


# --------------------------------------------------------------------------------------------------------------
# ResNet backbones (nets/resnet.py)
# --------------------------------------------------------------------------------------------------------------
def _pack(conv, bn, act, dtype, kinds=("dense",)):
    if conv_kind(conv) not in kinds:
        raise PlanUnsupported("conv not covered by the HIP kernels: {}".format(conv))
    return ConvPack(conv, bn, act, dtype)


def record_resnet(plan, val, net):
    """conv1/bn1/relu (7x7 stem kernel) -> maxpool -> layer1..4; every block ends in ONE launch that adds the
    identity and applies the ReLU in the epilogue of its last conv (res_mode bit 1)."""
    from ssds.modeling.nets.resnet import BasicBlock, Bottleneck, ResNet

    if not isinstance(net, ResNet):
        raise PlanUnsupported("backbone {} has no planner".format(type(net).__name__))
    if not StemPack.supported(net.conv1, net.bn1):
        raise PlanUnsupported("stem not covered")
    dt = plan.dtype
    cur = plan.stem7(val, StemPack(net.conv1, net.bn1, "relu", dt))
    pooled = plan.pool(cur)
    plan.release(cur)
    cur = pooled
    outputs = []
    for li, layer in enumerate([net.layer1, net.layer2, net.layer3, net.layer4]):
        level = li + 2
        if level > max(net.outputs):
            break
        for blk in layer:
            keep_cur = any(cur is o for o in outputs)
            idt = cur
            if blk.downsample is not None:
                dconv, dbn = blk.downsample[0], blk.downsample[1]
                idt = plan.conv(cur, _pack(dconv, dbn, "none", dt))
            if isinstance(blk, Bottleneck):
                o1 = plan.conv(cur, _pack(blk.conv1, blk.bn1, "relu", dt))
                o2 = plan.conv(o1, _pack(blk.conv2, blk.bn2, "relu", dt, kinds=("dense", "g16", "gany")))  # (ResNeXt: grouped)
                plan.release(o1)
                out = plan.conv(o2, _pack(blk.conv3, blk.bn3, "relu", dt), residual=idt, res_mode=2)
                plan.release(o2)
            elif isinstance(blk, BasicBlock):
                o1 = plan.conv(cur, _pack(blk.conv1, blk.bn1, "relu", dt))
                out = plan.conv(o1, _pack(blk.conv2, blk.bn2, "relu", dt), residual=idt, res_mode=2)
                plan.release(o1)
            else:
                raise PlanUnsupported("block {} has no planner".format(type(blk).__name__))
            if idt is not cur:
                plan.release(idt)
            if not keep_cur:
                plan.release(cur)
            cur = out
        if level in net.outputs:
            outputs.append(cur)
    return outputs


def record_regnet(plan, val, net):
    """RegNetX (nets/regnet.py): 3x3/s2 stem, then bottleneck blocks 1x1 -> grouped 3x3 (any supported group width,
    stride s) -> 1x1 whose last conv adds the (projected) skip and applies the ReLU in its epilogue."""
    from ssds.modeling.nets.regnet import RegNet

    if not isinstance(net, RegNet):
        raise PlanUnsupported("backbone {} has no planner".format(type(net).__name__))
    dt = plan.dtype
    cur = plan.conv(val, _pack(net.stem.conv, net.stem.bn, "relu", dt, kinds=("stem",)))
    outputs = []
    for i, stage in enumerate([net.s1, net.s2, net.s3, net.s4]):
        level = i + 1
        if level > max(net.outputs):
            break
        for blk in stage.children():
            keep_cur = any(cur is o for o in outputs)
            skip = cur
            if blk.proj_block:
                skip = plan.conv(cur, _pack(blk.proj, blk.bn, "none", dt))
            f = blk.f
            a = plan.conv(cur, _pack(f.a, f.a_bn, "relu", dt))
            b = plan.conv(a, _pack(f.b, f.b_bn, "relu", dt, kinds=("g16", "gany", "dense")))
            plan.release(a)
            out = plan.conv(b, _pack(f.c, f.c_bn, "relu", dt), residual=skip, res_mode=2)
            plan.release(b)
            if skip is not cur:
                plan.release(skip)
            if not keep_cur:
                plan.release(cur)
            cur = out
        if level in net.outputs:
            outputs.append(cur)
    return outputs


def record_efficientnet(plan, val, net):
    """EfficientNet (nets/efficientnet.py): 3x3/s2 stem + SiLU on the image-stem kernel, then per MBConv block the expand 1x1
    (SiLU; absent in the first block) as an ordinary conv and everything behind it as ONE mbse op (csrc/ssdk_mbse.hip) whose
    projection adds the block input in its epilogue.  The stem kernel exists for 16 / 32 / 64 output channels: B0 ... B2; the
    40- and 48-channel stems of B3 ... B5 are PlanUnsupported (the backbone then runs on PyTorch-ROCm, reported)."""
    from ssds.modeling.nets.efficientnet import EfficientEx, MBConvBlock
    from .fused_conv import mbse_enabled

    if not isinstance(net, EfficientEx):
        raise PlanUnsupported("backbone {} has no planner".format(type(net).__name__))
    if not mbse_enabled():
        raise PlanUnsupported("SSDK_MBSE=0: the EfficientNet backbone runs on PyTorch-ROCm")
    dt = plan.dtype
    (sconv, sbn, sact), = groups_of(net.conv1)
    cur = plan.conv(val, _pack(sconv, sbn, sact, dt, kinds=("stem",)))  # (the image is not an arena buffer)
    outputs = []
    for j in range(len(net.settings)):
        level = j + 1
        if level > max(net.outputs):
            break
        for blk in getattr(net, "stage{}".format(level)):
            if not isinstance(blk, MBConvBlock) or not MbSePack.supported(blk):
                raise PlanUnsupported("block not covered by ssdk_mbse: {}".format(type(blk).__name__))
            keep_cur = any(cur is o for o in outputs)
            expand = blk.parts()[0]
            mid = cur
            if expand is not None:
                (ec, eb, ea), = groups_of(expand)
                mid = plan.conv(cur, _pack(ec, eb, ea, dt))
            out = plan.mbse(mid, MbSePack(blk, dt), residual=cur if blk.use_residual else None)
            if mid is not cur:
                plan.release(mid)
            if not keep_cur:
                plan.release(cur)
            cur = out
        if level in net.outputs:
            outputs.append(cur)
    return outputs


def _darknet_group(module, kinds, what):
    """(conv, bn, act) of one Conv-BN-ReLU6 group of the DarkNet backbone; PlanUnsupported, with the reason, for anything else."""
    groups = sequential_groups(nn.Sequential(*flatten(module)))
    if groups is None or len(groups) != 1:
        raise PlanUnsupported("DarkNet {}: one Conv + BatchNorm + ReLU6 group expected, found {}".format(
            what, [type(m).__name__ for m in flatten(module)]))
    conv, bn, act = groups[0]
    if bn is None or act != "relu6":
        raise PlanUnsupported("DarkNet {}: Conv + BatchNorm + ReLU6 expected, found {} / {} / {}".format(
            what, type(conv).__name__, type(bn).__name__, act))
    if conv_kind(conv) not in kinds:
        raise PlanUnsupported("DarkNet {}: conv not covered by the HIP kernels ({} expected): {}".format(what, " | ".join(kinds), conv))
    return conv, bn, act


def record_darknet(plan, val, net):
    """DarkNet53 (nets/darknet.py): the stride-1 3 -> 32 image convolution on the image-stem kernel (its bias folded with the
    BatchNorm by fold_bn), each stage's stride-2 3x3 as a dense conv, and each Residual as ONE dkres op (csrc/ssdk_dkres.hip)
    where ``dkres_supported`` takes it -- otherwise two convs, the second adding x behind its activation (res_mode 0)."""
    from ssds.modeling.nets.darknet import DarkNet, Residual

    if not isinstance(net, DarkNet):
        raise PlanUnsupported("backbone {} has no planner".format(type(net).__name__))
    dt = plan.dtype
    sconv, sbn, sact = _darknet_group(net.conv1, ("stem",), "conv1")
    if sconv.stride != (1, 1):
        raise PlanUnsupported("DarkNet conv1: stride 1 expected, found {}".format(sconv.stride))
    cur = plan.conv(val, ConvPack(sconv, sbn, sact, dt))  # (the image is not an arena buffer)
    outputs = []
    for level in range(1, 6):
        if level > max(net.outputs):
            break
        for j, blk in enumerate(getattr(net, "block{}".format(level))):
            keep_cur = any(cur is o for o in outputs)
            what = "block{}.{}".format(level, j)
            if j == 0:
                conv, bn, act = _darknet_group(blk, ("dense",), what)
                if conv.kernel_size != (3, 3) or conv.stride != (2, 2):
                    raise PlanUnsupported("DarkNet {}: a 3x3 / stride 2 convolution expected: {}".format(what, conv))
                out = plan.conv(cur, ConvPack(conv, bn, act, dt))
            elif isinstance(blk, Residual):
                c1, b1, a1 = _darknet_group(blk.conv1x1, ("dense",), what + ".conv1x1")
                c2, b2, a2 = _darknet_group(blk.conv3x3, ("dense",), what + ".conv3x3")
                if (c1.kernel_size != (1, 1) or c2.kernel_size != (3, 3) or c1.stride != (1, 1) or c2.stride != (1, 1)
                        or c2.out_channels != c1.in_channels):
                    raise PlanUnsupported("DarkNet {}: 1x1 then 3x3, both stride 1, C -> C/2 -> C expected".format(what))
                p1, p2 = ConvPack(c1, b1, a1, dt), ConvPack(c2, b2, a2, dt)
                if dkres_supported(p1, p2, cur[3], cur[4], plan.dtype_code):
                    out = plan.dkres(cur, p1, p2)
                else:
                    mid = plan.conv(cur, p1)
                    out = plan.conv(mid, p2, residual=cur, res_mode=0)
                    plan.release(mid)
            else:
                raise PlanUnsupported("DarkNet {}: block {} has no planner".format(what, type(blk).__name__))
            if not keep_cur:
                plan.release(cur)
            cur = out
        if level in net.outputs:
            outputs.append(cur)
    return outputs


def record_densenet(plan, val, net):
    """DenseNet (nets/densenet.py): the stem on the 7x7 stem kernel + max-pool, then per dense block ONE buffer [n][h][w][Ctot] --
    ``place`` copies the block's input into its first channels and each dense layer is one ``dense`` op (csrc/ssdk_denselayer.hip)
    that reads channels [0, Cin) and writes [Cin, Cin + 32): no concatenation is recorded.  A transition pools FIRST
    (``densepool``: BN + ReLU + 2x2 average) and runs its bias-free 1x1 behind that, on a quarter of the pixels -- the same
    function in real arithmetic, since the convolution is linear.  A finished block's buffer IS the backbone map."""
    from ssds.modeling.nets.densenet import DenseNet, _DenseBlock, _DenseLayer, _Transition

    if not isinstance(net, DenseNet):
        raise PlanUnsupported("backbone {} has no planner".format(type(net).__name__))
    if not denselayer_enabled():
        raise PlanUnsupported("SSDK_DENSELAYER=0: the DenseNet backbone runs on PyTorch-ROCm")
    dt = plan.dtype
    stem = dict(net.conv1.named_children())
    if (list(stem) != ["conv", "norm", "relu", "pool"] or not isinstance(stem["conv"], nn.Conv2d)
            or not isinstance(stem["norm"], nn.BatchNorm2d) or not StemPack.supported(stem["conv"], stem["norm"])
            or stem["conv"].bias is not None or not isinstance(stem["relu"], nn.ReLU) or not isinstance(stem["pool"], nn.MaxPool2d)
            or _pair(stem["pool"].kernel_size) != (3, 3) or _pair(stem["pool"].stride) != (2, 2) or _pair(stem["pool"].padding) != (1, 1)
            or stem["pool"].ceil_mode):
        raise PlanUnsupported("DenseNet conv1: 7x7 / stride 2 conv + BatchNorm + ReLU + 3x3 / stride 2 max-pool expected")
    cur = plan.stem7(val, StemPack(stem["conv"], stem["norm"], "relu", dt))
    pooled = plan.pool(cur)
    plan.release(cur)
    cur = pooled
    outputs = []
    for level in range(1, len(net.block_config) + 1):
        if level > max(net.outputs):
            break
        if level > 1:
            what = "transition{}".format(level - 1)
            tr = getattr(net, what)
            parts = dict(tr.named_children())
            if not isinstance(tr, _Transition) or list(parts) != ["norm", "relu", "conv", "pool"]:
                raise PlanUnsupported("DenseNet {}: block {} has no planner".format(what, type(tr).__name__))
            conv, pool = parts["conv"], parts["pool"]
            if (not isinstance(parts["norm"], nn.BatchNorm2d) or not isinstance(parts["relu"], nn.ReLU) or not isinstance(conv, nn.Conv2d)
                    or conv.kernel_size != (1, 1) or conv.stride != (1, 1) or conv.groups != 1 or conv.bias is not None
                    or not isinstance(pool, nn.AvgPool2d) or _pair(pool.kernel_size) != (2, 2) or _pair(pool.stride) != (2, 2)
                    or _pair(pool.padding) != (0, 0) or pool.ceil_mode or parts["norm"].num_features != cur[2] or cur[2] % 8):
                raise PlanUnsupported("DenseNet {}: BatchNorm + ReLU + bias-free 1x1 + AvgPool2d(2, 2) expected".format(what))
            if cur[3] < 2 or cur[4] < 2:
                raise PlanUnsupported("DenseNet {}: a {} x {} map has no 2x2 window".format(what, cur[3], cur[4]))
            a, b = fold_norm(parts["norm"])
            pooled = plan.dense_pool(cur, a, b)
            if not any(cur is o for o in outputs):
                plan.release(cur)
            cur = plan.conv(pooled, ConvPack(conv, None, "none", dt))  # (linear and bias-free: it commutes with the average)
            plan.release(pooled)
        what = "denseblock{}".format(level)
        block = getattr(net, what)
        if not isinstance(block, _DenseBlock):
            raise PlanUnsupported("DenseNet {}: block {} has no planner".format(what, type(block).__name__))
        _, n, c0, h, w = cur
        layers = list(block.items())
        ctot = c0 + N.DENSE_COUT * len(layers)
        packs = []
        for j, (lname, layer) in enumerate(layers):
            lwhat = "{}.{}".format(what, lname)
            if not isinstance(layer, _DenseLayer):
                raise PlanUnsupported("DenseNet {}: block {} has no planner".format(lwhat, type(layer).__name__))
            why = DenseLayerPack.unsupported(layer)
            if why is not None:
                raise PlanUnsupported("DenseNet {}: {}".format(lwhat, why))
            if layer.drop_rate > 0 and layer.training:
                raise PlanUnsupported("DenseNet {}: drop_rate {} in training mode".format(lwhat, layer.drop_rate))
            cin = c0 + N.DENSE_COUT * j
            if layer.conv1.in_channels != cin:
                raise PlanUnsupported("DenseNet {}: {} input channels where the block has {}".format(lwhat, layer.conv1.in_channels, cin))
            if not N.lib.ssdk_dense_layer_supported(cin, h, w, ctot, plan.dtype_code):
                raise PlanUnsupported("DenseNet {}: ssdk_dense_layer_supported refuses Cin={} on {}x{} with pixel stride {}".format(
                    lwhat, cin, h, w, ctot))
            packs.append(DenseLayerPack(layer, dt))
        buf = plan.dense_block(n, ctot, h, w)
        c = plan.dense_place(cur, buf, ctot)
        plan.release(cur)
        for pk in packs:
            c = plan.dense(buf, n, c, h, w, ctot, pk)
        assert c == ctot, (c, ctot)
        cur = (buf, n, ctot, h, w)
        if level in net.outputs:
            outputs.append(cur)
    return outputs


def record_shufflenet(plan, val, net):
    """``_record_shufflenet`` inside the plan builder's ``padded_maps_scope`` (the neck behind it reads the padded maps), or inside
    one of its own when the backbone is recorded alone."""
    if in_padded_maps_scope():
        return _record_shufflenet(plan, val, net)
    with padded_maps_scope():
        return _record_shufflenet(plan, val, net)


def _record_shufflenet(plan, val, net):
    """ShuffleNetV2 (nets/shufflenet.py): conv1 on the stem kernel (its 24 output channels as 32 channels per pixel, zeros in the
    padding), the 3x3 / 2 max-pool, then ONE op per unit (csrc/ssdk_shuffle.hip): ``shuffledown`` for the first unit of a stage,
    ``shuffle`` for the others.  No chunk, concatenation or channel shuffle is recorded: the interleave is the store of the unit's
    kernel.  A stage's map has pad8(C) channels per pixel, zeros in [C, pad8(C)) (``fused_conv.PaddedValue`` when C % 8 != 0: 116 ->
    120, 244 -> 248); the packs of the convolutions that read it zero-pad their input channels (``ConvPack.in_segs``)."""
    from ssds.modeling.nets.shufflenet import InvertedResidual, ShuffleNetV2

    if not isinstance(net, ShuffleNetV2):
        raise PlanUnsupported("backbone {} has no planner".format(type(net).__name__))
    if not shuffleunit_enabled():
        raise PlanUnsupported("SSDK_SHUFFLEUNIT=0: the ShuffleNetV2 backbone runs on PyTorch-ROCm")
    allow_padded_maps()
    dt = plan.dtype
    pool = net.maxpool
    if (not isinstance(pool, nn.MaxPool2d) or _pair(pool.kernel_size) != (3, 3) or _pair(pool.stride) != (2, 2)
            or _pair(pool.padding) != (1, 1) or _pair(pool.dilation) != (1, 1) or pool.ceil_mode):
        raise PlanUnsupported("ShuffleNetV2 maxpool: a 3x3 / stride 2 / pad 1 max-pool expected, got {}".format(pool))
    try:
        groups = groups_of(net.conv1)
    except PlanUnsupported as e:
        raise PlanUnsupported("ShuffleNetV2 conv1: {}".format(e))
    if len(groups) != 1 or conv_kind(groups[0][0]) != "stem" or groups[0][0].stride != (2, 2) or groups[0][2] != "relu":
        raise PlanUnsupported("ShuffleNetV2 conv1: a 3x3 / stride 2 conv on the image + BatchNorm + ReLU expected")
    c_real = groups[0][0].out_channels
    cur = record_chain(plan, val, net.conv1, keep_input=True)  # the image is not an arena buffer
    pooled = plan.pool(cur)
    plan.release(cur)
    cur = plan._padded(pooled, c_real)
    outputs = []
    for level in (2, 3, 4):
        if level > max(net.outputs):
            break
        what = "stage{}".format(level)
        stage = getattr(net, what, None)
        if not isinstance(stage, nn.Sequential) or len(stage) == 0:
            raise PlanUnsupported("ShuffleNetV2 {}: a Sequential of units expected, got {}".format(what, type(stage).__name__))
        for j, unit in enumerate(stage):
            uwhat = "{}.{}".format(what, j)
            if not isinstance(unit, InvertedResidual):
                raise PlanUnsupported("ShuffleNetV2 {}: block {} has no planner".format(uwhat, type(unit).__name__))
            cls = ShuffleDownPack if unit.stride == 2 else ShuffleUnitPack
            why = cls.unsupported(unit)
            if why is not None:
                raise PlanUnsupported("ShuffleNetV2 {}: {}".format(uwhat, why))
            _, n, c, h, w = cur
            real = value_segs(cur)[0][0]
            cin = unit.branch2[0].in_channels if unit.stride == 2 else 2 * unit.branch2[0].in_channels
            if cin != real:
                raise PlanUnsupported("ShuffleNetV2 {}: a unit of {} input channels behind a map of {}".format(uwhat, cin, real))
            cb = unit.branch2[5].out_channels
            ok = (N.lib.ssdk_shuffle_down_supported(cin, cb, h, w, plan.dtype_code) if unit.stride == 2
                  else N.lib.ssdk_shuffle_unit_supported(cb, h, w, plan.dtype_code))
            if not ok:
                raise PlanUnsupported("ShuffleNetV2 {}: the kernel's predicate refuses Cin={} Cb={} on {}x{}".format(uwhat, cin, cb, h, w))
            pk = cls(unit, dt)
            nxt = plan.shuffle_down(cur, pk) if unit.stride == 2 else plan.shuffle_unit(cur, pk)
            if not any(cur is o for o in outputs):
                plan.release(cur)
            cur = nxt
        if level in net.outputs:
            outputs.append(cur)
    return outputs


def _pair(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


def record_backbone(plan, val, net):
    """Backbone maps of a planned backbone (MobileNet, ResNet, RegNetX, EfficientNet, DarkNet, DenseNet, ShuffleNetV2) from the image
    value; PlanUnsupported otherwise."""
    from ssds.modeling.nets.shufflenet import ShuffleNetV2
    from ssds.modeling.nets.darknet import DarkNet
    from ssds.modeling.nets.densenet import DenseNet
    from ssds.modeling.nets.efficientnet import EfficientEx
    from ssds.modeling.nets.mobilenet import MobileNetEx
    from ssds.modeling.nets.regnet import RegNet
    from ssds.modeling.nets.resnet import ResNet

    if isinstance(net, MobileNetEx):
        return record_mobilenet(plan, val, net)
    if isinstance(net, EfficientEx):
        return record_efficientnet(plan, val, net)
    if isinstance(net, ResNet):
        return record_resnet(plan, val, net)
    if isinstance(net, RegNet):
        return record_regnet(plan, val, net)
    if isinstance(net, DarkNet):
        return record_darknet(plan, val, net)
    if isinstance(net, DenseNet):
        return record_densenet(plan, val, net)
    if isinstance(net, ShuffleNetV2):
        return record_shufflenet(plan, val, net)
    raise PlanUnsupported("backbone {} has no planner".format(type(net).__name__))


# --------------------------------------------------------------------------------------------------------------
# FPN / BiFPN necks + shared towers on external backbone features
# --------------------------------------------------------------------------------------------------------------
def _tower_packs(tower, dtype):
    """SharedHead (4 x ConvBNReLU + final conv) -> ([ConvPack] of the ConvBNReLU layers, final ConvPack).  The
    towers are shared by every pyramid level, so they are packed once."""
    mods = list(tower.children())
    body = []
    for m in mods[:-1]:
        (conv, bn, act), = groups_of(m)
        body.append(ConvPack(conv, bn, act, dtype))
    last = mods[-1]
    if conv_kind(last) != "dense":
        raise PlanUnsupported("tower output conv not covered")
    return body, ConvPack(last, None, "none", dtype)


def _record_towers(plan, xx, loc_packs, conf_packs, lane=None, level=None):
    for (body, final), act, tag in ((loc_packs, "none", "loc"), (conf_packs, "sigmoid", "conf")):
        cur = xx
        for pk in body:
            nxt = plan.conv(cur, pk, role="tower", lane=lane or 0)
            if cur is not xx:
                plan.release(cur)
            cur = nxt
        plan.head(cur, final, act=act, tag=tag, lane=lane, level=level)
        if cur is not xx:
            plan.release(cur)


# pixels (batch x H x W) up to which a pyramid level goes to the side stream.  The 20x20, 10x10 and 5x5 levels of
# FPN-ResNet50@640 at batch 32 are 30 launches of a few dozen workgroups each, 0.85 ms one after the other, next to 3.3 ms of
# chip-filling launches on the two big levels (16384: +4 %); with the 40x40 level (51 200 pixels) on the side stream as well
# only the largest level stays in line and the two streams' launches fill each other's tails: another +1.9 % there, +2.3 % on
# BiFPN-RegNetX008@896 (measured, same box; SSDK_SMALL_LEVEL_PIXELS overrides).
SMALL_LEVEL_PIXELS = 65536


def _record_extras_and_towers(plan, model, pyramid, raw_last):
    """reference fpn.py:89-97 / bifpn.py:131-138: extras[i] on pyramid level i, extras[n] on the RAW last
    backbone map, later extras on the previous extra; both towers on every result.

    Order of the recording (round 4): all extras first, then the towers + heads of the SMALL levels as one contiguous
    block for the executor's side stream (one fork behind the extras, one join at the end of the plan), then the big
    levels on the main stream -- the small levels' launch chain runs next to the big levels instead of behind them.
    ``SSDK_LEVEL_LANES=0`` keeps everything in level order on one stream."""
    import os

    n = len(pyramid)
    loc_packs, conf_packs = _tower_packs(model.loc, plan.dtype), _tower_packs(model.conf, plan.dtype)
    levels = []
    xx = None
    for i, v in enumerate(model.extras):
        src = pyramid[i] if i < n else (raw_last if i == n else xx)
        xx = record_chain(plan, src, v, keep_input=True)
        levels.append(xx)
    limit = SMALL_LEVEL_PIXELS  # (a module attribute: tests monkeypatch it)
    small = [xx[1] * xx[3] * xx[4] <= limit for xx in levels]
    lanes = os.environ.get("SSDK_LEVEL_LANES", "1") != "0" and any(small) and not all(small)
    if lanes and sum(10 for sm in small if sm) > 320:
        lanes = False
    if not lanes:
        for i, xx in enumerate(levels):
            _record_towers(plan, xx, loc_packs, conf_packs, level=i)
        return
    for i, xx in enumerate(levels):
        if small[i]:
            _record_towers(plan, xx, loc_packs, conf_packs, lane=2, level=i)
    for i, xx in enumerate(levels):
        if not small[i]:
            _record_towers(plan, xx, loc_packs, conf_packs, lane=0, level=i)


def _neck_inputs(model, features, image):
    """(plan, backbone map values): from the image through a planned backbone, or the maps as external inputs."""
    if image is not None:
        plan = ConvPlan(image.device, image.dtype, image.shape)
        return plan, record_backbone(plan, plan.input_value(), model.backbone)
    f0 = features[0]
    for f in features:
        if f.shape[1] % 8:  # (a zero-padded map exists only inside a plan that also recorded its backbone)
            raise PlanUnsupported("a backbone map of {} channels (no multiple of 8) as an external input".format(f.shape[1]))
    plan = ConvPlan(f0.device, f0.dtype)
    return plan, [plan.add_input(f.shape) for f in features]


@_one_recording
def build_fpn_plan(model, features=None, image=None):
    """SSDFPN (ssds/fpn.py) neck + towers -> finalized ConvPlan, on the backbone maps ``features`` (external
    inputs) or, with ``image``, including a planned backbone.  The 1x1 lateral of level i and the nearest-x2
    upsample-add of level i+1 (reference fpn.py:80-87) are ONE launch: the coarser map rides in as a
    half-resolution residual of the lateral GEMM's epilogue."""
    plan, vals = _neck_inputs(model, features, image)
    n = len(vals)
    pyramid = [None] * n
    for i in range(n - 1, -1, -1):
        conv = model.transforms[i]
        if conv_kind(conv) != "dense":
            raise PlanUnsupported("lateral conv not covered: {}".format(conv))
        pack = ConvPack(conv, None, "none", plan.dtype)
        if i == n - 1:
            pyramid[i] = plan.conv(vals[i], pack)
        else:
            if pyramid[i + 1][3] * 2 != vals[i][3] or pyramid[i + 1][4] * 2 != vals[i][4]:
                raise PlanUnsupported("pyramid levels are not exact halves")
            pyramid[i] = plan.conv(vals[i], pack, residual=pyramid[i + 1], res_mode=1)
    _record_extras_and_towers(plan, model, pyramid, vals[n - 1])
    return plan.finalize()


def _fusion_weights(w, dtype):
    """relu(w) / (sum relu(w) + 1e-6), rounded to the model dtype like the module path does (bifpn.py:35-38)."""
    import torch

    w = torch.relu(w.detach().float())
    w = w / (w.sum(0) + 1e-6)
    return w.to(dtype).float().cpu()


def _record_bifpn_layer(plan, m, xx):
    from ssds import _native as N

    n = m.levels
    assert len(xx) == n
    w1, w2 = _fusion_weights(m.w1, plan.dtype), _fusion_weights(m.w2, plan.dtype)
    xx = list(xx)
    skips = [None] + xx[1:-1] + [None]
    for i in range(n - 1, 0, -1):  # top-down (reference bifpn.py:41-46)
        if xx[i][3] * 2 != xx[i - 1][3] or xx[i][4] * 2 != xx[i - 1][4]:
            raise PlanUnsupported("BiFPN levels are not exact halves")
        fused = plan.fuse(xx[i - 1], xx[i], weights=(w1[0, i - 1], w1[1, i - 1], 0.0), mode_b=N.FUSE_UP2)
        xx[i - 1] = record_chain(plan, fused, getattr(m, "top-down-{}".format(i - 1)))
    for i in range(0, n - 2):  # bottom-up with skip (reference bifpn.py:49-55)
        fused = plan.fuse(xx[i + 1], xx[i], skips[i + 1], weights=(w2[0, i], w2[1, i], w2[2, i]),
                          mode_b=N.FUSE_POOL2, mode_c=N.FUSE_SAME)
        xx[i + 1] = record_chain(plan, fused, getattr(m, "bottom-up-{}".format(i + 1)))
    fused = plan.fuse(xx[n - 1], xx[n - 2], weights=(w1[0, n - 1], w1[1, n - 1], 0.0), mode_b=N.FUSE_POOL2)
    xx[n - 1] = record_chain(plan, fused, getattr(m, "bottom-up-{}".format(n - 1)))  # reference bifpn.py:57-62
    return xx


@_one_recording
def build_bifpn_plan(model, features=None, image=None):
    """SSDBiFPN (ssds/bifpn.py): 1x1 transforms, stacked BiFPN layers (weighted fusions as one launch each),
    extras and shared towers -> finalized ConvPlan (inputs as in ``build_fpn_plan``)."""
    plan, vals = _neck_inputs(model, features, image)
    n = len(vals)
    xx = []
    for i in range(n):
        conv = model.transforms[i]
        if conv_kind(conv) != "dense":
            raise PlanUnsupported("transform conv not covered: {}".format(conv))
        xx.append(plan.conv(vals[i], ConvPack(conv, None, "none", plan.dtype)))
    for m in model.stack_bifpn:
        xx = _record_bifpn_layer(plan, m, xx)
    _record_extras_and_towers(plan, model, xx, vals[n - 1])
    return plan.finalize()


# --------------------------------------------------------------------------------------------------------------
# Shelf neck + per-level heads (ssds/shelf.py)
# --------------------------------------------------------------------------------------------------------------
def _record_shared_block(plan, blk, x):
    """SharedBlock (reference shelf.py:10-35): ONE 3x3 weight, two launches -- BatchNorm 1 + ReLU, then BatchNorm 2 + x and the
    ReLU behind the add (res_mode bit 1, as the ResNet blocks).  The Dropout2d between them is the identity in eval."""
    from ssds.modeling.ssds.shelf import SharedBlock

    if not isinstance(blk, SharedBlock) or blk.conv1.out_channels % 8:
        raise PlanUnsupported("block {} has no planner".format(type(blk).__name__))
    mid = plan.conv(x, _pack(blk.conv1, blk.bn1, "relu", plan.dtype))
    out = plan.conv(mid, _pack(blk.conv1, blk.bn2, "relu", plan.dtype), residual=x, res_mode=2)
    plan.release(mid)
    return out


def _record_shelf_pyramid(plan, pyr, xx):
    """ShelfPyramid (reference shelf.py:38-62) on the values ``xx``: block0 on the first, then per level
    block_i(conv_i(previous) + xx[i]) with the add in conv_i's epilogue -- a transposed convolution (decoder: one ssdk_convt op)
    or a ConvBNReLU / stride 2 (encoder: ReLU before the add, res_mode 0).  Returns the levels reversed, like the module; the
    inputs are handed back to the arena."""
    out, x = [], xx[0]
    for i in range(len(xx)):
        if i > 0:
            m = getattr(pyr, "conv{}".format(i))
            if isinstance(m, nn.ConvTranspose2d):
                if not ConvTPack.supported(m):
                    raise PlanUnsupported("transposed conv not covered by ssdk_convt3x3s2: {}".format(m))
                x = plan.convt(x, ConvTPack(m, plan.dtype), skip=xx[i])
            else:
                (conv, bn, act), = groups_of(m)
                if conv.kernel_size != (3, 3) or conv.stride != (2, 2) or conv.out_channels % 8:
                    raise PlanUnsupported("encoder step not covered: {}".format(conv))
                x = plan.conv(x, _pack(conv, bn, act, plan.dtype), residual=xx[i])
        blk_in = x
        x = _record_shared_block(plan, getattr(pyr, "block{}".format(i)), blk_in)
        if i > 0:
            plan.release(blk_in)
        out.append(x)
    for v in xx:
        plan.release(v)
    return out[::-1]


@_one_recording
def build_shelf_plan(model, features=None, image=None):
    """SSDShelf (ssds/shelf.py): 1x1 transforms (bias), decoder0 / encoder0 / decoder1 in the reference's orders and
    reversals, the string transforms ("Conv:S") on the last decoder's smallest map, and per level the two ``Head``s
    (ConvBNReLU + bare 3x3, sigmoid fused on conf) -> finalized ConvPlan (inputs as in ``build_fpn_plan``).  Everything runs
    in line on the caller's stream."""
    plan, vals = _neck_inputs(model, features, image)
    n = len(vals)
    for i in range(n - 1):
        if vals[i][3] != 2 * vals[i + 1][3] - 1 or vals[i][4] != 2 * vals[i + 1][4] - 1:
            raise PlanUnsupported("Shelf pyramid levels are not 2h - 1 of the next: {} over {}".format(vals[i][3:], vals[i + 1][3:]))
    xx = []
    for i in range(n):
        conv = model.transforms[i]
        if not isinstance(conv, nn.Conv2d) or conv_kind(conv) != "dense" or conv.out_channels % 8:
            raise PlanUnsupported("transform conv not covered: {}".format(conv))
        xx.append(plan.conv(vals[i], ConvPack(conv, None, "none", plan.dtype)))
    xx = xx[::-1]
    for pyr in model.shelf_head:
        xx = _record_shelf_pyramid(plan, pyr, xx)
    for i in range(n, len(model.transforms)):
        xx.append(record_extra(plan, xx[-1], model.transforms[i], keep_input=True))
    if len(xx) != len(model.loc) or len(xx) != len(model.conf):
        raise PlanUnsupported("{} levels, {} / {} heads".format(len(xx), len(model.loc), len(model.conf)))
    for i, f in enumerate(xx):
        for heads, act, tag in ((model.loc, "none", "loc"), (model.conf, "sigmoid", "conf")):
            mods = list(heads[i].children())
            if len(mods) != 2 or not isinstance(mods[1], nn.Conv2d) or conv_kind(mods[1]) != "dense":
                raise PlanUnsupported("head not covered: {}".format(type(heads[i]).__name__))
            (conv, bn, a), = groups_of(mods[0])
            mid = plan.conv(f, ConvPack(conv, bn, a, plan.dtype), role="tower")
            plan.head(mid, ConvPack(mods[1], None, "none", plan.dtype), act=act, tag=tag, lane=0, level=i)
            plan.release(mid)
    return plan.finalize()


# --------------------------------------------------------------------------------------------------------------
# YOLOv3 / YOLOv4 necks + per-level heads (ssds/yolo.py)
# --------------------------------------------------------------------------------------------------------------
def _record_cat(plan, a, b, up2):
    """``a || b`` (``up2``: ``b`` is the coarser level, nearest x2 on the way) as one ssdk_cat2 op; PlanUnsupported with the
    reason for maps that are not exact halves and for channel counts the kernel does not take."""
    if up2 and (b[3] * 2 != a[3] or b[4] * 2 != a[4]):
        raise PlanUnsupported("YOLO levels are not exact halves: {} over {}".format(a[3:], b[3:]))
    if not up2 and tuple(a[3:]) != tuple(b[3:]):
        raise PlanUnsupported("concatenation of maps of different sizes: {} and {}".format(a[3:], b[3:]))
    why = cat_supported(a[2], b[2], a[3], a[4], up2)
    if why:
        raise PlanUnsupported("concatenation not covered by ssdk_cat2: " + why)
    return plan.cat(a, b, up2=up2)


def _record_heads(plan, model, levels):
    """Per level the two ``Head``s (ConvBNReLU + bare 3x3, sigmoid fused on conf), in line, as in ``build_shelf_plan``."""
    if len(levels) != len(model.loc) or len(levels) != len(model.conf):
        raise PlanUnsupported("{} levels, {} / {} heads".format(len(levels), len(model.loc), len(model.conf)))
    for i, f in enumerate(levels):
        for heads, act, tag in ((model.loc, "none", "loc"), (model.conf, "sigmoid", "conf")):
            mods = list(heads[i].children())
            if len(mods) != 2 or not isinstance(mods[1], nn.Conv2d) or conv_kind(mods[1]) != "dense":
                raise PlanUnsupported("head not covered: {}".format(type(heads[i]).__name__))
            (conv, bn, a), = groups_of(mods[0])
            mid = plan.conv(f, ConvPack(conv, bn, a, plan.dtype), role="tower")
            plan.head(mid, ConvPack(mods[1], None, "none", plan.dtype), act=act, tag=tag, lane=0, level=i)
            plan.release(mid)


@_one_recording
def build_yolov3_plan(model, features=None, image=None):
    """YOLOV3 (ssds/yolo.py): from the smallest backbone map up, ``extras[i]`` on the concatenation of backbone map i with the
    nearest-x2 upsample of ``transforms[i]`` of the level below (one ssdk_cat2 op: the upsampled tensor is never written); the
    first string extra on the RAW last backbone map, later ones on the previous extra; per level the two heads -> finalized
    ConvPlan (inputs as in ``build_fpn_plan``).  Everything runs in line on the caller's stream."""
    plan, vals = _neck_inputs(model, features, image)
    n = len(vals)
    if len(model.transforms) != n - 1 or len(model.extras) < n:
        raise PlanUnsupported("{} backbone maps, {} transforms, {} extras".format(n, len(model.transforms), len(model.extras)))
    levels = [None] * n
    xx = None
    for i in range(n - 1, -1, -1):
        if i == n - 1:
            xx = record_chain(plan, vals[i], model.extras[i], keep_input=True)  # (the raw map is read again by the first string extra)
        else:
            up = record_chain(plan, xx, model.transforms[i], keep_input=True)  # (xx is level i + 1: its heads come later)
            fused = _record_cat(plan, vals[i], up, True)
            plan.release(up)
            plan.release(vals[i])
            xx = record_chain(plan, fused, model.extras[i])
        levels[i] = xx
    for i in range(n, len(model.extras)):
        xx = record_chain(plan, vals[n - 1] if i == n else xx, model.extras[i], keep_input=True)
        levels.append(xx)
    plan.release(vals[n - 1])
    _record_heads(plan, model, levels)
    return plan.finalize()


def _record_pan(plan, m, xx):
    """PANModule (ssds/yolo.py) on the values ``xx``, largest map first: top-down ``cat(x[i-1], up2(conv3x3(x[i])))`` +
    ConvBNReLUx2, then bottom-up ``cat(x[i+1], conv3x3/s2(x[i]))`` + ConvBNReLUx2.  A level's old value goes back to the arena
    when its last reader -- the concatenation that replaces it, or the step that reads it for its neighbour -- is recorded."""
    from ssds.modeling.ssds.yolo import PANModule

    if not isinstance(m, PANModule) or m.levels != len(xx):
        raise PlanUnsupported("neck block {} has no planner".format(type(m).__name__))
    xx = list(xx)
    n = m.levels
    for i in range(n - 1, 0, -1):
        up = record_chain(plan, xx[i], getattr(m, "top-down-{}-to-{}".format(i, i - 1)), keep_input=True)  # (read again bottom-up)
        fused = _record_cat(plan, xx[i - 1], up, True)
        plan.release(up)
        plan.release(xx[i - 1])
        xx[i - 1] = record_chain(plan, fused, getattr(m, "top-down-{}".format(i - 1)))
    for i in range(0, n - 1):
        down = record_chain(plan, xx[i], getattr(m, "bottom-up-{}-to-{}".format(i, i + 1)), keep_input=True)  # (xx[i] is an output)
        fused = _record_cat(plan, xx[i + 1], down, False)
        plan.release(down)
        plan.release(xx[i + 1])
        xx[i + 1] = record_chain(plan, fused, getattr(m, "bottom-up-{}".format(i + 1)))
    return xx


def _record_spp_transform(plan, val, seq):
    """``Sequential(ConvBNReLU, SPPModule(3), ConvBNReLU)`` of YOLOv4's last transform: the SPP block is one ssdk_spp op."""
    from ssds.modeling.ssds.yolo import SPPModule

    mods = list(seq.children())
    if len(mods) != 3 or not isinstance(mods[1], SPPModule):
        raise PlanUnsupported("transform not covered: {}".format(type(seq).__name__))
    spp = mods[1]
    if spp.pool_type != "max_pool":
        raise PlanUnsupported("SPP with {} has no kernel (ssdk_spp is the max-pool block)".format(spp.pool_type))
    if spp.num_levels != 3:
        raise PlanUnsupported("SPP with {} levels has no kernel (ssdk_spp pools 5, 9 and 13)".format(spp.num_levels))
    mid = record_chain(plan, val, mods[0])
    if mid[2] % 8:
        raise PlanUnsupported("SPP on {} channels is not covered by ssdk_spp (multiples of 8)".format(mid[2]))
    pooled = plan.spp(mid)
    plan.release(mid)
    return record_chain(plan, pooled, mods[2])


@_one_recording
def build_yolov4_plan(model, features=None, image=None):
    """YOLOV4 (ssds/yolo.py): the 3x3 ``transforms`` (the last one through the SPP block), the stacked PAN modules, the string
    extras behind the last level and per level the two heads -> finalized ConvPlan (inputs as in ``build_fpn_plan``)."""
    from ssds.modeling.ssds.yolo import SPPModule

    plan, vals = _neck_inputs(model, features, image)
    n = len(vals)
    if len(model.transforms) != n:
        raise PlanUnsupported("{} backbone maps, {} transforms".format(n, len(model.transforms)))
    xx = []
    for i, t in enumerate(model.transforms):
        if any(isinstance(m, SPPModule) for m in t.modules()):
            xx.append(_record_spp_transform(plan, vals[i], t))
        else:
            xx.append(record_chain(plan, vals[i], t))
    for m in model.fpn:
        xx = _record_pan(plan, m, xx)
    for e in model.extras:
        xx.append(record_chain(plan, xx[-1], e, keep_input=True))
    _record_heads(plan, model, xx)
    return plan.finalize()
