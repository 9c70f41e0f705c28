"""Which kernel families the training step runs on: ONE ordered table, read by ``train_ddp.Solver`` (``route_for_training``), by
tools/bench_train.py (``bench_fields``) and frozen by tests/test_route_digest_cpu.py.

A ``Pass`` swaps layers of the freshly built (CPU, fp32) model to their kernel-backed classes in place: no new parameters, same
``state_dict``.  ``PASSES`` is in the order the passes run, and the order is part of the routing:

  * shuffle runs after the BatchNorm passes and before pw_gemm / bn_stats, so that the DepthwiseConv2d / FastBatchNorm2d pairs it
    creates get their statistics hand-off;
  * dense3 runs before conv3_extras, which then skips the extras dense3 took (no longer plain nn.Conv2d);
  * the detector families (FPN / BiFPN, YOLO, Shelf) are mutually exclusive, so one order convt, dense3, neck, cat serves all three.

To add a kernel family: write its ``use_native_*`` in the layer module with a ``DEFAULT`` (a kernel-backed ``nn.Conv2d`` goes on
``layers/kernel_conv.KernelConv2d``, which says what the class has to declare), add ONE entry here at the place its order
constraints allow, a row in docs/SWITCHES.md, and regenerate tests/golden/route_digest.json (the digest names what moved).
docs/SWITCHES.md has every switch with the measurement behind its default; DESIGN.md section 6 describes the table."""
import collections
import os

import torch.nn as nn

from .layers import (batchnorm, cattrain, convttrain, denseconv, densetrain, groupedconv, headconv, mbconvtrain, neckfuse, pointwise,
                     shuffletrain, stemconv)
from .nets.densenet import DenseNet
from .nets.shufflenet import ShuffleNetV2
from .ssds.bifpn import SSDBiFPN
from .ssds.fpn import SSDFPN
from .ssds.shelf import SSDShelf
from .ssds.yolo import YOLOV3, YOLOV4


def _not0(value):
    return value != "0"


def _is(*values):
    return lambda value: value in values


# name     key of the pass in ``route_for_training``'s result and in ``needs``
# switch   its SSDK_* variable, read when the model is routed; None: unconditional (the function reads its own switch, if any)
# default  what an unset variable means: a string, or a function of the model where the model decides
# on       which values turn the pass on
# where    the models it applies to: (attribute of the model | None for the model itself, classes); None: any model
# needs    the earlier passes (or "sync_bn" / "local_bn") that must have been applied
# apply    the function that swaps the layers
# blocked  the line rank 0 prints when the pass is switched on for this model and ``needs`` keeps it off
# bench    (key of tools/bench_train.py's JSON line, () -> whether the kernels ran), or None
Pass = collections.namedtuple("Pass", "name switch default on where needs apply blocked bench")


def _pass(name, switch, default, apply, on=_not0, where=None, needs=(), blocked=None, bench=None):
    return Pass(name, switch, default, on, where, needs, apply, blocked, bench)


_NECKS = (None, (SSDFPN, SSDBiFPN, YOLOV3, YOLOV4, SSDShelf))


def _set_wgrad_min_pixels(pixels):
    def apply(model):
        headconv.WGRAD_MIN_PIXELS = pixels  # a module global: the last routed model decides for the process

    return apply


PASSES = (
    # --sync-bn with SSDK_FAST_BN=0: torch's SyncBatchNorm (the detector itself is no BatchNorm, so the conversion is in place)
    _pass("torch_sync_bn", "SSDK_FAST_BN", "1", nn.SyncBatchNorm.convert_sync_batchnorm, on=_is("0"), needs=("sync_bn",)),
    # training BN on the ssdk kernels: local statistics, like the default ...
    _pass("fast_bn", "SSDK_FAST_BN", "1", batchnorm.use_fast_batchnorm, needs=("local_bn",)),
    # ... or statistics over all ranks, on the same kernels and fusions (one name: what needs fast BN takes either)
    _pass("fast_bn", "SSDK_FAST_BN", "1", batchnorm.use_fast_sync_batchnorm, needs=("sync_bn",)),
    # Conv-BN-ReLU6: the clamp and its gradient mask ride on the BN passes
    _pass("bn_act", "SSDK_FUSE_BN_ACT", "1", batchnorm.fuse_bn_activations, needs=("fast_bn",)),
    # expand BN (+ ReLU6) applied by the depthwise kernels on load: no apply pass (SSDK_BN_DEFER=0, read by the function: off)
    _pass("bn_defer", "SSDK_FUSE_BN_ACT", "1", batchnorm.fuse_bn_into_depthwise, needs=("fast_bn",)),
    # ShuffleNetV2 backbones: the units' slice 1x1 and join on csrc/ssdk_shuffletrain.hip, their depthwise 3x3 on the
    # project's depthwise kernels, 1x1 layers of any width.  0: chunk / cat / channel_shuffle and nn.Conv2d
    _pass("shuffle", "SSDK_SHUFFLE_TRAIN", shuffletrain.DEFAULT, shuffletrain.use_native_shuffle, where=("backbone", (ShuffleNetV2,)),
          bench=("shuffle_train", lambda: shuffletrain.STATS["join_forward"] > 0)),
    # DenseNet backbones: a dense block trains on one feature buffer and one gradient buffer, norm1 + relu1 applied by
    # the first 1x1 on load (csrc/ssdk_densetrain.hip); swapped at block level, the layers keep their classes.  0: _DenseBlock.forward,
    # i.e. torch.cat and a full BatchNorm per layer.  The block's statistics are local sums, so not under --sync-bn
    _pass("dense", "SSDK_DENSE_TRAIN", densetrain.DEFAULT, densetrain.use_native_dense_block, where=("backbone", (DenseNet,)),
          needs=("local_bn",),
          blocked="SSDK_DENSE_TRAIN: --sync-bn keeps the dense blocks on the module path (the block's statistics are local)",
          bench=("dense_train", lambda: densetrain.STATS["native_forward"] > 0)),
    # 1x1 convolutions on the NCHW tensors (16 bit: csrc/ssdk_pwtrain.hip; fp32: library GEMMs)
    _pass("pw_gemm", "SSDK_PW_GEMM", "1", pointwise.use_pointwise_gemm),
    # the 1x1 kernels hand their BatchNorm the (local) batch statistics (SSDK_BN_STATS_FUSED=0, read by the function: off)
    _pass("bn_stats", None, None, pointwise.fuse_conv_bn_statistics, needs=("pw_gemm", "fast_bn")),
    # grouped 3x3 of the RegNetX / ResNeXt bottlenecks: forward, input gradient, weight gradient on csrc/ssdk_gconvtrain.hip
    # (0: nn.Conv2d, i.e. MIOpen's grouped convolution behind autocast's weight cast).  The benchmark reports the switch, not a counter
    _pass("gconv", "SSDK_GCONV_TRAIN", "1", groupedconv.use_native_gconv,
          bench=("gconv_train", lambda: _not0(os.environ.get("SSDK_GCONV_TRAIN", "1")))),
    # the image-side 3x3 / stride-2 convolution: forward + weight gradient on csrc/ssdk_stemtrain.hip (A/B tools/run/r06_s42.sh:
    # 17.0 vs 17.5 ms per step)
    _pass("stem3", None, None, pointwise.use_native_stem),
    # the 7x7 / stride-2 stem of the ResNet / ResNeXt backbones (any detector on them): forward + weight gradient on
    # csrc/ssdk_stem7train.hip.  0: nn.Conv2d, i.e. the library convolution behind autocast's weight cast
    _pass("stem7", "SSDK_STEM7_TRAIN", stemconv.DEFAULT, stemconv.use_native_stem7,
          bench=("stem7_train", lambda: stemconv.STATS["native_forward"] > 0)),
    # the EfficientNet MBConv blocks: 5x5 depthwise forward / gradients and SiLU + squeeze-excite on csrc/ssdk_mbconvtrain.hip, swapped
    # at block level (the convolution modules keep their classes).  0: MBConvBlock.forward, i.e. the library's depthwise kernels and
    # the eager SiLU / pool / 1x1 / multiply passes.  Any model: others have no such block
    _pass("mbconv", "SSDK_MBCONV_TRAIN", mbconvtrain.DEFAULT, mbconvtrain.use_native_mbconv,
          bench=("mbconv_train", lambda: mbconvtrain.STATS["native_forward"] > 0)),
    # SSD heads: forward of each level's loc | conf pair on the inference kernels (SSDK_HEAD_PAIR=0, read by the function: MIOpen)
    _pass("head_pairs", None, None, headconv.use_head_pairs),
    # SSDShelf: the decoders' transposed 3x3 / stride 2 + bias + skip add, forward and gradients on
    # csrc/ssdk_convttrain.hip; the step measured slower with it, so an unset variable means 0 (convttrain.DEFAULT has the figures)
    _pass("convt", "SSDK_CONVT_TRAIN", convttrain.DEFAULT, convttrain.use_native_convt, where=(None, (SSDShelf,)),
          bench=("convt_train", lambda: convttrain.STATS["native_forward"] > 0)),
    # dense 3x3 on csrc/ssdk_conv3train.hip (forward, input gradient, weight gradient).  FPN / BiFPN: towers, smoothing,
    # heads, ResNet bottlenecks, extras.  YOLO (4.5h): transforms, ConvBNReLUx2, heads, PAN stride-2 layers, ResNet BasicBlocks --
    # measured slower than nn.Conv2d there, so unset means 0 (denseconv.YOLO_DEFAULT has the figures).  Shelf (4.5i): the SharedBlock
    # 3x3 (one weight on two maps), the encoder's stride-2 layers, the heads, the ResNet blocks -- never timed on Shelf, slower on the
    # other ResNet-18 models, so unset means 0 as on YOLO.  0: nn.Conv2d / the im2col extras.  SSD models are not touched
    _pass("dense3", "SSDK_DENSE3_TRAIN",
          lambda model: denseconv.DEFAULT if isinstance(model, (SSDFPN, SSDBiFPN)) else denseconv.YOLO_DEFAULT,
          denseconv.use_native_dense3x3, where=_NECKS, bench=("dense3_train", lambda: denseconv.STATS["swapped"] > 0)),
    # the BiFPN weighted fusions, the FPN top-down upsample-adds and the ResNet stem's max-pool (on YOLO and Shelf models the pool is
    # all there is): forward and backward on csrc/ssdk_necktrain.hip.  0: the eager expressions / nn.MaxPool2d.  SSD models are not touched
    _pass("neck", "SSDK_NECK_TRAIN", neckfuse.DEFAULT, neckfuse.use_native_neck, where=_NECKS,
          bench=("neck_train", lambda: neckfuse.STATS["fuse_forward"] + neckfuse.STATS["pool_forward"] > 0)),
    # YOLOv3 / YOLOv4: the concatenations and the SPP block on csrc/ssdk_cattrain.hip
    _pass("cat", "SSDK_CAT_TRAIN", cattrain.DEFAULT, cattrain.use_native_cat, where=(None, (YOLOV3, YOLOV4)),
          bench=("cat_train", lambda: cattrain.STATS["cat_forward"] + cattrain.STATS["spp_forward"] > 0)),
    # SSDK_CONV3_NATIVE=0: the library convolution for the extras, and the weight gradients of head levels under 64 pixels with it
    _pass("head_wgrad_library", "SSDK_CONV3_NATIVE", "2", _set_wgrad_min_pixels(64), on=_is("0")),
    _pass("head_wgrad_native", "SSDK_CONV3_NATIVE", "2", _set_wgrad_min_pixels(0), on=_is("1", "2")),
    # 2 (default): NO library convolution in the step: the extras' 3x3 / stride-2 layers as im2col + ssdk_pw_* + col2im with the batch
    # folded into the GEMM's pixel dimension (64 / 16 / 4 / 1 pixels per image: pointwise.FOLD_BELOW), and the weight gradients of the
    # small head levels on ssdk_pw_wgrad the same way.  tools/run/r06_s53.sh: 16.7 vs 17.0 ms per step against the library (0); before
    # the fold the same path was 0.6 ms SLOWER than the library
    _pass("conv3_extras", "SSDK_CONV3_NATIVE", "2", lambda model: pointwise.use_native_conv3x3(model.extras), on=_is("2"),
          where=("extras", (nn.Module,))),
    # 1: EVERY 3x3 layer (the heads too) as im2col + the 1x1 kernels.  Correct (tests/test_gpu_train.py) and slow: 23.2 vs 20.8 ms per
    # step when it was measured (round 6, session 4: the streaming 1x1 kernels are the wrong shape for K = 864 ... 4608 at 480 output
    # channels; the heads run on the inference kernels instead: headconv.py)
    _pass("conv3_all", "SSDK_CONV3_NATIVE", "2", pointwise.use_native_conv3x3, on=_is("1")),
)


def _switched_on(p, model):
    if p.where is not None:
        attr, classes = p.where
        if not isinstance(getattr(model, attr, None) if attr else model, classes):
            return False
    if p.switch is None:
        return True
    return p.on(os.environ.get(p.switch, p.default(model) if callable(p.default) else p.default))


def route_for_training(model, sync_bn=False, local_rank=0):
    """Run ``PASSES`` over ``model`` in order (in place).  -> OrderedDict{pass name: applied}."""
    have = {"sync_bn": sync_bn, "local_bn": not sync_bn}
    applied = collections.OrderedDict()
    for p in PASSES:
        ok = _switched_on(p, model)
        if ok and not all(have[n] for n in p.needs):
            ok = False
            if p.blocked and local_rank == 0:
                print(p.blocked)
        if ok:
            p.apply(model)
        have[p.name] = applied[p.name] = ok or applied.get(p.name, False)
    return applied


def bench_fields():
    """[(JSON key, whether those kernels ran in this process)] for tools/bench_train.py, in table order."""
    return [(p.bench[0], p.bench[1]()) for p in PASSES if p.bench]
