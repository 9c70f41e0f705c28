"""Backbones, looked up by name from cfg.MODEL.NETS (reference model_builder.py:21).  Only the families
named by BASELINE.json's configs are part of the MI355X hot path:
MobileNet v1/v2, ResNet / ResNeXt, RegNetX; EfficientNet-B0 ... B5 (the backbone the BiFPN detector was designed
around) joined them later, and DarkNet53 (the backbone of the YOLO detectors) after that (section 4.5j);
DenseNet121 (one HIP launch per dense layer, in-place concatenation) followed (section 4.5k), and ShuffleNetV2 x1 / x2 (one HIP
launch per shuffle unit, no chunk / cat / shuffle) is the latest (section 4.5l)."""
from .resnet import *  # noqa: F401,F403
from .mobilenet import *  # noqa: F401,F403
from .regnet import *  # noqa: F401,F403
from .efficientnet import *  # noqa: F401,F403
from .darknet import *  # noqa: F401,F403
from .densenet import *  # noqa: F401,F403
from .shufflenet import *  # noqa: F401,F403
