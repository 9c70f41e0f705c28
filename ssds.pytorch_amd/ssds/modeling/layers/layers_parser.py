"""String -> layer parser for the extra layers named in cfg.MODEL.FEATURE_LAYER (reference
``ssds/modeling/layers/layers_parser.py:5-30``): all six strings of the reference, the RFB blocks under the reference's own
spelling "RBF" / "RBF:S"."""
from .basic_layers import ConvBNReLUx2, SepConvBNReLU
from .rfb_layers import BasicRFB


def parse_feature_layer(layer, in_channels, depth):
    """Return the list of modules for one FEATURE_LAYER entry."""
    if layer == "SepConv:S":
        return [SepConvBNReLU(in_channels, depth, stride=2, expand_ratio=1)]
    elif layer == "SepConv":
        return [SepConvBNReLU(in_channels, depth, stride=1, expand_ratio=1)]
    elif layer == "Conv:S":
        return [ConvBNReLUx2(in_channels, depth, stride=2)]
    elif layer == "Conv":
        return [ConvBNReLUx2(in_channels, depth, stride=1)]
    elif layer == "RBF:S":
        return [BasicRFB(in_channels, depth, stride=2, scale=1.0, visual=2)]
    elif layer == "RBF":
        return [BasicRFB(in_channels, depth, stride=1, scale=1.0, visual=2)]
    elif isinstance(layer, int):
        return []
    else:
        raise AssertionError("Undefined layer: {}".format(layer))
