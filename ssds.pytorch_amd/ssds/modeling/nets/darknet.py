"""DarkNet53 feature extractor (levels 1..5 = ``block1`` .. ``block5``) -- the interface of the reference's
``ssds/modeling/nets/darknet.py``: the backbone YOLOv3 / YOLOv4 were designed around (Redmon & Farhadi 2018, table 1), with the
reference's own choices kept so that its checkpoints and yaml configs carry over: every convolution has a bias in front of its
BatchNorm, the activation is ReLU6 (not LeakyReLU), the 3 -> 32 image convolution has stride 1, and a residual block adds its
input BEHIND the second activation with nothing after the add.

Module names follow the reference (``conv1``, ``block{i}.0`` = the stage's stride-2 convolution, ``block{i}.{j}.conv1x1`` /
``.conv3x3``).  In eval mode on a HIP device the backbone is part of the detector's recorded plan (layers/planner.py
``record_darknet``): each residual block is ONE launch of csrc/ssdk_dkres.hip where ``ssdk_dkres_supported`` accepts its width."""
import torch.nn as nn

from .rutils import register


def _conv_bn_relu6(cin, cout, k, stride=1):
    return nn.Sequential(nn.Conv2d(cin, cout, k, stride=stride, padding=k // 2, bias=True), nn.BatchNorm2d(cout),
                         nn.ReLU6(inplace=True))


class Residual(nn.Module):
    """x + ReLU6(BN(conv3x3(ReLU6(BN(conv1x1(x)))))), C -> C / 2 -> C."""

    def __init__(self, nchannels):
        super(Residual, self).__init__()
        self.conv1x1 = _conv_bn_relu6(nchannels, nchannels // 2, 1)
        self.conv3x3 = _conv_bn_relu6(nchannels // 2, nchannels, 3)

    def forward(self, x):
        return self.conv3x3(self.conv1x1(x)) + x


class DarkNet(nn.Module):
    WIDTHS = (64, 128, 256, 512, 1024)

    def __init__(self, layers=(1, 2, 8, 8, 4), outputs=(5,), groups=1, width_per_group=64, url=None):
        super(DarkNet, self).__init__()
        assert len(layers) == len(self.WIDTHS), layers
        self.outputs = list(outputs)
        self.url = url
        self.conv1 = _conv_bn_relu6(3, 32, 3)
        cin = 32
        for i, (cout, blocks) in enumerate(zip(self.WIDTHS, layers)):
            stage = [_conv_bn_relu6(cin, cout, 3, stride=2)] + [Residual(cout) for _ in range(blocks)]
            setattr(self, "block{}".format(i + 1), nn.Sequential(*stage))
            cin = cout

    def initialize(self):
        """Nothing to fetch: the reference publishes no DarkNet53 weights."""

    def forward(self, x):
        outs = []
        x = self.conv1(x)
        for level in range(1, max(self.outputs) + 1):
            x = getattr(self, "block{}".format(level))(x)
            if level in self.outputs:
                outs.append(x)
        return outs


@register
def DarkNet53(outputs, **kwargs):
    return DarkNet(layers=(1, 2, 8, 8, 4), outputs=outputs)
