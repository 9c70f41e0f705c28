"""DenseNet feature extractor (levels 1..4 = ``denseblock1`` .. ``denseblock4``) -- the interface of the reference's
``ssds/modeling/nets/densenet.py`` (Huang et al. 2017): ``conv1.{conv,norm,relu,pool}``, ``denseblock{i}.denselayer{j}.{norm1,relu1,
conv1,norm2,relu2,conv2}``, ``transition{i}.{norm,relu,conv,pool}``; no ``norm5`` and no classifier, so the reference's checkpoints
and yaml configs carry over.  torchvision is not a dependency: ``_DenseLayer`` / ``_DenseBlock`` / ``_Transition`` restate the
published blocks with torchvision 0.7's module names, which is what fixes the ``state_dict`` keys.

A dense layer is ``conv3x3(ReLU(BN(conv1x1(ReLU(BN(cat(features)))))))``, growth 32, middle map ``bn_size * growth`` = 128 channels.
In eval mode on a HIP device the backbone is part of the detector's recorded plan (layers/planner.py ``record_densenet``): a dense
block owns one buffer, and each layer is ONE launch of csrc/ssdk_denselayer.hip that reads channels [0, Cin) of it and writes its
32 new channels behind them.  Training runs through this module."""
from collections import OrderedDict

import torch
import torch.nn as nn
import torch.nn.functional as F

from .rutils import register


class _DenseLayer(nn.Module):
    def __init__(self, num_input_features, growth_rate, bn_size, drop_rate, memory_efficient=False):
        super(_DenseLayer, self).__init__()
        self.add_module("norm1", nn.BatchNorm2d(num_input_features))
        self.add_module("relu1", nn.ReLU(inplace=True))
        self.add_module("conv1", nn.Conv2d(num_input_features, bn_size * growth_rate, kernel_size=1, stride=1, bias=False))
        self.add_module("norm2", nn.BatchNorm2d(bn_size * growth_rate))
        self.add_module("relu2", nn.ReLU(inplace=True))
        self.add_module("conv2", nn.Conv2d(bn_size * growth_rate, growth_rate, kernel_size=3, stride=1, padding=1, bias=False))
        self.drop_rate = float(drop_rate)
        self.memory_efficient = memory_efficient  # accepted for the reference's signature; checkpointing is not used

    def forward(self, input):
        x = torch.cat(input, 1) if isinstance(input, (list, tuple)) else input
        y = self.conv2(self.relu2(self.norm2(self.conv1(self.relu1(self.norm1(x))))))
        if self.drop_rate > 0:
            y = F.dropout(y, p=self.drop_rate, training=self.training)
        return y


class _DenseBlock(nn.ModuleDict):
    def __init__(self, num_layers, num_input_features, bn_size, growth_rate, drop_rate, memory_efficient=False):
        super(_DenseBlock, self).__init__()
        for i in range(num_layers):
            self.add_module("denselayer%d" % (i + 1), _DenseLayer(num_input_features + i * growth_rate, growth_rate=growth_rate,
                                                                 bn_size=bn_size, drop_rate=drop_rate,
                                                                 memory_efficient=memory_efficient))

    def forward(self, init_features):
        features = [init_features]
        for _, layer in self.items():
            features.append(layer(features))
        return torch.cat(features, 1)


class _Transition(nn.Sequential):
    def __init__(self, num_input_features, num_output_features):
        super(_Transition, self).__init__()
        self.add_module("norm", nn.BatchNorm2d(num_input_features))
        self.add_module("relu", nn.ReLU(inplace=True))
        self.add_module("conv", nn.Conv2d(num_input_features, num_output_features, kernel_size=1, stride=1, bias=False))
        self.add_module("pool", nn.AvgPool2d(kernel_size=2, stride=2))


class DenseNet(nn.Module):
    def __init__(self, growth_rate=32, block_config=(6, 12, 24, 16), num_init_features=64, bn_size=4, drop_rate=0,
                 memory_efficient=False, outputs=[], url=None):
        super(DenseNet, self).__init__()
        self.url = url
        self.outputs = list(outputs)
        self.block_config = tuple(block_config)
        self.growth_rate, self.bn_size, self.drop_rate = growth_rate, bn_size, drop_rate
        self.conv1 = nn.Sequential(OrderedDict([
            ("conv", nn.Conv2d(3, num_init_features, kernel_size=7, stride=2, padding=3, bias=False)),
            ("norm", nn.BatchNorm2d(num_init_features)),
            ("relu", nn.ReLU(inplace=True)),
            ("pool", nn.MaxPool2d(kernel_size=3, stride=2, padding=1)),
        ]))
        num_features = num_init_features
        for i, num_layers in enumerate(self.block_config):
            self.add_module("denseblock%d" % (i + 1), _DenseBlock(num_layers=num_layers, num_input_features=num_features, bn_size=bn_size,
                                                                  growth_rate=growth_rate, drop_rate=drop_rate,
                                                                  memory_efficient=memory_efficient))
            num_features = num_features + num_layers * growth_rate
            if i != len(self.block_config) - 1:
                self.add_module("transition%d" % (i + 1), _Transition(num_features, num_features // 2))
                num_features = num_features // 2
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight)
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)

    def initialize(self):
        """Nothing to fetch: pretrained weights are loaded from a checkpoint file, as for the other backbones."""

    def forward(self, x):
        x = self.conv1(x)
        outputs = []
        for j in range(len(self.block_config)):
            level = j + 1
            if level > max(self.outputs):
                break
            if level > 1:
                x = getattr(self, "transition{}".format(level - 1))(x)
            x = getattr(self, "denseblock{}".format(level))(x)
            if level in self.outputs:
                outputs.append(x)
        return outputs


@register
def DenseNet121(outputs, **kwargs):
    return DenseNet(32, (6, 12, 24, 16), 64, outputs=outputs)
