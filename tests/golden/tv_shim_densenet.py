"""Stand-in for ``torchvision.models.densenet`` (0.7 API), so that the REFERENCE's ``ssds/modeling/nets/densenet.py`` can be imported
unmodified where torchvision is not installed: what tv_shim.py does for MobileNet and ResNet.  ``install()`` goes next to
``tv_shim.install()``.

Used ONLY by ``make_golden_densenet.py``.  The blocks restate the published DenseNet-BC layer (Huang et al. 2017) with torchvision
0.7's module names (``norm1, relu1, conv1, norm2, relu2, conv2``; ``denselayer%d``; ``norm, relu, conv, pool``), which is what fixes the
``state_dict`` keys of the reference model.  Nothing under ``ssds.pytorch_amd/`` imports them: backbone parity is "reference wiring
around restated standard blocks", as for ResNet."""
import sys
import types

import torch
import torch.nn as nn
import torch.nn.functional as F

model_urls = {k: None for k in ("densenet121", "densenet169", "densenet201", "densenet161")}


class _DenseLayer(nn.Module):
    def __init__(self, num_input_features, growth_rate, bn_size, drop_rate, memory_efficient=False):
        super().__init__()
        self.add_module("norm1", nn.BatchNorm2d(num_input_features))
        self.add_module("relu1", nn.ReLU(inplace=True))
        self.add_module("conv1", nn.Conv2d(num_input_features, bn_size * growth_rate, kernel_size=1, stride=1, bias=False))
        self.add_module("norm2", nn.BatchNorm2d(bn_size * growth_rate))
        self.add_module("relu2", nn.ReLU(inplace=True))
        self.add_module("conv2", nn.Conv2d(bn_size * growth_rate, growth_rate, kernel_size=3, stride=1, padding=1, bias=False))
        self.drop_rate = float(drop_rate)
        self.memory_efficient = memory_efficient

    def forward(self, input):
        prev = [input] if isinstance(input, torch.Tensor) else input
        bottleneck = self.conv1(self.relu1(self.norm1(torch.cat(prev, 1))))
        new = self.conv2(self.relu2(self.norm2(bottleneck)))
        if self.drop_rate > 0:
            new = F.dropout(new, p=self.drop_rate, training=self.training)
        return new


class _DenseBlock(nn.ModuleDict):
    def __init__(self, num_layers, num_input_features, bn_size, growth_rate, drop_rate, memory_efficient=False):
        super().__init__()
        for i in range(num_layers):
            self.add_module("denselayer%d" % (i + 1), _DenseLayer(num_input_features + i * growth_rate, growth_rate=growth_rate,
                                                                 bn_size=bn_size, drop_rate=drop_rate,
                                                                 memory_efficient=memory_efficient))

    def forward(self, init_features):
        features = [init_features]
        for name, layer in self.items():
            features.append(layer(features))
        return torch.cat(features, 1)


class _Transition(nn.Sequential):
    def __init__(self, num_input_features, num_output_features):
        super().__init__()
        self.add_module("norm", nn.BatchNorm2d(num_input_features))
        self.add_module("relu", nn.ReLU(inplace=True))
        self.add_module("conv", nn.Conv2d(num_input_features, num_output_features, kernel_size=1, stride=1, bias=False))
        self.add_module("pool", nn.AvgPool2d(kernel_size=2, stride=2))


def install():
    """Register this file's blocks as ``torchvision.models.densenet`` (call ``tv_shim.install()`` first)."""
    models = sys.modules["torchvision.models"]
    dn = types.ModuleType("torchvision.models.densenet")
    dn._DenseLayer, dn._DenseBlock, dn._Transition, dn.model_urls = _DenseLayer, _DenseBlock, _Transition, model_urls
    models.densenet = dn
    sys.modules["torchvision.models.densenet"] = dn
