"""ShuffleNetV2 feature extractor (levels 2..4 = ``stage2`` .. ``stage4``) -- the interface of the reference's
``ssds/modeling/nets/shufflenet.py`` (Ma et al. 2018): ``conv1.{0,1,2}``, ``maxpool``, ``stage{2,3,4}.{i}.branch1.{0..4}`` and
``.branch2.{0..7}``; the classifier tail (``conv5``, ``fc``) is not instantiated, as for MobileNet and ResNet, so the reference's
checkpoints and yaml configs carry over (``checkpoint.resume_checkpoint`` ignores the keys of the tail).  torchvision is not a
dependency: ``InvertedResidual`` restates the published unit with torchvision 0.7's module names, which is what fixes the
``state_dict`` keys.

A unit, with ``Cb = oup // 2``:
  stride 1   left = x[:, :Cb]        right = branch2(x[:, Cb:])
  stride 2   left = branch1(x)       right = branch2(x)
  y = channel_shuffle(cat(left, right), 2), i.e. y[2i] = left[i], y[2i + 1] = right[i]
``branch1`` = dw3x3/s + BN, 1x1 + BN + ReLU; ``branch2`` = 1x1 + BN + ReLU, dw3x3/s + BN, 1x1 + BN + ReLU.
In eval mode on a HIP device the backbone is part of the detector's recorded plan (layers/planner.py ``record_shufflenet``): every
unit is ONE launch of csrc/ssdk_shuffle.hip that writes the interleaved result directly -- no chunk, cat or shuffle exists as an
operation.  Training runs through this module: under ``layers/shuffletrain.use_native_shuffle`` a unit's 1x1 on the channel slice,
its depthwise 3x3 and the interleaving join run on the project's kernels, forward and backward (csrc/ssdk_shuffletrain.hip)."""
import torch
import torch.nn as nn

from .rutils import register


def channel_shuffle(x, groups):
    batchsize, num_channels, height, width = x.size()
    channels_per_group = num_channels // groups
    x = x.view(batchsize, groups, channels_per_group, height, width)
    x = torch.transpose(x, 1, 2).contiguous()
    return x.view(batchsize, -1, height, width)


class InvertedResidual(nn.Module):
    def __init__(self, inp, oup, stride):
        super(InvertedResidual, self).__init__()
        if not (1 <= stride <= 3):
            raise ValueError("illegal stride value")
        self.stride = stride
        branch_features = oup // 2
        assert (self.stride != 1) or (inp == branch_features << 1)
        if self.stride > 1:
            self.branch1 = nn.Sequential(
                self.depthwise_conv(inp, inp, kernel_size=3, stride=self.stride, padding=1),
                nn.BatchNorm2d(inp),
                nn.Conv2d(inp, branch_features, kernel_size=1, stride=1, padding=0, bias=False),
                nn.BatchNorm2d(branch_features),
                nn.ReLU(inplace=True),
            )
        else:
            self.branch1 = nn.Sequential()
        self.branch2 = nn.Sequential(
            nn.Conv2d(inp if (self.stride > 1) else branch_features, branch_features, kernel_size=1, stride=1, padding=0, bias=False),
            nn.BatchNorm2d(branch_features),
            nn.ReLU(inplace=True),
            self.depthwise_conv(branch_features, branch_features, kernel_size=3, stride=self.stride, padding=1),
            nn.BatchNorm2d(branch_features),
            nn.Conv2d(branch_features, branch_features, kernel_size=1, stride=1, padding=0, bias=False),
            nn.BatchNorm2d(branch_features),
            nn.ReLU(inplace=True),
        )

    @staticmethod
    def depthwise_conv(i, o, kernel_size, stride=1, padding=0, bias=False):
        return nn.Conv2d(i, o, kernel_size, stride, padding, bias=bias, groups=i)

    native_shuffle = False  # set per unit by layers/shuffletrain.use_native_shuffle

    def forward(self, x):
        if self.native_shuffle:
            from ssds.modeling.layers import shuffletrain

            out = shuffletrain.try_unit(self, x)  # (None: x is outside the kernels' contract)
            if out is not None:
                return out
        if self.stride == 1:
            x1, x2 = x.chunk(2, dim=1)
            out = torch.cat((x1, self.branch2(x2)), dim=1)
        else:
            out = torch.cat((self.branch1(x), self.branch2(x)), dim=1)
        return channel_shuffle(out, 2)


class ShuffleNetV2(nn.Module):
    def __init__(self, stages_repeats, stages_out_channels, outputs=[4], url=None):
        super(ShuffleNetV2, self).__init__()
        if len(stages_repeats) != 3:
            raise ValueError("expected stages_repeats as list of 3 positive ints")
        if len(stages_out_channels) != 5:
            raise ValueError("expected stages_out_channels as list of 5 positive ints")
        self.url = url
        self.outputs = list(outputs)
        self.stages_repeats = tuple(stages_repeats)
        self._stage_out_channels = tuple(stages_out_channels)
        input_channels, output_channels = 3, stages_out_channels[0]
        self.conv1 = nn.Sequential(
            nn.Conv2d(input_channels, output_channels, 3, 2, 1, bias=False),
            nn.BatchNorm2d(output_channels),
            nn.ReLU(inplace=True),
        )
        input_channels = output_channels
        self.maxpool = nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
        for name, repeats, output_channels in zip(("stage2", "stage3", "stage4"), stages_repeats, stages_out_channels[1:]):
            seq = [InvertedResidual(input_channels, output_channels, 2)]
            for _ in range(repeats - 1):
                seq.append(InvertedResidual(output_channels, output_channels, 1))
            setattr(self, name, nn.Sequential(*seq))
            input_channels = output_channels
        # (conv5 / fc: the classifier tail, never run by a detector, is not built)

    def initialize(self):
        """Nothing to fetch: pretrained weights are loaded from a checkpoint file, as for the other backbones."""

    def forward(self, x):
        x = self.maxpool(self.conv1(x))
        outputs = []
        for i, stage in enumerate([self.stage2, self.stage3, self.stage4]):
            level = i + 2
            if level > max(self.outputs):
                break
            x = stage(x)
            if level in self.outputs:
                outputs.append(x)
        return outputs


@register
def ShuffleNetV2_x1(outputs, **kwargs):
    return ShuffleNetV2([4, 8, 4], [24, 116, 232, 464, 1024], outputs=outputs)


@register
def ShuffleNetV2_x2(outputs, **kwargs):
    return ShuffleNetV2([4, 8, 4], [24, 244, 488, 976, 2048], outputs=outputs)
