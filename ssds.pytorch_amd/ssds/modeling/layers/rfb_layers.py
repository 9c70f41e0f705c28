"""The receptive-field block of the "RBF" / "RBF:S" extra layers (reference ``ssds/modeling/layers/rfb_layers.py``:
``BasicConv`` and ``BasicRFB``) -- constructor signatures, attribute names and ``state_dict`` keys (``branch0.0.conv.weight``, ...,
``ConvLinear``, ``shortcut``) are the reference's, so checkpoints are interchangeable.  ``BasicRFB_a`` and the two ``_lite`` blocks
are reached by no FEATURE_LAYER string and are not here.

The block, with i = in_planes // 8, s = stride, v = visual::

    branch0: 1x1 C->i  BN ReLU | 3x3 i->2i stride s BN ReLU                                   | 3x3 2i->2i dil v+1,  pad v+1,  BN
    branch1: 1x1 C->i  BN ReLU | 3x3 i->3(i//2) BN ReLU | 3x3 3(i//2)->2i stride s BN ReLU    | 3x3 2i->2i dil 2v+1, pad 2v+1, BN
    y = ReLU( scale * BN(1x1(cat(branch0, branch1))) + BN(1x1 stride s (x)) )

These modules are plain torch (training, CPU, anything the plan refuses).  In eval mode on a HIP device the detector's recorded
plan runs the block as ten ops (``planner.record_rfb``): the 1x1 / 3x3 convolutions on the fused kernels, the two dilated 3x3 on
``csrc/ssdk_dconv.hip``, the concatenation on ``ssdk_cat2``, and ``scale``, the shortcut add and the ReLU in ``ConvLinear``'s epilogue."""
import torch
import torch.nn as nn


class BasicConv(nn.Module):
    """conv (+ BN eps 1e-5 / momentum 0.01) (+ ReLU); ``self.bn`` / ``self.relu`` are None where switched off."""

    def __init__(self, in_planes, out_planes, kernel_size, stride=1, padding=0, dilation=1, groups=1, relu=True, bn=True, bias=False):
        super(BasicConv, self).__init__()
        self.out_channels = out_planes
        self.conv = nn.Conv2d(in_planes, out_planes, kernel_size=kernel_size, stride=stride, padding=padding, dilation=dilation,
                              groups=groups, bias=bias)
        self.bn = nn.BatchNorm2d(out_planes, eps=1e-5, momentum=0.01, affine=True) if bn else None
        self.relu = nn.ReLU(inplace=True) if relu else None

    def forward(self, x):
        x = self.conv(x)
        if self.bn is not None:
            x = self.bn(x)
        return x if self.relu is None else self.relu(x)


class BasicRFB(nn.Module):
    """Two branches that end in dilated 3x3 convolutions (dilation visual + 1 and 2 visual + 1), concatenated, projected by a 1x1 and
    added, times ``scale``, to a 1x1 shortcut of the input."""

    def __init__(self, in_planes, out_planes, stride=1, scale=0.1, visual=1):
        super(BasicRFB, self).__init__()
        self.scale = scale
        self.out_channels = out_planes
        i = in_planes // 8
        d0, d1 = visual + 1, 2 * visual + 1
        self.branch0 = nn.Sequential(
            BasicConv(in_planes, i, kernel_size=1, stride=1),
            BasicConv(i, 2 * i, kernel_size=(3, 3), stride=stride, padding=(1, 1)),
            BasicConv(2 * i, 2 * i, kernel_size=3, stride=1, padding=d0, dilation=d0, relu=False),
        )
        self.branch1 = nn.Sequential(
            BasicConv(in_planes, i, kernel_size=1, stride=1),
            BasicConv(i, (i // 2) * 3, kernel_size=3, stride=1, padding=1),
            BasicConv((i // 2) * 3, 2 * i, kernel_size=3, stride=stride, padding=1),
            BasicConv(2 * i, 2 * i, kernel_size=3, stride=1, padding=d1, dilation=d1, relu=False),
        )
        self.ConvLinear = BasicConv(4 * i, out_planes, kernel_size=1, stride=1, relu=False)
        self.shortcut = BasicConv(in_planes, out_planes, kernel_size=1, stride=stride, relu=False)
        self.relu = nn.ReLU(inplace=False)

    def forward(self, x):
        out = self.ConvLinear(torch.cat((self.branch0(x), self.branch1(x)), 1))
        return self.relu(out * self.scale + self.shortcut(x))
