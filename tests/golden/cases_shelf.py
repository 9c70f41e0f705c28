"""Whole-detector cases of the Shelf detector (the reference's ``SSDShelf``, ssds/modeling/ssds/shelf.py; fixtures
tests/golden/net_<case>.npz written by make_golden_shelf.py).  Same tuple layout as ``cases.NET_CASES``; the weights come
from ``cases.seeded_state`` and the inputs from the case's seed, so the fixtures hold only the schema, the calibrated
BatchNorm statistics and the outputs.

The transposed convolution of the Shelf decoder (3 x 3, stride 2, padding 1, no output padding) turns an ``h x w`` map into
``(2h - 1) x (2w - 1)``, and the reference adds the next level to it: every map must be exactly ``2h - 1`` of the next.
``cases.stub_features`` builds maps of ``H // stride`` (exact halves), so the stub maps are given explicitly here, and the
ResNet18 case uses an image of 129 x 97 (129 -> 65 -> 33 -> 17 -> 9 -> 5, 97 -> 49 -> 25 -> 13 -> 7 -> 4).

The seeded state is ``cases.seeded_state`` unchanged: the generator prints per-level conf std (0.12 ... 0.20 on
sigmoid outputs) and loc abs-max (1.6 ... 4.7), finite and non-constant on every level of both cases, so no BatchNorm weight
had to be rescaled."""
from collections import OrderedDict

import numpy as np

from cases import seeded_state  # noqa: F401  (re-exported: the tests and the generator take it from here)

# name: (seed, head class, backbone factory | "stub", FEATURE_LAYER, anchors per location, classes, (B, H, W))
NET_CASES = OrderedDict(
    [
        ("shelf_stub", (111, "SSDShelf", "stub", [[0, 1, 2, "Conv:S"], [24, 40, 64, 48]], 3, 4, (2, 136, 104))),
        ("shelf_r18", (112, "SSDShelf", "ResNet18", [[3, 4, 5, "Conv:S"], [128, 256, 512, 256]], 9, 3, (2, 129, 97))),
    ]
)
# feature maps of the stub backbones, largest first: each is 2h - 1 of the next
STUB_MAPS = {"shelf_stub": ((17, 13), (9, 7), (5, 4))}


def net_image(name):
    seed, _, _, _, _, _, (B, H, W) = NET_CASES[name]
    return np.random.RandomState(seed).random_sample((B, 3, H, W)).astype(np.float32)


def stub_features(name):
    seed, _, net, fl, _, _, (B, _, _) = NET_CASES[name]
    assert net == "stub"
    rs = np.random.RandomState(seed + 1000)
    depths = [d for layer, d in zip(*fl[:2]) if isinstance(layer, int)]
    return [(rs.standard_normal((B, d, h, w)) * 0.7).astype(np.float32) for d, (h, w) in zip(depths, STUB_MAPS[name])]
