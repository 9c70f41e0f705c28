"""Whole-detector cases of the YOLO detectors (the reference's ``YOLOV3`` / ``YOLOV4``, ssds/modeling/ssds/yolo.py; fixtures
tests/golden/net_<case>.npz written by make_golden_yolo.py).  Same tuple layout as ``cases.NET_CASES``; the weights come from
``cases.seeded_state`` and the inputs from the case's seed, so the fixtures hold only the schema, the calibrated BatchNorm
statistics and the outputs.

Both necks concatenate a map with the nearest-x2 upsample of the next one, so every map must be an exact half of the one before
it: the stub maps are ``H // stride`` with strides 8, 16, 32 (16 x 12, 8 x 6, 4 x 3 -- the SPP block of ``yolov4_stub`` runs on
a map smaller than each of its windows), and the ResNet18 images are multiples of 32.  ``yolov4_stub`` stacks two PAN modules.

The seeded state is ``cases.seeded_state`` unchanged: the generator prints per-level conf std (0.12 ... 0.19 on sigmoid
outputs) and loc abs-max (1.4 ... 5.3), finite and non-constant on every level of all four cases."""
from collections import OrderedDict

import numpy as np

from cases import seeded_state  # noqa: F401  (re-exported: the tests and the generator take it from here)

# name: (seed, head class, backbone factory | "stub", FEATURE_LAYER, anchors per location, classes, (B, H, W))
NET_CASES = OrderedDict(
    [
        ("yolov3_stub", (121, "YOLOV3", "stub", [[0, 1, 2, "Conv:S"], [32, 64, 128, 64]], 3, 4, (2, 128, 96))),
        ("yolov4_stub", (122, "YOLOV4", "stub", [[0, 1, 2, "Conv:S"], [32, 64, 128, 64], 2], 3, 4, (2, 128, 96))),
        ("yolov3_r18", (123, "YOLOV3", "ResNet18", [[3, 4, 5], [128, 256, 512]], 9, 3, (2, 96, 64))),
        ("yolov4_r18", (124, "YOLOV4", "ResNet18", [[3, 4, 5, "Conv:S"], [128, 256, 512, 256]], 9, 3, (2, 160, 96))),
    ]
)


def net_image(name):
    seed, _, _, _, _, _, (B, H, W) = NET_CASES[name]
    return np.random.RandomState(seed).random_sample((B, 3, H, W)).astype(np.float32)


def stub_features(name):
    """Feature map l of a stub backbone: stride 8 * 2**l, the channel count FEATURE_LAYER names for it."""
    seed, _, net, fl, _, _, (B, H, W) = NET_CASES[name]
    assert net == "stub"
    rs = np.random.RandomState(seed + 1000)
    feats = []
    for l, (layer, depth) in enumerate(zip(*fl[:2])):
        if isinstance(layer, int):
            s = 8 << l
            feats.append((rs.standard_normal((B, depth, H // s, W // s)) * 0.7).astype(np.float32))
    return feats
