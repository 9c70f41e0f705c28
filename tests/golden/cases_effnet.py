"""Whole-detector cases on the EfficientNet backbones (the reference's SSD / SSDFPN / SSDBiFPN around its own
``nets/efficientnet.py``; fixtures tests/golden/net_<case>.npz written by make_golden_effnet.py).  Same tuple layout as
``cases.NET_CASES``; the weights come from ``cases.seeded_state`` and the image from the case's seed, so the fixtures hold
only the schema, the calibrated BatchNorm statistics and the outputs."""
from collections import OrderedDict

import numpy as np

from cases import seeded_state  # noqa: F401  (re-exported: the tests and the generator take it from here)

# name: (seed, head class, backbone factory, FEATURE_LAYER, anchors per location, classes, (B, H, W))
NET_CASES = OrderedDict(
    [
        ("bifpn_effb0", (101, "SSDBiFPN", "EfficientNetB0", [[3, 5, 7, "Conv:S", "Conv:S"], [40, 112, 320, 320, 256]], 9, 3,
                         (2, 128, 128))),
        ("fpn_effb2", (102, "SSDFPN", "EfficientNetB2", [[3, 5, 7, "Conv:S", "Conv:S"], [48, 120, 352, 352, 256]], 9, 3,
                       (2, 96, 128))),
        ("ssd_effb0", (103, "SSD", "EfficientNetB0", [[5, 7, "Conv:S"], [112, 320, 256]], 6, 4, (2, 128, 128))),
    ]
)


def net_image(name):
    seed, _, _, _, _, _, (B, H, W) = NET_CASES[name]
    return np.random.RandomState(seed).random_sample((B, 3, H, W)).astype(np.float32)
