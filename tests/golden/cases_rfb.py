"""Cases of the RFB extra layers (the reference's ``BasicRFB``, ssds/modeling/layers/rfb_layers.py, reached through the
FEATURE_LAYER strings "RBF" and "RBF:S"; fixtures tests/golden/net_<case>.npz, rfb_blocks.npz and rfb_state_keys.txt written by
make_golden_rfb.py).  ``NET_CASES`` has the tuple layout of ``cases.NET_CASES``; the weights come from ``cases.seeded_state`` and
the inputs from the case's seed, so the fixtures hold only the schema, the calibrated BatchNorm statistics and the outputs.

Every ``in_planes`` is a multiple of 128 (the widths inside a block are multiples of 8 exactly then: the plan's condition).

* ``ssd_rfb_stub``: one stub map of 7 x 5, a stride-1 "RBF" (7 x 5), two "RBF:S" (4 x 3, 2 x 2) and a "Conv:S" (1 x 1).  The last
  RFB level, 2 x 2, is smaller than dilation 3 both ways: only the centre taps of its dilated convolutions are inside the map.
* ``ssd_rfb_r18``: ResNet18 at 160 x 96 -> 20 x 12, 10 x 6, 5 x 3, then "RBF:S" -> 3 x 2 -> 2 x 1.
* ``shelf_rfb_stub``: the Shelf neck on stub maps that are 2h - 1 of the next (17 x 13, 9 x 7, 5 x 4), then "RBF:S" -> 3 x 2.

``BLOCK_CASES``: single blocks, the reference's fp32 output for a seeded input -- three through the parser's arguments (scale 1.0,
visual 2: dilations 3 and 5) and one with the constructor's defaults (scale 0.1, visual 1: dilations 2 and 3)."""
from collections import OrderedDict

import numpy as np

from cases import seeded_state  # noqa: F401  (re-exported: the tests and the generator take it from here)

# name: (seed, head class, backbone factory | "stub", FEATURE_LAYER, anchors per location, classes, (B, H, W))
NET_CASES = OrderedDict(
    [
        ("ssd_rfb_stub", (131, "SSD", "stub", [[0, "RBF", "RBF:S", "RBF:S", "Conv:S"], [128, 128, 256, 128, 64]], 6, 5, (2, 56, 40))),
        ("ssd_rfb_r18", (132, "SSD", "ResNet18", [[3, 4, 5, "RBF:S", "RBF:S"], [128, 256, 512, 512, 256]], 6, 4, (2, 160, 96))),
        ("shelf_rfb_stub", (133, "SSDShelf", "stub", [[0, 1, 2, "RBF:S"], [24, 40, 128, 128]], 3, 4, (2, 136, 104))),
    ]
)
# feature maps of the stub backbones, largest first
STUB_MAPS = {"ssd_rfb_stub": ((7, 5),), "shelf_rfb_stub": ((17, 13), (9, 7), (5, 4))}

# name: (seed, in_planes, out_planes, stride, scale, visual, (B, H, W))
BLOCK_CASES = OrderedDict(
    [
        ("b128_s1_7x5", (141, 128, 128, 1, 1.0, 2, (2, 7, 5))),
        ("b256_s2_5x3", (142, 256, 128, 2, 1.0, 2, (2, 5, 3))),
        ("b256_s2_1x1", (143, 256, 256, 2, 1.0, 2, (8, 1, 1))),  # (8 images: BatchNorm is calibrated on B H W values per channel)
        ("b128_s2_scale01", (144, 128, 256, 2, 0.1, 1, (2, 5, 3))),
    ]
)
# the block whose state_dict keys and shapes rfb_state_keys.txt lists
STATE_KEYS_BLOCK = (256, 128, 2, 1.0, 2)


def net_image(name):
    seed, _, _, _, _, _, (B, H, W) = NET_CASES[name]
    return np.random.RandomState(seed).random_sample((B, 3, H, W)).astype(np.float32)


def stub_features(name):
    seed, _, net, fl, _, _, (B, _, _) = NET_CASES[name]
    assert net == "stub"
    rs = np.random.RandomState(seed + 1000)
    depths = [d for layer, d in zip(*fl[:2]) if isinstance(layer, int)]
    return [(rs.standard_normal((B, d, h, w)) * 0.7).astype(np.float32) for d, (h, w) in zip(depths, STUB_MAPS[name])]


def block_input(name):
    seed, cin, _, _, _, _, (B, H, W) = BLOCK_CASES[name]
    return (np.random.RandomState(seed + 1000).standard_normal((B, cin, H, W)) * 0.7).astype(np.float32)
