"""Cases of the DarkNet53 backbone (the reference's ``ssds/modeling/nets/darknet.py``) under the reference's ``YOLOV3`` / ``YOLOV4``
and on its own (fixtures tests/golden/net_<case>.npz written by make_golden_darknet.py).  ``NET_CASES`` has the tuple layout of
``cases.NET_CASES`` / ``cases_yolo.NET_CASES``; ``BACKBONE_CASES`` holds the bare backbone.  The weights come from
``cases.seeded_state`` and the images from the case's seed, so the fixtures hold only the schema, the calibrated BatchNorm statistics
(17 856 channels in the backbone) and the outputs.

Image sides are multiples of 32 (the YOLO necks need every map to be an exact half of the one before it): 96 x 64 gives the maps
12 x 8, 6 x 4 and 3 x 2; 160 x 96 gives 20 x 12, 10 x 6, 5 x 3 and, through ``Conv:S``, 3 x 2.

The seeded state is ``cases.seeded_state`` unchanged: the generator asserts on the REFERENCE, per backbone map, that it is finite, not
constant and has fewer than 95 % zeros, and prints per residual block the zero fraction of the branch (49 - 50 %) and the RMS of
branch and input."""
from collections import OrderedDict

import numpy as np

from cases import seeded_state  # noqa: F401  (re-exported: the tests and the generator take it from here)

# name: (seed, head class, backbone factory, FEATURE_LAYER, anchors per location, classes, (B, H, W))
NET_CASES = OrderedDict(
    [
        ("yolov3_dk53", (131, "YOLOV3", "DarkNet53", [[3, 4, 5], [256, 512, 1024]], 9, 3, (2, 96, 64))),
        ("yolov4_dk53", (132, "YOLOV4", "DarkNet53", [[3, 4, 5, "Conv:S"], [256, 512, 1024, 512]], 9, 3, (2, 160, 96))),
    ]
)

# name: (seed, backbone factory, outputs, (B, H, W)): fixture keys ``out<i>`` instead of ``loc<i>`` / ``conf<i>``.  Levels 4 and 5 only
# (6 x 4 and 3 x 2): with the 12 x 8 map of level 3 the file would be larger than any other fixture.
BACKBONE_CASES = OrderedDict([("dk53_bare", (133, "DarkNet53", [4, 5], (2, 96, 64)))])


def net_image(name):
    B, H, W = (NET_CASES[name] if name in NET_CASES else BACKBONE_CASES[name])[-1]
    seed = (NET_CASES[name] if name in NET_CASES else BACKBONE_CASES[name])[0]
    return np.random.RandomState(seed).random_sample((B, 3, H, W)).astype(np.float32)
