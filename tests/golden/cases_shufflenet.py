"""Cases of the ShuffleNetV2 backbones (the reference's ``ssds/modeling/nets/shufflenet.py``) under the reference's ``SSDFPN`` / ``YOLOV3``
and on their own (fixtures tests/golden/net_<case>.npz written by make_golden_shufflenet.py).  ``NET_CASES`` has the tuple layout of
``cases.NET_CASES`` / ``cases_densenet.NET_CASES``; ``BACKBONE_CASES`` holds the bare backbone.  The weights come from
``cases.seeded_state`` and the images from the case's seed, so the fixtures hold only the schema (without the keys of the
classifier tail ``conv5.`` / ``fc.``, which no detector runs), the calibrated BatchNorm statistics and the outputs.

96 x 64 images give the maps 12 x 8, 6 x 4 and 3 x 2 of stages 2, 3, 4 (and, through ``Conv:S``, 2 x 1 and 1 x 1 under FPN).

The seeded state is ``cases.seeded_state`` unchanged: the generator asserts on the REFERENCE, per backbone map, that it is finite, not
constant and has fewer than 95 % zeros, and prints per unit the zero fraction of branch2's middle map; a case whose seed fails that is
given another seed here."""
from collections import OrderedDict

import numpy as np

from cases import seeded_state  # noqa: F401  (re-exported: the tests and the generator take it from here)

# name: (seed, head class, backbone factory, FEATURE_LAYER, anchors per location, classes, (B, H, W))
NET_CASES = OrderedDict(
    [
        ("fpn_sfv2x1", (151, "SSDFPN", "ShuffleNetV2_x1", [[2, 3, 4, "Conv:S", "Conv:S"], [116, 232, 464, 464, 256]], 9, 3, (2, 96, 64))),
        ("yolov3_sfv2x2", (152, "YOLOV3", "ShuffleNetV2_x2", [[2, 3, 4], [244, 488, 976]], 9, 3, (2, 96, 64))),
    ]
)

# name: (seed, backbone factory, outputs, (B, H, W)): fixture keys ``out<i>`` instead of ``loc<i>`` / ``conf<i>``.  Levels 3 and 4 only
# (6 x 4 and 3 x 2), as dn121_bare drops its largest map.
BACKBONE_CASES = OrderedDict([("sfv2x1_bare", (153, "ShuffleNetV2_x1", [3, 4], (2, 96, 64)))])

TAIL_PREFIXES = ("conv5.", "fc.")  # the classifier tail of torchvision's ShuffleNetV2: not in the schema, not in the package's module


def is_tail(key):
    """``conv5.*`` / ``fc.*`` of the backbone, bare or as ``backbone.<key>`` inside a detector."""
    key = key[len("backbone."):] if key.startswith("backbone.") else key
    return key.startswith(TAIL_PREFIXES)


def net_image(name):
    B, H, W = (NET_CASES[name] if name in NET_CASES else BACKBONE_CASES[name])[-1]
    seed = (NET_CASES[name] if name in NET_CASES else BACKBONE_CASES[name])[0]
    return np.random.RandomState(seed).random_sample((B, 3, H, W)).astype(np.float32)


def bn_state(fx):
    """{state_dict key: calibrated running_mean / running_var} of a fixture: ``bn_flat`` is their concatenation in schema order."""
    flat, at, out = fx["bn_flat"], 0, {}
    for k, sh in zip(fx["keys"], fx["shapes"]):
        k = str(k)
        if k.endswith("running_mean") or k.endswith("running_var"):
            n = int(str(sh))
            out[k] = flat[at:at + n]
            at += n
    assert at == flat.size, (at, flat.size)
    return out
