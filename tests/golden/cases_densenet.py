"""Cases of the DenseNet121 backbone (the reference's ``ssds/modeling/nets/densenet.py``) under the reference's ``SSDFPN`` / ``YOLOV3``
and on its own (fixtures tests/golden/net_<case>.npz written by make_golden_densenet.py).  ``NET_CASES`` has the tuple layout of
``cases.NET_CASES`` / ``cases_darknet.NET_CASES``; ``BACKBONE_CASES`` holds the bare backbone.  The weights come from
``cases.seeded_state`` and the images from the case's seed, so the fixtures hold only the schema, the calibrated BatchNorm statistics
and the outputs.

96 x 64 images give the maps 12 x 8, 6 x 4 and 3 x 2 of dense blocks 2, 3, 4 (and, through ``Conv:S``, 2 x 1 and 1 x 1 under FPN).

The seeded state is ``cases.seeded_state`` unchanged: the generator asserts on the REFERENCE, per backbone map, that it is finite, not
constant and has fewer than 95 % zeros, and prints per dense layer the zero fraction of ``relu(norm1(.))`` and of the middle map."""
from collections import OrderedDict

import numpy as np

from cases import seeded_state  # noqa: F401  (re-exported: the tests and the generator take it from here)

# name: (seed, head class, backbone factory, FEATURE_LAYER, anchors per location, classes, (B, H, W))
NET_CASES = OrderedDict(
    [
        ("fpn_dn121", (141, "SSDFPN", "DenseNet121", [[2, 3, 4, "Conv:S", "Conv:S"], [512, 1024, 1024, 1024, 256]], 9, 3, (2, 96, 64))),
        ("yolov3_dn121", (142, "YOLOV3", "DenseNet121", [[2, 3, 4], [512, 1024, 1024]], 9, 3, (2, 96, 64))),
    ]
)

# name: (seed, backbone factory, outputs, (B, H, W)): fixture keys ``out<i>`` instead of ``loc<i>`` / ``conf<i>``.  Levels 3 and 4 only
# (6 x 4 and 3 x 2), as dk53_bare drops its largest map.
BACKBONE_CASES = OrderedDict([("dn121_bare", (143, "DenseNet121", [3, 4], (2, 96, 64)))])


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
