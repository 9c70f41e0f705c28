"""Generate the RFB fixtures by running the REFERENCE's own classes, unmodified: tests/golden/net_<case>.npz for
cases_rfb.NET_CASES (``SSD`` / ``SSDShelf`` whose extras come from the reference's ``parse_feature_layer``), rfb_blocks.npz for
cases_rfb.BLOCK_CASES (single ``BasicRFB`` blocks) and rfb_state_keys.txt (the block's ``state_dict`` keys and shapes).

Run in the build container only (needs the reference checkout and torch CPU):

    python tests/golden/make_golden_rfb.py

Nothing in the test-suite imports this file."""
import importlib
import os
import sys
import types
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
# the reference checkout: SSDS_REFERENCE, or a `reference` directory next to this repository
REFERENCE = os.environ.get("SSDS_REFERENCE") or os.path.abspath(os.path.join(HERE, "..", "..", "..", "reference"))
sys.path.insert(0, HERE)
sys.path.insert(0, REFERENCE)
warnings.filterwarnings("ignore")

import cases_rfb as cases  # noqa: E402

torch.set_num_threads(1)
F32 = np.float32


def t(x):
    return torch.from_numpy(np.ascontiguousarray(x))


class _Stub(torch.nn.Module):
    """Backbone stand-in of the ``*_stub`` cases: returns the seeded feature maps whatever the image."""

    def __init__(self, feats):
        super().__init__()
        self.feats = feats

    def initialize(self):
        pass

    def forward(self, x):
        return [f.clone() for f in self.feats]


def _reference_nets():
    """The reference's ``nets`` package star-imports every backbone family (torchvision subclasses); it is registered as an
    empty namespace and only its resnet module is loaded, on top of ``tv_shim`` (as make_golden._reference_nets does)."""
    import tv_shim

    tv_shim.install()
    import ssds.modeling  # noqa: F401  (the reference's: REFERENCE is first on sys.path)

    pkg = types.ModuleType("ssds.modeling.nets")
    pkg.__path__ = [os.path.join(REFERENCE, "ssds", "modeling", "nets")]
    sys.modules["ssds.modeling.nets"] = pkg
    mod = importlib.import_module("ssds.modeling.nets.resnet")
    return {n: getattr(mod, n) for n in mod.__all__}


def _calibrate(model, x):
    """BatchNorm calibration: cumulative average over two train-mode passes (make_golden.gen_nets); -> the eval-mode output."""
    for m in model.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.momentum = None
    drops = [m for m in model.modules() if isinstance(m, torch.nn.Dropout2d)]
    kept = [m.p for m in drops]
    for m in drops:  # (the Dropout2d inside every SharedBlock of the Shelf neck would make the calibration passes random)
        m.p = 0.0
    model.train()
    with torch.no_grad():
        model(x)
        model(x)
    for m, p in zip(drops, kept):
        m.p = p
    model.eval()
    with torch.no_grad():
        return model(x)


def _bn_stats(model, prefix):
    return {prefix + k: v.numpy().astype(F32) for k, v in model.state_dict().items()
            if k.endswith("running_mean") or k.endswith("running_var")}


def gen_nets():
    from ssds.modeling import ssds as rssds
    from ssds.modeling.layers.rfb_layers import BasicRFB

    rnets = _reference_nets()
    for name, (seed, head, net, fl, A, C, (B, H, W)) in cases.NET_CASES.items():
        cls = getattr(rssds, head)
        nets_outputs, extras, hd = cls.add_extras(feature_layer=fl, mbox=[A] * len(fl[0]), num_classes=C)
        if net == "stub":
            backbone = _Stub([t(f) for f in cases.stub_features(name)])
        else:
            backbone = rnets[net](outputs=nets_outputs)
            backbone.url = None  # no network: skip the ImageNet download of initialize()
        model = cls(backbone=backbone, extras=extras, head=hd, num_classes=C)
        assert sum(isinstance(m, BasicRFB) for m in model.modules()) == sum(isinstance(s, str) and s.startswith("RBF") for s in fl[0])
        sd = model.state_dict()
        spec = [(k, tuple(v.shape)) for k, v in sd.items()]
        model.load_state_dict({k: t(v) for k, v in cases.seeded_state(spec, seed).items()})
        loc, conf = _calibrate(model, t(cases.net_image(name)))
        out = {"keys": np.array([k for k, _ in spec]), "shapes": np.array([",".join(map(str, s)) for _, s in spec])}
        out.update(_bn_stats(model, "bn/"))
        for i, (l, c) in enumerate(zip(loc, conf)):
            out["loc%d" % i], out["conf%d" % i] = l.numpy(), c.numpy()
        assert all(np.isfinite(v).all() for k, v in out.items() if k[:3] in ("loc", "con"))
        path = os.path.join(HERE, "net_" + name + ".npz")
        np.savez_compressed(path, **out)
        print("net", name, "levels", [tuple(l.shape[-2:]) for l in loc], "params", sum(v.numel() for v in sd.values()),
              "conf std", ["%.3f" % float(c.std()) for c in conf], "loc absmax", ["%.2f" % float(l.abs().max()) for l in loc],
              os.path.getsize(path), "bytes")


def gen_blocks():
    from ssds.modeling.layers.rfb_layers import BasicRFB

    out = {}
    for name, (seed, cin, cout, stride, scale, visual, _) in cases.BLOCK_CASES.items():
        blk = BasicRFB(cin, cout, stride=stride, scale=scale, visual=visual)
        spec = [(k, tuple(v.shape)) for k, v in blk.state_dict().items()]
        blk.load_state_dict({k: t(v) for k, v in cases.seeded_state(spec, seed).items()})
        y = _calibrate(blk, t(cases.block_input(name)))
        out.update(_bn_stats(blk, name + "/bn/"))
        out[name + "/y"] = y.numpy()
        assert np.isfinite(out[name + "/y"]).all()
        print("block", name, tuple(y.shape), "rms %.3f" % float(y.pow(2).mean().sqrt()), "zeros %.2f" % float((y == 0).float().mean()))
    path = os.path.join(HERE, "rfb_blocks.npz")
    np.savez_compressed(path, **out)
    print(os.path.getsize(path), "bytes")
    cin, cout, stride, scale, visual = cases.STATE_KEYS_BLOCK
    blk = BasicRFB(cin, cout, stride=stride, scale=scale, visual=visual)
    with open(os.path.join(HERE, "rfb_state_keys.txt"), "w") as f:
        for k, v in blk.state_dict().items():
            f.write("%s %s\n" % (k, ",".join(map(str, v.shape))))


if __name__ == "__main__":
    gen_blocks()
    gen_nets()
