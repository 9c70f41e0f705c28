"""Generate the ShuffleNetV2 fixtures (tests/golden/net_<case>.npz for cases_shufflenet.NET_CASES and BACKBONE_CASES) by running the
REFERENCE's own ``ShuffleNetV2_x1`` / ``_x2`` -- under its ``SSDFPN`` / ``YOLOV3`` and on their own -- like make_golden_densenet.py does for DenseNet121.

Run in the build container only (needs the reference checkout and torch CPU):

    python tests/golden/make_golden_shufflenet.py

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

import cases_shufflenet as cases  # noqa: E402

torch.set_num_threads(max(1, min(8, os.cpu_count() or 1)))
F32 = np.float32
MAX_ZERO_FRACTION = 0.95  # tests/planaudit.py: an fp32 map with more zeros than this is a dead layer


def t(x):
    return torch.from_numpy(np.ascontiguousarray(x))


def _reference_shufflenet():
    """The reference's ``nets`` package star-imports every backbone family (torchvision subclasses); it is registered as an empty
    namespace and only its shufflenet module is loaded (as make_golden_densenet._reference_densenet does)."""
    import tv_shim
    import tv_shim_shufflenet

    tv_shim.install()
    tv_shim_shufflenet.install()
    import ssds.modeling  # noqa: F401  (the reference's: REFERENCE is first on sys.path)

    pkg = types.ModuleType("ssds.modeling.nets")
    pkg.__path__ = [os.path.join(REFERENCE, "ssds", "modeling", "nets")]
    sys.modules["ssds.modeling.nets"] = pkg
    return importlib.import_module("ssds.modeling.nets.shufflenet")


def _seed_and_calibrate(model, seed, x):
    """Seeded weights, then the BatchNorm statistics as the cumulative average over two train-mode passes (make_golden.gen_nets).
    The classifier tail (``conv5.`` / ``fc.``) is never run by the reference's forward: it keeps its initial values and is left out
    of the schema."""
    sd = model.state_dict()
    spec = [(k, tuple(v.shape)) for k, v in sd.items() if not cases.is_tail(k)]
    assert len(spec) < len(sd), "the reference model has a conv5 / fc tail"
    model.load_state_dict({k: t(v) for k, v in cases.seeded_state(spec, seed).items()}, strict=False)
    for m in model.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.momentum = None
    model.train()
    with torch.no_grad():
        model(x)
        model(x)
    model.eval()
    out = {"keys": np.array([k for k, _ in spec]), "shapes": np.array([",".join(map(str, s)) for _, s in spec])}
    # The statistics are stored as ONE fp32 vector, the running_mean / running_var tensors in schema order
    # (cases_shufflenet.bn_state splits it by the schema): one zip member per statistic would triple the fixture.
    now = model.state_dict()
    out["bn_flat"] = np.concatenate([now[k].numpy().astype(F32).ravel() for k, _ in spec
                                     if k.endswith("running_mean") or k.endswith("running_var")])
    return out, sum(int(np.prod(s)) for _, s in spec)


def _check_backbone(name, backbone, x):
    """The conditions under which a comparison on this backbone decides something, asserted on the reference itself."""
    with torch.no_grad():
        maps = backbone(x)
        for i, o in enumerate(maps):
            zeros = float((o == 0).float().mean())
            assert bool(torch.isfinite(o).all()) and zeros < MAX_ZERO_FRACTION and float(o.std()) > 1e-3, (name, i, zeros, float(o.std()))
        print("   maps", [(tuple(o.shape), "rms %.2f" % float(o.pow(2).mean().sqrt()), "zeros %.3f" % float((o == 0).float().mean()))
                          for o in maps])
        h = backbone.maxpool(backbone.conv1(x))
        for level in range(2, max(backbone.outputs) + 1):
            for j, unit in enumerate(getattr(backbone, "stage%d" % level)):
                src = h if unit.stride > 1 else h.chunk(2, dim=1)[1]
                m = unit.branch2[2](unit.branch2[1](unit.branch2[0](src)))
                h = unit(h)
                print("      stage%d.%d %s zeros m %.3f  y rms %.3f zeros %.3f" % (level, j, tuple(h.shape[-2:]), float((m == 0).float().mean()),
                                                                               float(h.pow(2).mean().sqrt()), float((h == 0).float().mean())))


def _save(name, out):
    path = os.path.join(HERE, "net_" + name + ".npz")
    np.savez_compressed(path, **out)
    return os.path.getsize(path)


def gen_nets():
    from ssds.modeling import ssds as rssds

    rshuffle = _reference_shufflenet()
    for name, (seed, head, net, fl, A, C, _) in cases.NET_CASES.items():
        cls = getattr(rssds, head)
        nets_outputs, extras, hd = cls.add_extras(feature_layer=fl, mbox=[A] * len(fl[0]), num_classes=C)
        model = cls(backbone=getattr(rshuffle, net)(outputs=nets_outputs), extras=extras, head=hd, num_classes=C)
        x = t(cases.net_image(name))
        out, params = _seed_and_calibrate(model, seed, x)
        with torch.no_grad():
            loc, conf = model(x)
        for i, (l, c) in enumerate(zip(loc, conf)):
            out["loc%d" % i], out["conf%d" % i] = l.numpy(), c.numpy()
        assert all(np.isfinite(v).all() for k, v in out.items() if k[:3] in ("loc", "con"))
        print("net", name, "levels", [tuple(l.shape[-2:]) for l in loc], "params", params,
              "conf std", ["%.3f" % float(c.std()) for c in conf], "loc absmax", ["%.2f" % float(l.abs().max()) for l in loc],
              _save(name, out), "bytes")
        _check_backbone(name, model.backbone, x)
    for name, (seed, net, outputs, _) in cases.BACKBONE_CASES.items():
        model = getattr(rshuffle, net)(outputs=outputs)
        x = t(cases.net_image(name))
        out, params = _seed_and_calibrate(model, seed, x)
        with torch.no_grad():
            maps = model(x)
        for i, o in enumerate(maps):
            out["out%d" % i] = o.numpy()
        print("backbone", name, "maps", [tuple(o.shape[-2:]) for o in maps], "params", params, _save(name, out), "bytes")
        _check_backbone(name, model, x)


if __name__ == "__main__":
    gen_nets()
