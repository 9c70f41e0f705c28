"""Generate the DarkNet53 fixtures (tests/golden/net_<case>.npz for cases_darknet.NET_CASES and BACKBONE_CASES) by running the
REFERENCE's own ``DarkNet53`` -- under its ``YOLOV3`` / ``YOLOV4`` and on its own -- like make_golden_yolo.gen_nets does for the
ResNet18 cases.

Run in the build container only (needs the reference checkout and torch CPU):

    python tests/golden/make_golden_darknet.py

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

import cases_darknet as cases  # noqa: E402

torch.set_num_threads(max(1, min(8, os.cpu_count() or 1)))
F32 = np.float32
MAX_ZERO_FRACTION = 0.95  # tests/planaudit.py: an fp32 map with more zeros than this is a dead layer


def t(x):
    return torch.from_numpy(np.ascontiguousarray(x))


def _reference_darknet():
    """The reference's ``nets`` package star-imports every backbone family (torchvision subclasses); it is registered as an empty
    namespace and only its darknet module is loaded (as make_golden_yolo._reference_nets does for resnet)."""
    import tv_shim

    tv_shim.install()
    import ssds.modeling  # noqa: F401  (the reference's: REFERENCE is first on sys.path)

    pkg = types.ModuleType("ssds.modeling.nets")
    pkg.__path__ = [os.path.join(REFERENCE, "ssds", "modeling", "nets")]
    sys.modules["ssds.modeling.nets"] = pkg
    return importlib.import_module("ssds.modeling.nets.darknet")


def _seed_and_calibrate(model, seed, x):
    """Seeded weights, then the BatchNorm statistics as the cumulative average over two train-mode passes (make_golden.gen_nets)."""
    sd = model.state_dict()
    spec = [(k, tuple(v.shape)) for k, v in sd.items()]
    model.load_state_dict({k: t(v) for k, v in cases.seeded_state(spec, seed).items()})
    for m in model.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.momentum = None
    model.train()
    with torch.no_grad():
        model(x)
        model(x)
    model.eval()
    out = {"keys": np.array([k for k, _ in spec]), "shapes": np.array([",".join(map(str, s)) for _, s in spec])}
    for k, v in model.state_dict().items():
        if k.endswith("running_mean") or k.endswith("running_var"):
            out["bn/" + k] = v.numpy().astype(F32)
    return out, sum(v.numel() for v in sd.values())


def _check_backbone(name, backbone, x):
    """The conditions under which a comparison on this backbone decides something, asserted on the reference itself."""
    with torch.no_grad():
        maps = backbone(x)
        for i, o in enumerate(maps):
            zeros = float((o == 0).float().mean())
            assert bool(torch.isfinite(o).all()) and zeros < MAX_ZERO_FRACTION and float(o.std()) > 1e-3, (name, i, zeros)
        print("   maps", [(tuple(o.shape[-2:]), "rms %.2f" % float(o.pow(2).mean().sqrt()), "zeros %.3f" % float((o == 0).float().mean()))
                          for o in maps])
        h, rows = backbone.conv1(x), []
        for level in range(1, max(backbone.outputs) + 1):
            for j, blk in enumerate(getattr(backbone, "block%d" % level)):
                if j == 0:
                    h = blk(h)
                    continue
                br = blk.conv3x3(blk.conv1x1(h))
                rows.append((float((br == 0).float().mean()), float((br == 6).float().mean()), float(br.pow(2).mean().sqrt()),
                             float(h.pow(2).mean().sqrt())))
                h = br + h
        r = np.array(rows)
        print("   %d residuals: branch zeros %.2f-%.2f, at 6 <= %.4f, branch rms %.2f-%.2f, x rms %.2f-%.2f" % (
            len(rows), r[:, 0].min(), r[:, 0].max(), r[:, 1].max(), r[:, 2].min(), r[:, 2].max(), r[:, 3].min(), r[:, 3].max()))


def _save(name, out):
    path = os.path.join(HERE, "net_" + name + ".npz")
    np.savez_compressed(path, **out)
    return os.path.getsize(path)


def gen_nets():
    from ssds.modeling import ssds as rssds

    rdark = _reference_darknet()
    for name, (seed, head, net, fl, A, C, _) in cases.NET_CASES.items():
        cls = getattr(rssds, head)
        nets_outputs, extras, hd = cls.add_extras(feature_layer=fl, mbox=[A] * len(fl[0]), num_classes=C)
        model = cls(backbone=getattr(rdark, net)(outputs=nets_outputs), extras=extras, head=hd, num_classes=C)
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
        model = getattr(rdark, net)(outputs=outputs)
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
