"""Digest of the training step's routing: what ``train_ddp.Solver`` turns a config's model into under every routing switch (shared by
tests/test_route_digest_cpu.py and tests/golden/make_route_digest.py).

``canonical(cfg_name, setting)`` builds ``train_ddp.Solver(cfg, 0, torch.device("cpu"), sync_bn=...)`` -- nothing else of the project
is called, so the same file runs on the commit whose routing is the reference and on a rewrite of the code underneath -- and writes
down, one line per module of ``model.named_modules()``: its name, its class with the class's module, and the instance attributes
whose key starts with ``_ssdk_`` or ``native_`` (scalars by ``repr``, a module-valued one such as ``_ssdk_defer_to`` as the name of
the module it points to).  The last line is ``headconv.WGRAD_MIN_PIXELS``, the one module global the routing sets.  The golden file
stores the SHA-256 of that text per key; to see WHAT differs, print the text on both commits and diff:

    python tests/routedigest.py fpn_resnet50_640.yml/SSDK_DENSE3_TRAIN=0

``SETTINGS`` names the builds of every config: nothing set, each switch of ``SWITCHES`` alone at each of its values, and ``--sync-bn``
with nothing set, with SSDK_FAST_BN=0 (torch's SyncBatchNorm) and with SSDK_DENSE_TRAIN=1 (the dense block stays on the module path).
SSDK_PW_NATIVE is read by the layers' forward, not by the routing, and is left out."""
import collections
import contextlib
import glob
import hashlib
import io
import os
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG_DIR = os.path.join(ROOT, "experiments", "cfgs")

# switch -> (its values, the one an unset variable means; None: the model decides -- FPN / BiFPN 1, YOLO / Shelf 0)
SWITCHES = collections.OrderedDict(
    [(name, (("0", "1"), default)) for name, default in (
        ("SSDK_FAST_BN", "1"), ("SSDK_FUSE_BN_ACT", "1"), ("SSDK_BN_DEFER", "1"), ("SSDK_BN_STATS_FUSED", "1"), ("SSDK_SHUFFLE_TRAIN", "1"),
        ("SSDK_DENSE_TRAIN", "0"), ("SSDK_PW_GEMM", "1"), ("SSDK_GCONV_TRAIN", "1"), ("SSDK_STEM7_TRAIN", "0"), ("SSDK_MBCONV_TRAIN", "1"),
        ("SSDK_HEAD_PAIR", "1"), ("SSDK_DENSE3_TRAIN", None), ("SSDK_NECK_TRAIN", "1"), ("SSDK_CAT_TRAIN", "1"), ("SSDK_CONVT_TRAIN", "0"))]
    + [("SSDK_CONV3_NATIVE", (("0", "1", "2"), "2"))])

Setting = collections.namedtuple("Setting", "env sync_bn")


def _settings():
    out = collections.OrderedDict([("unset", Setting({}, False))])
    for name, (values, _) in SWITCHES.items():
        for v in values:
            out["%s=%s" % (name, v)] = Setting({name: v}, False)
    out["sync_bn"] = Setting({}, True)
    out["sync_bn,SSDK_FAST_BN=0"] = Setting({"SSDK_FAST_BN": "0"}, True)
    out["sync_bn,SSDK_DENSE_TRAIN=1"] = Setting({"SSDK_DENSE_TRAIN": "1"}, True)
    return out


SETTINGS = _settings()


def configs():
    return sorted(os.path.basename(p) for p in glob.glob(os.path.join(CFG_DIR, "*.yml")))


def keys(cfg_names=None):
    return ["%s/%s" % (c, s) for c in (configs() if cfg_names is None else cfg_names) for s in SETTINGS]


@contextlib.contextmanager
def _isolated(env):
    """None of the listed switches set but those of ``env``, WGRAD_MIN_PIXELS back at 0, the Solver's prints swallowed."""
    from ssds.modeling.layers import headconv

    saved = {k: os.environ.pop(k) for k in SWITCHES if k in os.environ}
    os.environ.update(env)
    pixels, headconv.WGRAD_MIN_PIXELS = headconv.WGRAD_MIN_PIXELS, 0
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            yield
    finally:
        for k in env:
            os.environ.pop(k, None)
        os.environ.update(saved)
        headconv.WGRAD_MIN_PIXELS = pixels


def _value(v, names):
    if v is None or isinstance(v, (bool, int, float, str)):
        return repr(v)
    if isinstance(v, torch.nn.Module):
        return "->" + names.get(id(v), "<a module outside the model>")
    return "<%s>" % type(v).__name__


def model_text(model):
    named = list(model.named_modules())
    names = {id(m): n for n, m in named}
    lines = []
    for name, m in named:
        attrs = ["%s=%s" % (k, _value(v, names)) for k, v in sorted(vars(m).items()) if k.startswith(("_ssdk_", "native_"))]
        lines.append(" ".join([name or ".", type(m).__module__ + "." + type(m).__qualname__] + attrs))
    return lines


def canonical(cfg_name, setting):
    """The text of one key: the Solver-built model of ``cfg_name`` under ``SETTINGS[setting]``."""
    from ssds.core import config
    from ssds.modeling.layers import headconv
    from ssds.utils import train_ddp

    s = SETTINGS[setting]
    with tempfile.TemporaryDirectory() as tmp, _isolated(s.env):
        cfg = config.cfg_from_file(os.path.join(CFG_DIR, cfg_name))
        cfg.EXP_DIR = tmp  # a stray checkpoint of the config's own directory cannot change the build
        solver = train_ddp.Solver(cfg, 0, torch.device("cpu"), sync_bn=s.sync_bn)
        lines = model_text(solver.model) + ["WGRAD_MIN_PIXELS=%r" % headconv.WGRAD_MIN_PIXELS]
    return "\n".join(lines) + "\n"


def digest(text):
    return hashlib.sha256(text.encode()).hexdigest()


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(ROOT, "ssds.pytorch_amd"))
    cfg_name, _, setting = sys.argv[1].partition("/")
    sys.stdout.write(canonical(cfg_name, setting))
