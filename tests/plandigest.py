"""Digest of a recorded plan: everything the C executor sees of it (shared by tests/test_plan_digest_cpu.py and
tests/golden/make_plan_digest.py).

The executor reads nothing of a ``ConvPlan`` but the ``ssdk_op`` array, the patch list, the head list and the sizes of the arena's
buffers.  ``canonical(plan)`` writes those down so that two recordings can be compared across commits and processes: every op as its
raw bytes in 8-byte words, a word that is an address replaced by WHERE it points --

  A<i>+<offset>       inside arena buffer i (allocation order),
  <path>+<offset>     inside a tensor reached from ``plan.keep`` (K[...]) or a layer dict (L<i>[...]) by walking lists, dicts, slots and
                      attributes -- the cached ``ConvPack._frag`` / ``MbPack._image`` and the ``a`` / ``b`` of a densepool included;
                      the path is structural (``K[12].scale``), never derived from a tensor's contents,

every other word in hex.  The helper reads raw words on purpose: it does not know which union member a kind uses and shares no
knowledge with the code that filled them.  A pointer it failed to resolve would be printed in hex and differ between two recordings,
so ``record(...)`` records every plan TWICE in one process (the addresses then differ) and asserts that the two texts are equal.

``PLANS`` names the recordings: every case of ``NET_CASES`` / ``BACKBONE_CASES`` of tests/golden/cases*.py in bf16 with no switch set,
a subset in fp16 and under SSDK_DKRES=0 / 1, SSDK_WFRAG=0, a lowered planner.SMALL_LEVEL_PIXELS and SSDK_LEVEL_LANES=0, at the golden cases' image sizes on the CPU device
(recording calls only host predicates of the library)."""
import collections
import contextlib
import ctypes
import hashlib
import os

import torch

Variant = collections.namedtuple("Variant", "case dtype env")

_FAMILIES = ("cases", "cases_effnet", "cases_shelf", "cases_yolo", "cases_darknet", "cases_densenet", "cases_shufflenet")
_BARE = {"cases_darknet": "test_darknet_cpu", "cases_densenet": "test_densenet_cpu", "cases_shufflenet": "test_shufflenet_cpu"}
_BUILD = {"cases_shelf": "test_shelf_cpu", "cases_yolo": "test_yolo_cpu", "cases_darknet": "test_darknet_cpu",
          "cases_densenet": "test_densenet_cpu", "cases_shufflenet": "test_shufflenet_cpu"}
FP16 = ("ssd_mnv2", "fpn_r18", "bifpn_regx008", "bifpn_effb0", "shelf_stub", "yolov4_stub", "dk53_bare", "dn121_bare", "sfv2x1_bare")
SWITCHES = (
    ({"SSDK_DKRES": "0"}, ("dk53_bare", "yolov3_dk53")),
    ({"SSDK_DKRES": "1"}, ("dk53_bare", "yolov4_dk53")),
    ({"SSDK_WFRAG": "0"}, ("ssd_mnv2", "fpn_stub", "dn121_bare", "yolov3_dk53")),
    # the golden cases are small images, every pyramid level below planner.SMALL_LEVEL_PIXELS: the bar lowered as
    # tests/test_gpu_nets.py lowers it, the levels split into big ones and small ones (lane 2) unless SSDK_LEVEL_LANES=0
    ({"SMALL_LEVEL_PIXELS": "200"}, ("fpn_r18", "fpn_stub")),
    ({"SMALL_LEVEL_PIXELS": "100"}, ("bifpn_stub",)),
    ({"SMALL_LEVEL_PIXELS": "200", "SSDK_LEVEL_LANES": "0"}, ("fpn_r18",)),
    ({"SMALL_LEVEL_PIXELS": "100", "SSDK_LEVEL_LANES": "0"}, ("bifpn_stub",)),
)


def all_cases():
    """{case name: cases module name} of every NET_CASES / BACKBONE_CASES entry, in the modules' order."""
    out = collections.OrderedDict()
    for fam in _FAMILIES:
        mod = __import__(fam)
        for name in list(mod.NET_CASES) + list(getattr(mod, "BACKBONE_CASES", ())):
            out[name] = fam
    return out


def _plans():
    out = collections.OrderedDict()
    for name in all_cases():
        out[name + "/bf16"] = Variant(name, torch.bfloat16, {})
    for name in FP16:
        out[name + "/fp16"] = Variant(name, torch.float16, {})
    for env, names in SWITCHES:
        for name in names:
            out["%s/bf16/%s" % (name, ",".join("%s=%s" % kv for kv in sorted(env.items())))] = Variant(name, torch.bfloat16, env)
    return out


PLANS = _plans()


class _Patch(object):
    """What the ``build(name, monkeypatch)`` helpers of the test files need of pytest's monkeypatch."""

    def __init__(self):
        self.saved = []

    def setattr(self, obj, name, value):
        self.saved.append((obj, name, getattr(obj, name)))
        setattr(obj, name, value)

    def undo(self):
        for obj, name, value in reversed(self.saved):
            setattr(obj, name, value)


def build_model(case):
    """(model in eval mode in fp32 on the CPU, image) of a case, through the helpers the CPU tests build it with."""
    fam = all_cases()[case]
    mod = __import__(fam)
    if case in getattr(mod, "BACKBONE_CASES", ()):
        return __import__(_BARE[fam]).build_bare(case)[:2]
    if fam == "cases_effnet":
        return __import__("mbseaudit").build_case(case)[:2]
    if fam == "cases":
        return __import__("nethelp").build(case)[:2]
    patch = _Patch()
    try:
        return __import__(_BUILD[fam]).build(case, patch)[:2]
    finally:
        patch.undo()


@contextlib.contextmanager
def switches(env):
    """No SSDK_* variable set but those of ``env``; SSDK_WFRAG, which fused_conv reads when it is imported, through the module
    global the functions read (as tests/test_gpu_conv.py sets it); SMALL_LEVEL_PIXELS is the planner's module attribute."""
    from ssds.modeling.layers import fused_conv as FC
    from ssds.modeling.layers import planner

    env = dict(env)
    pixels = planner.SMALL_LEVEL_PIXELS
    planner.SMALL_LEVEL_PIXELS = int(env.pop("SMALL_LEVEL_PIXELS", pixels))
    saved = {k: v for k, v in os.environ.items() if k.startswith("SSDK_")}
    wfrag = FC.USE_WFRAG
    for k in saved:
        del os.environ[k]
    os.environ.update(env)
    FC.USE_WFRAG = env.get("SSDK_WFRAG", "1") != "0"
    try:
        yield
    finally:
        for k in env:
            os.environ.pop(k, None)
        os.environ.update(saved)
        FC.USE_WFRAG = wfrag
        planner.SMALL_LEVEL_PIXELS = pixels


def record_plan(model, x, case):
    """The finalized plan of ``model`` (already in the plan's dtype) for the image ``x``, or the PlanUnsupported message."""
    from ssds.modeling.layers import fused_conv as FC
    from ssds.modeling.layers import planner

    fam = all_cases()[case]
    try:
        with torch.no_grad():
            if case in getattr(__import__(fam), "BACKBONE_CASES", ()):
                plan = FC.ConvPlan(x.device, x.dtype, x.shape)
                planner.record_backbone(plan, plan.input_value(), model)
                return plan.finalize()
            if type(model.backbone).__name__ == "StubBackbone":
                feats = [f.to(x.dtype) for f in model.backbone(x)]
                return planner.build_ssd_plan(model, x) if type(model).__name__ == "SSD" else model._build_neck_plan(feats)
            return planner.build_ssd_plan(model, x) if type(model).__name__ == "SSD" else model._build_neck_plan(None, image=x)
    except planner.PlanUnsupported as e:
        return str(e)


def _tensors(obj, path, out, seen):
    if obj is None or id(obj) in seen:
        return
    seen.add(id(obj))
    if isinstance(obj, torch.Tensor):
        out.append((path, obj))
    elif isinstance(obj, (list, tuple)):
        for i, v in enumerate(obj):
            _tensors(v, "%s[%d]" % (path, i), out, seen)
    elif isinstance(obj, dict):
        for k, v in obj.items():
            _tensors(v, "%s[%r]" % (path, k), out, seen)
    elif type(obj).__module__.startswith("ssds"):
        names = [n for klass in type(obj).__mro__ for n in getattr(klass, "__slots__", ())] + list(getattr(obj, "__dict__", ()))
        for name in names:
            if hasattr(obj, name):
                _tensors(getattr(obj, name), path + "." + name, out, seen)


def canonical(plan):
    """dict(ops=[(name, kind, repr(flops), repr(bytes), text)], patches, heads, bufs, pinned) of a finalized plan."""
    ranges = [(t.data_ptr(), t.numel(), "A%d" % i) for i, (t, _) in enumerate(plan.arena.bufs)]
    found, seen = [], set()
    _tensors(plan.keep, "K", found, seen)
    for i, L in enumerate(plan.layers):
        _tensors(L, "L%d" % i, found, seen)
    ranges += [(t.data_ptr(), max(t.numel() * t.element_size(), 1), path) for path, t in found]
    ranges.sort()

    def word(v):
        for base, size, name in ranges:
            if base <= v < base + size:
                return "%s+%d" % (name, v - base)
        return "%x" % v

    table = plan.layer_table()
    assert len(table) == len(plan.ops) == len(plan.layers)
    size = ctypes.sizeof(plan.ops[0]) if len(plan.ops) else 0
    assert size % 8 == 0, size
    ops = []
    for op, row in zip(plan.ops, table):
        raw = ctypes.string_at(ctypes.addressof(op), size)
        text = " ".join(word(int.from_bytes(raw[o:o + 8], "little")) for o in range(0, size, 8))
        ops.append((row["name"], row["kind"], repr(row["flops"]), repr(row["bytes"]), text))
    return dict(ops=ops, patches=[list(p) for p in plan.patches], heads=[list(h) for h in plan.heads],
                bufs=[int(t.numel()) for t, _ in plan.arena.bufs], pinned=sorted(plan.pinned))


def digest(canon):
    """``canonical``'s result with every op's text replaced by the first 12 hex digits of its SHA-1 (what the golden file stores)."""
    out = dict(canon)
    out["ops"] = [list(o[:4]) + [hashlib.sha1(o[4].encode()).hexdigest()[:12]] for o in canon["ops"]]
    return out


def record(key, models=None):
    """(canonical text of PLANS[key] | {"unsupported": message}, the plan | None).  ``models``: a dict that caches the built models
    per (case, dtype) across calls."""
    v = PLANS[key]
    models = {} if models is None else models
    if (v.case, v.dtype) not in models:
        model, x = build_model(v.case)
        models[(v.case, v.dtype)] = (model.to(v.dtype), x.to(v.dtype))
    model, x = models[(v.case, v.dtype)]
    with switches(v.env):
        first = record_plan(model, x, v.case)
        if isinstance(first, str):
            return {"unsupported": first}, None
        second = record_plan(model, x, v.case)  # (``first`` is alive: every buffer and pack of ``second`` lies elsewhere)
    a, b = canonical(first), canonical(second)
    assert a == b, "%s: two recordings in one process differ -- an address the walk does not resolve?\n%s" % (
        key, [(i, p[4], q[4]) for i, (p, q) in enumerate(zip(a["ops"], b["ops"])) if p != q][:1])
    return a, first
