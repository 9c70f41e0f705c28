"""The decisions of the five kernel-backed ``nn.Conv2d`` subclasses of the training step, pinned without a GPU: for every
combination of weight dtype, input dtype, autocast state, input layout and layer geometry, whether ``forward`` enters the HIP
kernels or ``nn.Conv2d.forward``, and with which input dtype and contiguity; and which modules the ``use_*`` swap functions
take.  The expected answers are data, tests/golden/kernel_conv_decisions.json, recorded from the code as it stood before the
layers were put on one base class; regenerate them (only when a decision is meant to change) with

    python tests/test_kernel_conv_cpu.py

The input is a stub that carries what a gate may look at (shape, dtype, device, contiguity) and raises from anything that would
touch memory, so "the kernels were entered" is the stub's exception leaving the autograd function."""
import contextlib
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "kernel_conv_decisions.json")
if __name__ == "__main__":
    for _p in (ROOT, os.path.join(ROOT, "ssds.pytorch_amd")):
        sys.path.insert(0, _p)

import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
NAMES = {v: k for k, v in DTYPES.items()}


class Touched(Exception):
    """The stub was asked for something only a tensor with memory behind it has."""

    def __init__(self, stub, what):
        Exception.__init__(self, what)
        self.stub = stub


class Stub(object):
    def __init__(self, shape, dtype, cuda=True, contiguous=True):
        self.shape, self.dtype, self.is_cuda, self._contiguous = tuple(shape), dtype, cuda, contiguous
        self.device = torch.device("cuda", 0) if cuda else torch.device("cpu")

    def dim(self):
        return len(self.shape)

    def is_contiguous(self):
        return self._contiguous

    def contiguous(self):
        return self if self._contiguous else Stub(self.shape, self.dtype, self.is_cuda, True)

    def to(self, dtype):
        return self if dtype == self.dtype else Stub(self.shape, dtype, self.is_cuda, self._contiguous)

    def __getattr__(self, name):
        raise Touched(self, name)

    def describe(self):
        return "{} {}".format(NAMES[self.dtype], "contiguous" if self._contiguous else "strided")


# class -> (module, class name, constructor arguments of the layer the kernels take, geometry variants as overrides).  The first
# variants of a class stay inside its geometry; the others leave it one property at a time
LAYERS = {
    "NativeConv3x3": ("pointwise", dict(in_channels=16, out_channels=8, kernel_size=3, stride=1, padding=1), {
        "base": {}, "stride2": dict(stride=2), "no_bias": dict(bias=False), "stride3": dict(stride=3), "pad0": dict(padding=0),
        "dilation2": dict(dilation=2), "reflect": dict(padding_mode="reflect"), "groups2": dict(groups=2), "kernel5": dict(kernel_size=5)}),
    "StemConv3x3s2": ("pointwise", dict(in_channels=3, out_channels=32, kernel_size=3, stride=2, padding=1, bias=False), {
        "base": {}, "cin1": dict(in_channels=1), "bias": dict(bias=True), "stride1": dict(stride=1), "stride3": dict(stride=3),
        "dilation2": dict(dilation=2), "reflect": dict(padding_mode="reflect"), "cin4": dict(in_channels=4),
        "cout64": dict(out_channels=64), "pad0": dict(padding=0)}),
    "StemConv7x7s2": ("stemconv", dict(in_channels=3, out_channels=64, kernel_size=7, stride=2, padding=3, bias=False), {
        "base": {}, "cout32": dict(out_channels=32), "bias": dict(bias=True), "stride1": dict(stride=1), "stride3": dict(stride=3),
        "dilation2": dict(dilation=2), "reflect": dict(padding_mode="reflect"), "cin4": dict(in_channels=4),
        "cout128": dict(out_channels=128), "pad2": dict(padding=2)}),
    "GroupedConv3x3": ("groupedconv", dict(in_channels=16, out_channels=16, kernel_size=3, stride=1, padding=1, groups=2), {
        "base": {}, "stride2": dict(stride=2), "merged4": dict(in_channels=8, out_channels=8), "bias_off": dict(bias=False),
        "stride3": dict(stride=3), "dilation2": dict(dilation=2), "reflect": dict(padding_mode="reflect"),
        "width12": dict(in_channels=24, out_channels=24), "width4_odd": dict(in_channels=12, out_channels=12, groups=3),
        "depthwise": dict(groups=16), "dense": dict(groups=1), "cout32": dict(out_channels=32), "pad0": dict(padding=0)}),
    "DenseConv3x3": ("denseconv", dict(in_channels=16, out_channels=4, kernel_size=3, stride=1, padding=1), {
        "base": {}, "stride2": dict(stride=2), "no_bias": dict(bias=False), "stride3": dict(stride=3),
        "dilation2": dict(dilation=2), "reflect": dict(padding_mode="reflect"), "cin8": dict(in_channels=8),
        "cin24": dict(in_channels=24), "cout6": dict(out_channels=6), "cout2": dict(out_channels=2),
        "groups2": dict(groups=2), "pad0": dict(padding=0)}),
}
# what the input may be besides a contiguous 4-D HIP tensor of the layer's width; the variants that leave the geometry see "good" only
INPUTS = ("good", "strided", "cpu", "3d", "channels")
INSIDE = ("base", "stride2", "no_bias", "cin1", "cout32", "merged4", "bias_off")
ENVIRONMENT = {"NativeConv3x3": ("SSDK_CONV3_NATIVE", "0")}


def _stats():
    from ssds.modeling.layers import denseconv, groupedconv, stemconv

    return {"stem7": stemconv.STATS, "gconv": groupedconv.STATS, "dense3": denseconv.STATS}


def _stub(kind, cin, dtype):
    shape = (2, cin + 1, 8, 8) if kind == "channels" else (cin, 8, 8) if kind == "3d" else (2, cin, 8, 8)
    return Stub(shape, dtype, cuda=kind != "cpu", contiguous=kind != "strided")


@contextlib.contextmanager
def _patched(autocast_dtype, entered, env=None):
    class FakeAutocast(object):
        def __init__(self, device_type, dtype=None, enabled=True):
            entered.append((device_type, enabled))

        def __enter__(self):
            return self

        def __exit__(self, *exc):
            return False

    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(nn.Conv2d, "forward", lambda self, x: ("conv2d", x))
        mp.setattr(torch, "is_autocast_enabled", lambda *a: autocast_dtype is not None)
        mp.setattr(torch, "get_autocast_dtype", lambda device_type: autocast_dtype)
        mp.setattr(torch, "autocast", FakeAutocast)
        mp.delenv("SSDK_CONV3_NATIVE", raising=False)
        if env is not None:
            mp.setenv(*env)
        yield


def decide(layer, x, autocast_dtype, env=None):
    """-> "kernels <dtype> <layout>" or "conv2d <dtype> <layout>" (what reached either), plus the STATS counters that moved."""
    entered = []
    stats = _stats()
    before = {k: dict(v) for k, v in stats.items()}
    with _patched(autocast_dtype, entered, env):
        try:
            tag, seen = layer(x)
            assert tag == "conv2d", tag
            assert entered == [], "nn.Conv2d.forward is reached outside any autocast block of the layer's"
            out = "conv2d " + seen.describe()
        except Touched as t:
            assert entered == [("cuda", False)], "the kernels run with autocast switched off, once: {}".format(entered)
            out = "kernels " + t.stub.describe()
    moved = ["{}.{}{:+d}".format(k, n, v[n] - before[k][n]) for k, v in sorted(stats.items()) for n in sorted(v) if v[n] != before[k][n]]
    return " ".join([out] + moved)


def sweep_class(name):
    import importlib

    modname, base, variants = LAYERS[name]
    cls = getattr(importlib.import_module("ssds.modeling.layers." + modname), name)
    table = {}
    for vname, override in sorted(variants.items()):
        kwargs = dict(base, **override)
        for wname, wdt in DTYPES.items():
            layer = cls(**kwargs).to(wdt)
            for xname, xdt in DTYPES.items():
                for aname, adt in (("off", None), ("bf16", torch.bfloat16), ("fp16", torch.float16)):
                    for kind in (INPUTS if vname in INSIDE else INPUTS[:1]):
                        key = "{} w={} x={} autocast={} {}".format(vname, wname, xname, aname, kind)
                        table[key] = decide(layer, _stub(kind, kwargs["in_channels"], xdt), adt)
                        if name in ENVIRONMENT and vname == "base" and kind in ("good", "strided"):
                            env = ENVIRONMENT[name]
                            table[key + " {}={}".format(*env)] = decide(layer, _stub(kind, kwargs["in_channels"], xdt), adt, env)
    return table


# ---- the swap functions on synthetic modules -------------------------------------------------------------------------------------
def _conv(cin, cout, k, s=1, p=0, **kw):
    return dict(in_channels=cin, out_channels=cout, kernel_size=k, stride=s, padding=p, **kw)


SWAP_LAYERS = [
    _conv(16, 16, 1), _conv(16, 8, 1, bias=False), _conv(16, 16, 1, s=2), _conv(16, 16, 1, p=1), _conv(16, 16, 1, groups=2),
    _conv(16, 16, 1, dilation=2), _conv(16, 16, 1, padding_mode="reflect"), _conv(12, 20, 1),
    _conv(16, 8, 3, 1, 1), _conv(16, 8, 3, 2, 1), _conv(16, 8, 3, 3, 1), _conv(16, 8, 3, 1, 0), _conv(16, 8, 3, 1, 2, dilation=2),
    _conv(16, 8, 3, 1, 1, dilation=2), _conv(16, 8, 3, 1, 1, padding_mode="reflect"), _conv(16, 8, 3, 1, 1, bias=False),
    _conv(16, 8, 3, (1, 2), 1), _conv(8, 8, 3, 1, 1), _conv(24, 24, 3, 1, 1), _conv(16, 6, 3, 1, 1), _conv(16, 2, 3, 1, 1),
    _conv(32, 4, 3, 2, 1), _conv(5, 8, 3, 1, 1),
    _conv(16, 16, 3, 1, 1, groups=2), _conv(16, 16, 3, 2, 1, groups=2), _conv(8, 8, 3, 1, 1, groups=2), _conv(12, 12, 3, 1, 1, groups=3),
    _conv(24, 24, 3, 1, 1, groups=2), _conv(16, 32, 3, 1, 1, groups=2), _conv(16, 16, 3, 1, 1, groups=16, bias=False),
    _conv(16, 16, 3, 3, 1, groups=2), _conv(16, 16, 3, 1, 1, groups=2, padding_mode="reflect"), _conv(16, 16, 3, 1, 1, groups=2, dilation=2),
    _conv(3, 32, 3, 2, 1, bias=False), _conv(3, 32, 3, 2, 1), _conv(1, 16, 3, 2, 1, bias=False), _conv(3, 64, 3, 2, 1, bias=False),
    _conv(4, 32, 3, 2, 1, bias=False), _conv(3, 32, 3, 1, 1, bias=False), _conv(3, 32, 3, 2, 1, bias=False, padding_mode="reflect"),
    _conv(3, 32, 3, 2, 0, bias=False), _conv(3, 32, 3, 2, 1, bias=False, dilation=2),
    _conv(3, 64, 7, 2, 3, bias=False), _conv(3, 64, 7, 2, 3), _conv(1, 32, 7, 2, 3, bias=False), _conv(3, 128, 7, 2, 3, bias=False),
    _conv(4, 64, 7, 2, 3, bias=False), _conv(3, 64, 7, 1, 3, bias=False), _conv(3, 64, 7, 2, 2, bias=False),
    _conv(3, 64, 7, 2, 3, bias=False, padding_mode="reflect"), _conv(3, 64, 7, 2, 3, bias=False, dilation=2),
    _conv(16, 16, 5, 1, 2),
]
# (subclasses of nn.Conv2d are nobody's to take: the kernel-backed classes of other families, and a user's own)
SWAP_SUBCLASSES = [_conv(16, 16, 1), _conv(16, 8, 3, 1, 1), _conv(16, 16, 3, 1, 1, groups=2), _conv(3, 32, 3, 2, 1, bias=False),
                   _conv(3, 64, 7, 2, 3, bias=False), _conv(16, 16, 3, 1, 1, groups=16, bias=False)]
SWAPS = [("pointwise", "use_pointwise_gemm", {}), ("pointwise", "use_native_conv3x3", {}),
         ("pointwise", "use_native_conv3x3", dict(min_in_channels=16)), ("pointwise", "use_native_conv3x3", dict(min_in_channels=17)),
         ("pointwise", "use_native_stem", {}), ("stemconv", "use_native_stem7", {}), ("groupedconv", "use_native_gconv", {}),
         ("denseconv", "use_native_dense3x3", {})]


class OwnConv(nn.Conv2d):
    pass


def _swap_model():
    from ssds.modeling.layers.dwconv import DepthwiseConv2d

    plain = [nn.Conv2d(**kw) for kw in SWAP_LAYERS]
    own = [OwnConv(**kw) for kw in SWAP_SUBCLASSES] + [DepthwiseConv2d(16, 16, 3, 1, 1, groups=16, bias=False)]
    # nested containers, and a non-convolution in between: the walk is over model.modules()
    return nn.Sequential(nn.Sequential(*plain[:10]), nn.ModuleList(plain[10:]), nn.ReLU(), nn.ModuleDict({"own": nn.Sequential(*own)}))


def _layer_name(m):
    extra = "".join(", {}={}".format(k, getattr(m, k)) for k, d in (("dilation", (1, 1)), ("groups", 1), ("padding_mode", "zeros"))
                    if getattr(m, k) != d)
    return "{}->{} k{} s{} p{}{}{}".format(m.in_channels, m.out_channels, m.kernel_size[0], m.stride if m.stride[0] != m.stride[1] else m.stride[0],
                                          m.padding[0], "" if m.bias is not None else " no bias", extra)


def sweep_swaps():
    import importlib

    table = {}
    for modname, fname, kwargs in SWAPS:
        mod = importlib.import_module("ssds.modeling.layers." + modname)
        model = _swap_model()
        convs = [m for m in model.modules() if isinstance(m, nn.Conv2d)]
        was = [type(m).__name__ for m in convs]
        keys = list(model.state_dict().keys())
        stats = {k: v["swapped"] for k, v in _stats().items()}
        ret = getattr(mod, fname)(model, **kwargs)
        again = getattr(mod, fname)(model, **kwargs)
        assert list(model.state_dict().keys()) == keys
        table[fname + "".join(" {}={}".format(*kv) for kv in sorted(kwargs.items()))] = {
            "returns": "model" if ret is model else ret,
            "returns_again": "model" if again is model else again,
            "swapped": {k: v["swapped"] - stats[k] for k, v in sorted(_stats().items()) if v["swapped"] != stats[k]},
            "taken": ["{}: {} -> {}".format(_layer_name(m), a, type(m).__name__) for m, a in zip(convs, was) if type(m).__name__ != a],
            "layers": len(convs),
        }
    return table


def sweep():
    out = {name: sweep_class(name) for name in sorted(LAYERS)}
    out["swaps"] = sweep_swaps()
    return out


def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


def _differences(got, want):
    keys = sorted(set(got) | set(want))
    return ["{}: {} (recorded: {})".format(k, got.get(k), want.get(k)) for k in keys if got.get(k) != want.get(k)]


@pytest.mark.parametrize("name", sorted(LAYERS))
def test_forward_decisions_are_the_recorded_ones(name):
    got, want = sweep_class(name), _golden()[name]
    diff = _differences(got, want)
    assert not diff, "{} of {} decisions changed:\n{}".format(len(diff), len(want), "\n".join(diff[:40]))
    # the table is worth something only if both answers occur, with both layouts where the class copies a strided input
    assert any(v.startswith("kernels") for v in want.values()) and any(v.startswith("conv2d") for v in want.values())


def test_swap_functions_take_the_recorded_layers():
    got, want = sweep_swaps(), _golden()["swaps"]
    assert sorted(got) == sorted(want)
    for fname in sorted(want):
        assert got[fname] == want[fname], fname
        assert want[fname]["taken"], fname + ": the synthetic model has nothing for it"
        # no subclass of nn.Conv2d is ever taken (type(m) is nn.Conv2d)
        assert all(": Conv2d -> " in line for line in want[fname]["taken"]), fname


def test_the_stub_raises_from_whatever_touches_memory():
    x = Stub((2, 3, 8, 8), torch.bfloat16, contiguous=False)
    assert x.dim() == 4 and not x.is_contiguous() and x.contiguous().is_contiguous() and x.to(torch.bfloat16) is x
    assert x.to(torch.float16).dtype == torch.float16 and not x.to(torch.float16).is_contiguous()
    for touch in (lambda: x.data_ptr(), lambda: x.detach(), lambda: x.float(), lambda: x.view(2, -1)):
        with pytest.raises(Touched):
            touch()


if __name__ == "__main__":
    with open(GOLDEN, "w") as f:
        json.dump(sweep(), f, indent=0, sort_keys=True)
        f.write("\n")
    print("wrote", GOLDEN)
