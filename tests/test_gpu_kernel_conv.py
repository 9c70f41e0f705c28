"""The five kernel-backed ``nn.Conv2d`` classes on their shared base (ssds/modeling/layers/kernel_conv.py) on the GPU: a swapped
module under autocast computes exactly what its family's autograd function computes on the cast input, counts exactly the
launches it makes, hands every input its gate refuses to ``nn.Conv2d.forward``, and (the stems) copies a strided input.

No tolerances: the kernels are bit-reproducible and both sides of every comparison run the same kernels on the same operands, so
every comparison is ``torch.equal``.  The shapes are the smallest that reach each branch of the Python side."""
import pytest

pytestmark = pytest.mark.gpu

# id -> (class, nn.Conv2d arguments, (N, H, W))
CASES = {
    "dense-s1-bias": ("DenseConv3x3", dict(in_channels=16, out_channels=4, kernel_size=3, stride=1, padding=1), (2, 5, 6)),
    "dense-s2-bias": ("DenseConv3x3", dict(in_channels=16, out_channels=4, kernel_size=3, stride=2, padding=1), (2, 5, 6)),
    "dense-s1": ("DenseConv3x3", dict(in_channels=16, out_channels=4, kernel_size=3, stride=1, padding=1, bias=False), (2, 5, 6)),
    "dense-s2": ("DenseConv3x3", dict(in_channels=16, out_channels=4, kernel_size=3, stride=2, padding=1, bias=False), (2, 5, 6)),
    "grouped-16-s1-bias": ("GroupedConv3x3", dict(in_channels=16, out_channels=16, kernel_size=3, stride=1, padding=1, groups=2), (2, 5, 6)),
    "grouped-16-s2": ("GroupedConv3x3", dict(in_channels=16, out_channels=16, kernel_size=3, stride=2, padding=1, groups=2, bias=False), (2, 5, 6)),
    "grouped-8-s1": ("GroupedConv3x3", dict(in_channels=8, out_channels=8, kernel_size=3, stride=1, padding=1, groups=2, bias=False), (2, 5, 6)),
    "grouped-8-s2-bias": ("GroupedConv3x3", dict(in_channels=8, out_channels=8, kernel_size=3, stride=2, padding=1, groups=2), (2, 5, 6)),
    "im2col-folded": ("NativeConv3x3", dict(in_channels=16, out_channels=8, kernel_size=3, stride=1, padding=1), (2, 4, 6)),
    "im2col-unfolded": ("NativeConv3x3", dict(in_channels=16, out_channels=8, kernel_size=3, stride=1, padding=1), (1, 12, 12)),
    "im2col-cout4": ("NativeConv3x3", dict(in_channels=16, out_channels=4, kernel_size=3, stride=1, padding=1, bias=False), (2, 4, 6)),
    "stem3-kernel-wgrad": ("StemConv3x3s2", dict(in_channels=3, out_channels=32, kernel_size=3, stride=2, padding=1, bias=False), (2, 10, 16)),
    "stem3-library-wgrad": ("StemConv3x3s2", dict(in_channels=3, out_channels=32, kernel_size=3, stride=2, padding=1, bias=False), (2, 10, 18)),
    "stem7": ("StemConv7x7s2", dict(in_channels=3, out_channels=64, kernel_size=7, stride=2, padding=3, bias=False), (2, 20, 20)),
}
STEMS = ("StemConv3x3s2", "StemConv7x7s2")
DTYPES = ("bfloat16", "float16")


def _family(cls_name):
    """-> (class, swap(model), direct(x, w, bias, module) on the cast input, STATS or None,
    {counter: launches of one forward + backward with every gradient asked for})"""
    from ssds.modeling.layers import denseconv, groupedconv, pointwise, stemconv

    full = {"native_forward": 1, "native_dgrad": 1, "native_wgrad": 1}
    return {
        "DenseConv3x3": (denseconv.DenseConv3x3, denseconv.use_native_dense3x3,
                         lambda x, w, b, m: denseconv.dense_conv3x3(x, w, b, m.stride[0]), denseconv.STATS, full),
        "GroupedConv3x3": (groupedconv.GroupedConv3x3, groupedconv.use_native_gconv,
                           lambda x, w, b, m: groupedconv.grouped_conv3x3(x, w, b, m.stride[0], m.groups), groupedconv.STATS, full),
        "NativeConv3x3": (pointwise.NativeConv3x3, pointwise.use_native_conv3x3,
                          lambda x, w, b, m: pointwise._Conv3x3Native.apply(x, w, b, m.stride[0]), None, {}),
        "StemConv3x3s2": (pointwise.StemConv3x3s2, pointwise.use_native_stem,
                          lambda x, w, b, m: stemconv._StemConv.apply(x, w, stemconv._STEM3), None, {}),
        "StemConv7x7s2": (stemconv.StemConv7x7s2, stemconv.use_native_stem7,
                          lambda x, w, b, m: stemconv.stem_conv7x7s2(x, w), stemconv.STATS, {"native_forward": 1, "native_wgrad": 1}),
    }[cls_name]


def _layer(case, seed=0):
    """The case's plain ``nn.Conv2d`` with fp32 master weights on the GPU, switched by its family's swap function; an fp32 input."""
    import torch
    import torch.nn as nn

    cls_name, kwargs, (n, h, w) = CASES[case]
    cls, swap = _family(cls_name)[:2]
    torch.manual_seed(1000 + seed + sorted(CASES).index(case))
    model = nn.Sequential(nn.Conv2d(**kwargs)).cuda()
    swap(model)
    assert type(model[0]) is cls, type(model[0])
    return model[0], torch.randn(n, kwargs["in_channels"], h, w, device="cuda")


def _counters(stats):
    return {} if stats is None else {k: v for k, v in stats.items() if k != "swapped"}


def _moved(stats, before):
    return {k: v - before[k] for k, v in _counters(stats).items() if v != before[k]}


def _grads(layer, x):
    out = (x.grad, layer.weight.grad, None if layer.bias is None else layer.bias.grad)
    x.grad = layer.weight.grad = None
    if layer.bias is not None:
        layer.bias.grad = None
    return out


@pytest.mark.parametrize("dtype_name", DTYPES)
@pytest.mark.parametrize("case", sorted(CASES))
def test_module_under_autocast_is_the_family_function_on_the_cast_input(case, dtype_name):
    import torch

    dt = getattr(torch, dtype_name)
    layer, x = _layer(case)
    _, _, direct, stats, launches = _family(CASES[case][0])
    x.requires_grad_(True)
    before = _counters(stats)
    with torch.autocast("cuda", dt):
        y = layer(x)
    assert y.dtype == dt
    dy = torch.randn(y.shape, device="cuda").to(dt)
    y.backward(dy)
    assert _moved(stats, before) == launches
    dx, dw, db = _grads(layer, x)

    xc = x.detach().to(dt).requires_grad_(True)
    before = _counters(stats)
    want = direct(xc, layer.weight, layer.bias, layer)
    want.backward(dy)
    assert _moved(stats, before) == launches
    want_dx, want_dw, want_db = _grads(layer, xc)

    assert torch.equal(y, want)
    assert dx.dtype == torch.float32 and torch.equal(dx, want_dx.float())  # (autocast's cast hands the 16-bit gradient on in fp32)
    assert dw.dtype == torch.float32 and dw.shape == layer.weight.shape and torch.equal(dw, want_dw)
    assert (db is None) == (layer.bias is None)
    if db is not None:
        assert db.dtype == torch.float32 and torch.equal(db, want_db)
    assert bool(dw.abs().sum() > 0) and bool(dx.abs().sum() > 0)


@pytest.mark.parametrize("case", sorted(CASES))
def test_fp32_input_without_autocast_is_conv2d_forward(case):
    import torch
    import torch.nn as nn

    layer, x = _layer(case, seed=1)
    stats = _family(CASES[case][0])[3]
    before = _counters(stats)
    with torch.no_grad():
        y = layer(x)
        moved = _moved(stats, before)
        want = nn.Conv2d.forward(layer, x)
    assert y.dtype == torch.float32 and torch.equal(y, want)
    assert moved == ({"fallback": 1} if CASES[case][0] == "StemConv7x7s2" else {})


@pytest.mark.parametrize("case", [c for c in sorted(CASES) if CASES[c][0] not in STEMS])
def test_channels_last_input_is_conv2d_forward(case):
    import torch
    import torch.nn as nn

    layer, x = _layer(case, seed=2)
    x = x.contiguous(memory_format=torch.channels_last)
    assert not x.is_contiguous()
    stats = _family(CASES[case][0])[3]
    before = _counters(stats)
    with torch.no_grad(), torch.autocast("cuda", torch.bfloat16):
        y = layer(x)
        moved = _moved(stats, before)
        want = nn.Conv2d.forward(layer, x)
    assert y.dtype == torch.bfloat16 and torch.equal(y, want)
    assert moved == {}


@pytest.mark.parametrize("case", [c for c in sorted(CASES) if CASES[c][0] in STEMS])
def test_strided_input_into_a_stem_is_the_contiguous_call(case):
    import torch

    layer, x = _layer(case, seed=3)
    strided = x.permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2)  # the same values, the two image axes swapped in memory
    assert not strided.is_contiguous() and torch.equal(strided, x)
    stats, launches = _family(CASES[case][0])[3:]
    got = []
    for inp in (x, strided):
        before = _counters(stats)
        with torch.autocast("cuda", torch.bfloat16):
            y = layer(inp)
        dy = torch.ones_like(y)
        y.backward(dy)
        assert _moved(stats, before) == launches
        got.append((y, _grads(layer, inp)[1]))
    assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1])
    assert got[0][1].dtype == torch.float32
