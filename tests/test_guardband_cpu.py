"""tests/guardband.py can fail: on CPU tensors, with torch expressions standing in for a kernel, every helper flags the
dishonest stand-in and passes the honest one.  (If a stand-in here were made honest, or an honest one dishonest, its test fails.)"""
import pytest
import torch

import guardband as G

DTYPES = [torch.bfloat16, torch.float16, torch.float32]


def _typed(storage, dtype):
    """The whole allocation as a flat tensor of ``dtype`` -- what a kernel's raw pointer can reach."""
    return storage.view(dtype)


def _flat_index(storage, view):
    return (view.data_ptr() - storage.data_ptr()) // view.element_size()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("channels_last", [False, True])
def test_guarded_view_keeps_shape_strides_and_bits(dtype, channels_last):
    t = torch.randn(3, 8, 5, 7).to(dtype)
    t[1, 2, 3, 4] = float("nan")
    t[0, 0, 0, 0] = -0.0
    if channels_last:
        t = t.contiguous(memory_format=torch.channels_last)
    storage, view = G.guarded(t)
    assert view.shape == t.shape and view.stride() == t.stride() and view.dtype == t.dtype
    assert view.is_contiguous(memory_format=torch.channels_last if channels_last else torch.contiguous_format)
    assert G.same_bits(view, t) and G.guards_intact(storage, view)
    es = t.element_size()
    lo = view.data_ptr() - storage.data_ptr()
    assert lo % 256 == 0 and lo >= (4096 + 8 * 5 * 7) * es and storage.numel() == 2 * lo + t.numel() * es
    typed = _typed(storage, dtype)
    i = _flat_index(storage, view)
    assert torch.isnan(typed[:i]).all() and torch.isnan(typed[i + t.numel():]).all(), "0xFF bytes are NaN in every float type"


def test_guards_of_packed_u16_and_fp32_vectors():
    img = torch.arange(3 * 5 * 4, dtype=torch.int16).view(3, 5, 4)
    storage, view = G.guarded(img)
    assert torch.equal(view, img) and G.guards_intact(storage, view) and int(_typed(storage, torch.int16)[0]) == -1
    bias = torch.randn(40)
    storage, view = G.guarded(bias)
    assert G.same_bits(view, bias) and view.data_ptr() - storage.data_ptr() >= 4 * (4096 + 1)


@pytest.mark.parametrize("dtype", DTYPES)
def test_infinity_guards(dtype):
    t = torch.rand(2, 6, 3, 3).to(dtype)
    storage, view = G.guarded(t, fill=G.INF_FILL[dtype])
    typed = _typed(storage, dtype)
    i = _flat_index(storage, view)
    assert bool((typed[:i] == float("inf")).all()) and bool((typed[i + t.numel():] == float("inf")).all())
    assert G.guards_intact(storage, view, G.INF_FILL[dtype]) and not G.guards_intact(storage, view)
    typed[i - 1] = 1.0
    assert not G.guards_intact(storage, view, G.INF_FILL[dtype])


@pytest.mark.parametrize("where", ["before", "after", "honest"])
def test_a_write_next_to_the_view_is_flagged(where):
    storage, y = G.guarded_like((2, 8, 3, 5), torch.bfloat16, torch.channels_last)
    typed = _typed(storage, torch.bfloat16)
    i = _flat_index(storage, y)

    def kernel():  # writes every element of y -- and, when dishonest, one element before / after it
        y.copy_(torch.ones(y.shape, dtype=y.dtype))
        if where == "before":
            typed[i - 1] = 1.0
        elif where == "after":
            typed[i + y.numel()] = 1.0

    assert G.guards_intact(storage, y)
    kernel()
    assert not G.has_nan(y)
    assert G.guards_intact(storage, y) == (where == "honest")


@pytest.mark.parametrize("honest", [True, False])
def test_an_unwritten_output_element_is_flagged(honest):
    storage, y = G.guarded_like((2, 3, 4, 4), torch.float16)
    assert G.has_nan(y) and bool(torch.isnan(y).all()), "the interior of an output starts as NaN"
    y.copy_(torch.ones(y.shape, dtype=y.dtype))
    if not honest:  # the "kernel" skipped the last element of the last row of image 0
        y[0, 2, 3, 3] = float("nan")
    assert G.has_nan(y) == (not honest)
    assert G.guards_intact(storage, y)


@pytest.mark.parametrize("honest", [True, False])
def test_a_read_past_the_input_times_zero_is_flagged(honest):
    n = 24
    x = torch.randn(n).to(torch.bfloat16)
    storage, xv = G.guarded(x)
    i = _flat_index(storage, xv)
    x_ext = _typed(storage, torch.bfloat16)[i:i + n + 1]  # the input and the one element behind it

    def kernel(src):
        if honest:
            return src[..., :n] + 0 * src[..., :n]
        return src[..., :n] + 0 * src[..., 1:n + 1]  # reads one element past its input and multiplies it by zero

    clean = kernel(torch.cat([x, torch.zeros(1, dtype=x.dtype)]))  # ordinary allocation: the stray read meets a finite value
    got = kernel(x_ext)
    assert not G.has_nan(clean), "on an ordinary allocation the stray read is invisible"
    assert G.has_nan(got) == (not honest)
    assert G.same_bits(got, clean) == honest


@pytest.mark.parametrize("honest", [True, False])
def test_a_modified_source_is_flagged(honest):
    gs = G.GuardSet()
    x = gs.inp("x", torch.randn(2, 8, 3, 3).to(torch.float16).contiguous(memory_format=torch.channels_last))
    y = gs.out("y", (2, 8, 3, 3), torch.float16, torch.channels_last)
    gs.arm()
    y.copy_(x * 2)
    if not honest:
        x[1, 7, 2, 2] = 0.0  # an "in-place" kernel
    bad = gs.problems()
    assert (bad == []) == honest
    assert honest or bad == ["the input x was written"]


def test_guardset_names_the_buffer_whose_guard_changed():
    gs = G.GuardSet()
    gs.inp("x", torch.zeros(4, 4))
    y = gs.out("y", (4, 4), torch.float32)
    ws = gs.zeros("ws", 512)
    gs.arm()
    assert gs.problems() == [] and int(ws.sum()) == 0 and ws.numel() == 512
    storage = gs.items[1][1]
    storage[storage.numel() - 1] = 0
    y.zero_()
    assert gs.problems() == ["a guard of y was written"]


def test_same_bits_is_not_float_equality():
    nan = torch.tensor([float("nan"), 1.0])
    assert G.same_bits(nan, nan.clone()) and not torch.equal(nan, nan.clone())
    assert not G.same_bits(torch.tensor([0.0]), torch.tensor([-0.0])) and torch.equal(torch.tensor([0.0]), torch.tensor([-0.0]))
    assert not G.same_bits(torch.zeros(2), torch.zeros(2, dtype=torch.float16))
    assert not G.same_bits(torch.zeros(2), torch.zeros(3))


def test_non_dense_tensors_are_refused():
    with pytest.raises(AssertionError):
        G.guarded(torch.zeros(4, 8)[:, ::2])


def test_guard_pack_relocates_every_tensor_and_reinstalls_the_images():
    """On the CPU the packs build without the library's kernels; the fragment images need ssdk_*_bytes from the library, so
    this case needs the built package (as every test of the suite does), not a GPU."""
    import torch.nn as nn
    from ssds.modeling.layers import fused_conv as FC

    torch.manual_seed(0)
    conv, bn = nn.Conv2d(64, 40, 3, 1, 1, bias=False), nn.BatchNorm2d(40)
    pack = FC.ConvPack(conv, bn, "relu", torch.bfloat16)
    old = {f: getattr(pack, f).clone() for f in ("w", "scale", "bias")}
    old_img = pack.frag().clone()
    moved = G.guard_pack(pack)
    assert [m[0] for m in moved] == ["w", "scale", "bias", "w_frag"]
    for name, storage, view in moved:
        assert G.guards_intact(storage, view)
        want = old_img if name == "w_frag" else old[name]
        assert G.same_bits(view, want) and view.stride() == want.stride()
    assert pack.w.data_ptr() == moved[0][2].data_ptr() and pack.frag().data_ptr() == moved[3][2].data_ptr()
    assert moved[3][2].shape == (3, 18, 4, 16, 8), "rows padded to 16: the padding belongs to the image"
    stem = FC.StemPack(nn.Conv2d(3, 64, 7, 2, 3, bias=False), nn.BatchNorm2d(64), "relu", torch.float16)
    assert [m[0] for m in G.guard_pack(stem)] == ["w", "scale", "bias"] and stem.w.shape == (64, 7, 8, 4)
