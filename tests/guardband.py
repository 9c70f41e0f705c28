"""Guard bands: one procedure for "a kernel touches only the buffers it is handed" (include/ssdk.h: the caller owns every buffer,
kernels fully write their outputs).  Plain torch, importable and usable on the CPU (tests/test_guardband_cpu.py shows each
helper failing on a dishonest stand-in); tests/test_gpu_guard.py applies it to the inference kernels, the plan executor and the
decode stage.

A guarded tensor is a view in the middle of ONE larger allocation whose every other BYTE is a fill pattern.  The default fill,
0xFF, is a NaN in bf16, fp16 and fp32 alike (and 0xFFFF in a packed u16 image), so
  * a guard element that reaches arithmetic -- multiplied by a zero weight, added into a padded tap -- turns the result into NaN;
  * an output element the kernel never wrote still holds the NaN ``guarded_like`` put there;
  * a write outside the view changes a guard byte (``guards_intact``);
  * a write into an input changes its bits against a snapshot (``GuardSet``).
What the method cannot see: a stray READ whose value is then discarded by a select (``cond ? v : 0``), which changes no result,
and a stray access further away than the guard (4096 elements plus one image of the tensor on each side).

``fill`` is a byte (int) or a little-endian byte pattern of the element size (``INF_FILL``: +Inf guards for the score tensors of
the decode stage, where a NaN would never pass ``>= threshold`` but an Inf would surface as the top candidate)."""
import torch

GUARD_ELEMS = 4096
INF_FILL = {torch.bfloat16: bytes([0x80, 0x7F]), torch.float16: bytes([0x00, 0x7C]),
            torch.float32: bytes([0x00, 0x00, 0x80, 0x7F])}
_INT_VIEW = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def _pattern(fill, nbytes, device):
    """``nbytes`` bytes of the fill on ``device`` (uint8)."""
    if isinstance(fill, int):
        return torch.full((nbytes,), fill, dtype=torch.uint8, device=device)
    pat = torch.tensor(list(fill), dtype=torch.uint8, device=device)
    assert nbytes % pat.numel() == 0, (nbytes, pat.numel())
    return pat.repeat(nbytes // pat.numel())


def guard_bytes(shape, dtype):
    """Bytes of one guard: at least GUARD_ELEMS elements plus one image (``shape[1:]``) of the tensor, rounded up to 256 bytes so
    that the view keeps the 256-byte alignment of a torch allocation."""
    es = torch.empty((), dtype=dtype).element_size()
    image = 1
    for v in tuple(shape)[1:]:
        image *= int(v)
    return ((GUARD_ELEMS + image) * es + 255) // 256 * 256


def _is_dense(t):
    """Strides are a permutation of a contiguous layout: the elements fill ``numel`` consecutive slots, none twice."""
    expect = 1
    for size, stride in sorted(((s, st) for s, st in zip(t.shape, t.stride()) if s != 1), key=lambda p: p[1]):
        if stride != expect:
            return False
        expect *= size
    return True


def _carve(shape, strides, dtype, device, fill, interior_fill):
    es = torch.empty((), dtype=dtype).element_size()
    numel = 1
    for v in shape:
        numel *= int(v)
    g, body = guard_bytes(shape, dtype), numel * es
    storage = torch.cat([_pattern(fill, g, device), _pattern(interior_fill, body, device) if body else
                         torch.empty(0, dtype=torch.uint8, device=device), _pattern(fill, g, device)])
    view = storage[g:g + body].view(dtype).as_strided(tuple(shape), tuple(strides))
    assert view.data_ptr() == storage.data_ptr() + g and g % 256 == 0  # (a device allocation itself is 256-byte aligned)
    return storage, view


def guarded(t, fill=0xFF):
    """-> (storage, view): ``view`` has ``t``'s shape, dtype, strides (channels_last included), device and bits; it sits in the
    middle of ``storage`` (uint8), whose every other byte is ``fill``."""
    assert _is_dense(t), "guarded() takes dense tensors (contiguous in some dimension order): strides %s" % (tuple(t.stride()),)
    storage, view = _carve(tuple(t.shape), tuple(t.stride()), t.dtype, t.device, fill, 0)
    view.copy_(t)
    return storage, view


def guarded_like(shape, dtype, memory_format=torch.contiguous_format, device="cpu", fill=0xFF):
    """guarded() for an output: the interior holds the fill as well, so an element the kernel never wrote shows (0xFF: NaN)."""
    strides = torch.empty(tuple(shape), dtype=dtype, device="meta", memory_format=memory_format).stride()
    return _carve(tuple(shape), strides, dtype, torch.device(device), fill, fill)


def _extent(storage, view):
    lo = view.data_ptr() - storage.data_ptr()
    hi = lo + view.numel() * view.element_size()
    assert 0 < lo and hi < storage.numel(), "the view does not lie inside the storage"
    return lo, hi


def guards_intact(storage, view, fill=0xFF):
    """Both guards of ``storage`` around ``view`` still hold the fill, bit for bit."""
    lo, hi = _extent(storage, view)
    return bool(torch.equal(storage[:lo], _pattern(fill, lo, storage.device))
                and torch.equal(storage[hi:], _pattern(fill, storage.numel() - hi, storage.device)))


def same_bits(a, b):
    """Equal shape, dtype and bit patterns (integer views: NaN equals the same NaN, +0.0 differs from -0.0)."""
    if tuple(a.shape) != tuple(b.shape) or a.dtype != b.dtype:
        return False
    if not a.dtype.is_floating_point:
        return bool(torch.equal(a, b))
    iv = _INT_VIEW[a.element_size()]
    return bool(torch.equal(a.view(iv), b.view(iv)))


def has_nan(t):
    return bool(torch.isnan(t).any())


class GuardSet(object):
    """The guarded buffers of one call.  ``inp`` / ``out`` hand out the views; ``arm()`` snapshots every storage once all are
    made; ``problems()`` after the call lists every guard that changed and every input whose interior changed."""

    def __init__(self, device="cpu"):
        self.device = torch.device(device)
        self.items = []  # [name, storage, view, fill, is_input]
        self.before = None

    def inp(self, name, t, fill=0xFF):
        storage, view = guarded(t.to(self.device), fill)
        self.items.append((name, storage, view, fill, True))
        return view

    def out(self, name, shape, dtype, memory_format=torch.contiguous_format, fill=0xFF):
        storage, view = guarded_like(shape, dtype, memory_format, self.device, fill)
        self.items.append((name, storage, view, fill, False))
        return view

    def zeros(self, name, nbytes, fill=0xFF):
        """A zero-filled uint8 scratch between guards (split-K tickets are zero by contract); watched like an output."""
        storage, view = guarded(torch.zeros(int(nbytes), dtype=torch.uint8, device=self.device), fill)
        self.items.append((name, storage, view, fill, False))
        return view

    def adopt(self, name, storage, view, fill=0xFF, is_input=True):
        self.items.append((name, storage, view, fill, is_input))
        return view

    def arm(self):
        self.before = [storage.clone() for _, storage, _, _, _ in self.items]
        return self

    def problems(self):
        assert self.before is not None, "arm() first"
        bad = []
        for (name, storage, view, fill, is_input), before in zip(self.items, self.before):
            if not guards_intact(storage, view, fill):
                bad.append("a guard of %s was written" % name)
            lo, hi = _extent(storage, view)
            if is_input and not torch.equal(storage[lo:hi], before[lo:hi]):
                bad.append("the input %s was written" % name)
        return bad


# ---- packs: every tensor a descriptor filler takes a pointer from, relocated into guarded storage of exactly its size ----------
_CONV_FIELDS = ("w", "scale", "bias")
_STEM_FIELDS = ("w", "scale", "bias")
_MBSE_FIELDS = ("w_dw", "scale_dw", "bias_dw", "w_se1", "b_se1", "w_se2", "b_se2", "w_proj", "scale_proj", "bias_proj")


def _move(obj, field, label, out, fill):
    t = getattr(obj, field)
    if t is None:
        return
    storage, view = guarded(t, fill)
    setattr(obj, field, view)
    out.append((label, storage, view))


def guard_pack(pack, width=None, fill=0xFF):
    """Relocates the tensors of a ``ConvPack`` / ``MbPack`` / ``StemPack`` / ``MbSePack`` (in place) -> [(name, storage, view)].
    The pack as built is the contract: a layout documented as padded (StemPack's taps and channels, the rows of a fragment image
    rounded up to 16) keeps its padding inside the view.  ``width``: the map width an ``MbPack``'s ``image(width)`` is built for
    (None: no image)."""
    from ssds.modeling.layers import fused_conv as FC

    out = []
    if isinstance(pack, FC.ConvPack):
        for f in _CONV_FIELDS:
            _move(pack, f, f, out, fill)
        # frag() / gfrag() cache by (w.data_ptr(), w._version): build the image from the moved w, move it too, re-install it
        pack._frag = None
        img = pack.gfrag() if pack.kind == "gany" else pack.frag()
        if img is not None:
            storage, view = guarded(img, fill)
            pack._frag = ((pack.w.data_ptr(), pack.w._version), view)
            assert (pack.gfrag() if pack.kind == "gany" else pack.frag()).data_ptr() == view.data_ptr()
            out.append(("w_frag", storage, view))
    elif isinstance(pack, FC.MbPack):
        for f in _CONV_FIELDS:
            _move(pack.e, f, "e." + f, out, fill)
        for f in ("wd", "bd", "wp"):
            _move(pack, f, f, out, fill)
        for f in ("scale", "bias"):
            _move(pack.p, f, "p." + f, out, fill)
        pack._image = None
        im = pack.image(width) if width is not None else None
        if im is not None:
            nw, img = im
            storage, view = guarded(img, fill)
            pack._image = (pack._image[0], (nw, view))
            assert pack.image(width)[1].data_ptr() == view.data_ptr() and view.numel() == img.numel()
            out.append(("w_image", storage, view))
    elif isinstance(pack, FC.StemPack):
        for f in _STEM_FIELDS:
            _move(pack, f, f, out, fill)
    elif isinstance(pack, FC.MbSePack):
        for f in _MBSE_FIELDS:
            _move(pack, f, f, out, fill)
    else:
        raise TypeError("guard_pack: %r" % type(pack))
    return out
