"""``ssdk_augment`` on the device against the fp64 oracle (tests/augment_oracle.py), and ``AugmentedLoader`` end to end.

The tolerance is derived, not tuned (DESIGN.md "Data input").  The kernel as written, per output element:
  * integer taps, exact; weights ``remainder / (2 W)`` in fp32: one rounding (relative 2^-24);
  * per tap 6 fp32 operations before the clamp (3 products, 3 sums of ``color . (r, g, b, 1)``; the uint8 -> fp32 conversions
    are exact) on magnitudes below 1 024 (below 600 with the default PREPROC ranges: |row| sums <= 2.19, offset <= 34, which
    tests/test_augment_cpu.py::test_color_matrix asserts): each off by at most half an ulp, 2^-15 = 3.1e-5 -> 1.8e-4;
  * 3 interpolations ``a + (b - a) * f`` of values <= 255, two levels deep: a difference, a product (which also carries the
    weight's rounding, 255 * 2^-24) and a sum, each at most half an ulp of 256 (7.6e-6) -> 3.8e-5 per level, 7.6e-5;
  * ``(o - mean) / std``: a difference (7.6e-6) and a quotient (relative 2^-24 of at most 255: 1.5e-5);
  together under 3e-4 grey levels, inside the 6e-4 of the issue's count (seven operations and three interpolations) and the
  bound asserted here: fp32 outputs within 1e-3 / STD[c] of the oracle.  16-bit outputs: within one ulp of the type of the
  oracle's value rounded to that type (the fp32 error can flip one rounding) -- see ``compare`` for outputs next to zero, where
  a 16-bit ulp is smaller than the fp32 bound itself.  Every element is compared.

Measured on an MI355X with the kernel as written (printed by every case before it asserts): fp32 largest error 4.8e-5 ..
6.0e-5 grey levels over all cases (the issue's numpy emulation of the chain: 5.6e-5); bf16 / f16 never more than one ulp
where the ulp is at least T = 1e-3 / STD[c] (12 .. 8 658 elements of 2.4 M .. 47 M one ulp off).  Next to zero (|v| < 0.004
bf16, < 0.031 f16, reached with MEAN = (104, 117, 123) where an output crosses zero) 11 .. 602 elements per case are more than
one ulp of their own tiny magnitude off, all within 0.91 T; with the shipped MEAN 0 / STD 255 there is none."""
import os
from collections import OrderedDict

import numpy as np
import pytest

import augment_oracle as AO

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PREPROC = {"MEAN": 0, "STD": 255, "CROP_SCALE": [0.3, 1.0], "CROP_ASPECT_RATIO": [0.5, 2.0], "CROP_ATTEMPTS": 50, "HUE_DELTA": 9,
           "BRI_DELTA": 16, "CONTRAST_RANGE": [0.75, 1.25], "SATURATION_RANGE": [0.75, 1.25], "MAX_EXPAND_RATIO": 2.0}
GUARD_BYTE, GUARD_BYTES = 0xA5, 1 << 16


def _pack_tool():
    import importlib.util

    spec = importlib.util.spec_from_file_location("pack_dataset", os.path.join(ROOT, "tools", "pack_dataset.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def run_kernel(pixels, descs, H, W, mean, std, dtype):
    """The packed buffer lies at the front of an allocation whose rest is a guard of GUARD_BYTE: pixels_bytes ends exactly
    where the guard begins, so a read past the last image would show as 165 in the output instead of faulting."""
    import torch

    from ssds import _native as N
    from ssds.dataset import augment as A

    dev = torch.device("cuda")
    buf = torch.full((pixels.size + GUARD_BYTES,), GUARD_BYTE, dtype=torch.uint8, device=dev)
    buf[:pixels.size].copy_(torch.from_numpy(pixels))
    B = len(descs)
    out = torch.full((B, 3, H, W), float("nan"), dtype=getattr(torch, dtype), device=dev)
    ws = torch.empty(int(N.lib.ssdk_augment_workspace_bytes(B)), dtype=torch.uint8, device=dev)
    host = np.ascontiguousarray(descs).view(np.uint8).reshape(-1)
    A.augment_into(out, buf, pixels.size, host, B, mean, std, ws)
    torch.cuda.synchronize()
    assert N.last_kernel() == "augment_kernel"
    assert bool((buf[pixels.size:] == GUARD_BYTE).all())
    return out.float().cpu().numpy().astype(np.float64)


def compare(got, want, std, dtype, what):
    """fp32: |got - want| <= T = 1e-3 / STD[c].  16-bit: |got - round(want)| <= one ulp of the type at round(want) -- except
    where that ulp is smaller than T itself (outputs next to zero, |v| < T * 2^(mantissa bits): the subtraction of MEAN and
    the colour sum cancel there, and a 16-bit grid finer than the fp32 bound cannot be held by any fp32 chain), where the
    fp32 bound T is what is asserted.  Prints every figure, then asserts."""
    from ssds.dataset.augment import vec3

    assert got.shape == want.shape and np.isfinite(got).all(), what
    T = 1e-3 / vec3(std).reshape(1, 3, 1, 1)
    if dtype == "float32":
        err = np.abs(got - want) / T * 1e-3
        print("{}: {} elements, largest |error| {:.3g} grey levels (bound 1e-3)".format(what, got.size, err.max()))
        assert err.max() <= 1e-3, what
    else:
        r, ulp = AO.round_to(want, dtype)
        err = np.abs(got - r)
        fine = np.broadcast_to(ulp < T, err.shape)  # the 16-bit grid is finer than the fp32 bound
        e_ulp = np.where(fine, 0.0, err / ulp)
        e_fine = np.where(fine, err / T, 0.0)
        print("{}: {} elements; {} with ulp >= T: largest |error| {:.3g} ulp of {} (bound 1), {} off by one; {} with ulp < T "
              "(largest |value| {:.3g}): largest |error| {:.3g} T (bound 1), {} of them more than one ulp off".format(
                  what, got.size, int((~fine).sum()), e_ulp.max(), dtype, int((e_ulp > 0).sum()), int(fine.sum()),
                  np.abs(r[fine]).max() if fine.any() else 0.0, e_fine.max(), int((fine & (err > ulp)).sum())))
        assert e_ulp.max() <= 1.0, what
        assert e_fine.max() <= 1.0, what


def desc(A, src_offset, sh, sw, crop=None, canvas=None, paste=(0, 0), flip=0, color=None, fill=(0, 0, 0)):
    d = np.zeros((), A.DESC_DTYPE)
    cx, cy, cw, ch = crop if crop is not None else (0, 0, sw, sh)
    cvw, cvh = canvas if canvas is not None else (cw, ch)
    for k, v in dict(src_offset=src_offset, src_h=sh, src_w=sw, crop_x=cx, crop_y=cy, crop_w=cw, crop_h=ch, canvas_w=cvw,
                     canvas_h=cvh, paste_x=paste[0], paste_y=paste[1], flip=flip).items():
        d[k] = v
    d["color"] = A.IDENTITY_COLOR if color is None else np.asarray(color, np.float64).reshape(12)
    d["fill"] = fill
    return d


def hand_batch():
    """Sources from 1x1 to 1333x800 with odd widths; crops touching every border; flip on and off; the pasted crop in each
    corner of its canvas and inside it; identity and twisted colours; up- and down-scaling follows from the target size."""
    from ssds.dataset import augment as A

    rs = np.random.default_rng(17)
    sizes = [(1, 1), (1, 7), (5, 1), (37, 53), (800, 1333), (480, 640), (301, 299)]
    imgs = [rs.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]
    off = np.concatenate([[0], np.cumsum([im.size for im in imgs])])
    pixels = np.concatenate([im.reshape(-1) for im in imgs])
    twist = lambda: A.color_matrix(rs.uniform(-9, 9), rs.uniform(0.75, 1.25), rs.uniform(15 / 16, 17 / 16), rs.uniform(0.75, 1.25))  # noqa: E731
    fill = (104, 117, 123)
    D = []
    for i, (h, w) in enumerate(sizes):  # whole images, identity and twisted, flipped and not
        D.append(desc(A, off[i], h, w, fill=fill))
        D.append(desc(A, off[i], h, w, flip=1, color=twist(), fill=fill))
    h, w = sizes[4]
    i = 4
    for crop in ((0, 0, 400, 300), (w - 401, 0, 401, 333), (0, h - 299, 555, 299), (w - 777, h - 555, 777, 555), (w - 1, h - 1, 1, 1),
                 (0, 0, w, 1), (w - 1, 0, 1, h), (100, 50, 900, 700)):
        cw, ch = crop[2], crop[3]
        cv = (int(cw * 1.7) + 1, int(ch * 1.3) + 2)
        for k, paste in enumerate(((0, 0), (cv[0] - cw, 0), (0, cv[1] - ch), (cv[0] - cw, cv[1] - ch), ((cv[0] - cw) // 2, (cv[1] - ch) // 3))):
            D.append(desc(A, off[i], h, w, crop, cv, paste, flip=k & 1, color=twist() if k % 3 else None, fill=fill))
    for i in (3, 5, 6):  # smaller sources: upscaling to every target
        h, w = sizes[i]
        D.append(desc(A, off[i], h, w, (1, 2, w - 3, h - 5), (w + 9, h + 4), (9, 0), 1, twist(), fill))
        D.append(desc(A, off[i], h, w, (w // 2, h // 2, w - w // 2, h - h // 2), (w, h), (3, h // 2 - 1), 0, twist(), fill))
    return pixels, np.array(D, A.DESC_DTYPE)


def sampled_batch(H, W, mean):
    from ssds.dataset import augment as A

    rs = np.random.default_rng(23)
    shapes = np.stack([rs.integers(100, 500, 12), rs.integers(100, 700, 12)], 1)
    shapes[0] = (800, 1333)
    imgs = [rs.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in shapes]
    boxes = []
    for h, w in shapes:
        k = int(rs.integers(0, 6))
        bw, bh = rs.uniform(0.2, 0.9, k) * w, rs.uniform(0.2, 0.9, k) * h
        l, t = rs.uniform(0, 1, k) * (w - bw), rs.uniform(0, 1, k) * (h - bh)
        boxes.append(np.stack([l, t, l + bw, t + bh, rs.integers(0, 5, k).astype(np.float64)], 1))
    descs, _, _ = A.sample_batch(A.batch_rng(1, 0, 0, 0), shapes, boxes, dict(PREPROC, MEAN=mean), (H, W), True)
    size = np.array([im.size for im in imgs])
    descs["src_offset"] = np.concatenate([[0], np.cumsum(size)[:-1]])
    return np.concatenate([im.reshape(-1) for im in imgs]), descs


MEAN3, STD3 = [104.0, 117.0, 123.0], [58.0, 57.0, 59.5]
_CASES = {}


def cases(size):
    """(name, pixels, descs, mean, std, oracle output) of one target size; the oracle is rendered once for the three dtypes."""
    if size not in _CASES:
        H, W = size
        hp, hd = hand_batch()
        sp, sd = sampled_batch(H, W, MEAN3)
        _CASES[size] = [("hand-made descriptors", hp, hd, MEAN3, STD3, AO.render_batch(hp, hd, H, W, MEAN3, STD3)),
                        ("sampled descriptors", sp, sd, MEAN3, STD3, AO.render_batch(sp, sd, H, W, MEAN3, STD3)),
                        # the shipped configs' scalars
                        ("sampled descriptors, MEAN 0 STD 255", sp, sd, 0, 255, AO.render_batch(sp, sd, H, W, [0] * 3, [255] * 3))]
    return _CASES[size]


@pytest.mark.parametrize("dtype", ["float32", "bfloat16", "float16"])
@pytest.mark.parametrize("size", [(300, 300), (512, 512), (200, 333)])
def test_kernel_matches_fp64_oracle(size, dtype):
    H, W = size
    for name, pixels, descs, mean, std, want in cases(size):
        got = run_kernel(pixels, descs, H, W, mean, std, dtype)
        compare(got, want, std, dtype, "{} {}x{} {}".format(name, H, W, dtype))


@pytest.mark.parametrize("dtype", ["float32", "bfloat16", "float16"])
def test_identity_case_is_ssdk_preprocess_bit_for_bit(dtype):
    """Eval mode with the source already at IMAGE_SIZE: every weight is 0, the colour matrix the exact identity."""
    import torch

    from ssds.dataset import augment as A
    from ssds.ssds import preprocess

    rs = np.random.default_rng(5)
    B, H, W = 3, 300, 300
    raw = rs.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    for mean, std in ((0, 255), ([104.0, 117.0, 123.0], [58.0, 57.0, 59.5])):
        descs, _, _ = A.sample_batch(A.batch_rng(0, 0, 0, 0), [(H, W)] * B, [np.zeros((0, 5))] * B, dict(PREPROC, MEAN=mean), (H, W), False)
        descs["src_offset"] = np.arange(B) * H * W * 3
        dev = torch.from_numpy(raw).cuda()
        out = torch.empty((B, 3, H, W), dtype=getattr(torch, dtype), device="cuda")
        from ssds import _native as N

        ws = torch.empty(int(N.lib.ssdk_augment_workspace_bytes(B)), dtype=torch.uint8, device="cuda")
        A.augment_into(out, dev.view(-1), raw.size, descs.view(np.uint8).reshape(-1), B, mean, std, ws)
        m, s = (list(A.vec3(v)) for v in (mean, std))
        want = preprocess(dev, m, s, getattr(torch, dtype))
        torch.cuda.synchronize()
        assert out.dtype == want.dtype and torch.equal(out.view(torch.uint8), want.view(torch.uint8))


def test_no_read_past_the_end_of_the_packed_buffer():
    """The last image's last row and column are the last bytes of ``pixels``; behind them lies the guard of 0xA5 = 165.  The
    sources hold values <= 100 and the colour matrix is the identity, so any output above 100 would be a guard byte."""
    from ssds.dataset import augment as A

    rs = np.random.default_rng(9)
    sizes = [(33, 47), (64, 61)]
    imgs = [rs.integers(0, 101, (h, w, 3), dtype=np.uint8) for h, w in sizes]
    pixels = np.concatenate([im.reshape(-1) for im in imgs])
    o1 = imgs[0].size
    h, w = sizes[1]
    D = [desc(A, o1, h, w), desc(A, o1, h, w, flip=1), desc(A, o1, h, w, (w - 9, h - 7, 9, 7)), desc(A, o1, h, w, (w - 1, h - 1, 1, 1), flip=1),
         desc(A, o1, h, w, (0, h - 1, w, 1)), desc(A, o1, h, w, (w - 1, 0, 1, h)), desc(A, 0, 33, 47, (40, 30, 7, 3)),
         desc(A, o1, h, w, (w - 20, h - 20, 20, 20), (31, 29), (11, 9), 1, fill=(50, 50, 50))]
    descs = np.array(D, A.DESC_DTYPE)
    for H, W in ((96, 96), (17, 23)):
        got = run_kernel(pixels, descs, H, W, 0, 1, "float32")
        compare(got, AO.render_batch(pixels, descs, H, W, [0] * 3, [1] * 3), 1, "float32", "last row / column {}x{}".format(H, W))
        assert got.max() <= 100.0 + 1e-3


def _toy(tmp_path, n=24):
    from ssds.dataset import augment as A

    pk = _pack_tool()
    images, boxes = pk.synthetic_set(n, seed=2, height=(100, 160), width=(120, 200))
    pk.write_shards(str(tmp_path), images, boxes, per_shard=10)
    return A.PackedDetectionSource(str(tmp_path))


def test_loader_equals_synchronous_launches(tmp_path):
    """Two epochs: the side stream and the prefetch change nothing -- every batch is bit for bit what one synchronous
    ``ssdk_augment`` on the same descriptors gives; nothing is dropped by max_gt."""
    import torch

    from ssds import _native as N
    from ssds.dataset import augment as A

    src = _toy(tmp_path)
    cfg = {"IMAGE_SIZE": [128, 160], "PREPROC": PREPROC}
    dev = torch.device("cuda")
    loader = A.AugmentedLoader(src, cfg, 4, dev, dtype=torch.bfloat16, training=True, seed=7, max_gt=8)
    twin = A.AugmentedLoader(src, cfg, 4, dev, dtype=torch.bfloat16, training=True, seed=7, max_gt=8)
    assert len(loader) == 6
    first = []
    for epoch in range(2):
        seen = 0
        for b, (images, targets) in enumerate(loader):
            idx = twin.batches(epoch)[b]
            descs, want_t, _, nbytes = twin.describe(epoch, b, idx)
            pixels = np.concatenate([src.pixels(int(i)) for i in idx])
            assert pixels.size == nbytes
            out = torch.empty((4, 3, 128, 160), dtype=torch.bfloat16, device=dev)
            ws = torch.empty(int(N.lib.ssdk_augment_workspace_bytes(4)), dtype=torch.uint8, device=dev)
            A.augment_into(out, torch.from_numpy(pixels).to(dev), nbytes, descs.view(np.uint8).reshape(-1), 4, 0, 255, ws)
            torch.cuda.synchronize()
            assert images.shape == out.shape and images.dtype == torch.bfloat16 and images.device.type == "cuda"
            assert torch.equal(images.view(torch.int16), out.view(torch.int16)), (epoch, b)
            assert targets.shape == (4, 8, 5) and targets.dtype == torch.float32
            np.testing.assert_array_equal(targets.cpu().numpy(), want_t)
            if b == 0:
                first.append(images.clone())
            seen += 1
        assert seen == 6 and loader.dropped == 0
    assert not torch.equal(first[0], first[1]), "another epoch draws another order and other augmentations"


def test_train_and_eval_epochs_take_the_loader(tmp_path):
    """train_step runs three steps on the loader's batches with finite losses; eval_anchor_based_epoch runs on the
    eval-mode loader (maxG per batch, as the reference's contract has it)."""
    import torch

    from ssds.core import criterion
    from ssds.dataset import augment as A
    from ssds.modeling import nets, ssds
    from ssds.modeling.layers import box
    from ssds.modeling.layers.decoder import Decoder
    from ssds.pipeline.pipeline_anchor_ddp import ModelWithLossBasic, eval_anchor_based_epoch, train_step

    src = _toy(tmp_path)
    cfg = {"IMAGE_SIZE": [128, 128], "PREPROC": PREPROC}
    dev = torch.device("cuda")
    torch.manual_seed(0)
    o, e, h = ssds.SSD.add_extras([[5, 7, "Conv:S"], [96, 320, 64]], [2, 2, 2], 5)
    model = ssds.SSD(nets.MobileNetV2(outputs=o), e, h, 5)
    mwl = ModelWithLossBasic(model, criterion.FocalLoss(), criterion.SmoothL1Loss(), 5, [0.5, 0.4], 0).cuda()
    anchors = OrderedDict((s, box.generate_anchors(s, [1], [2.0, 2.828])) for s in (16, 32, 64))
    opt = torch.optim.SGD(mwl.parameters(), lr=0.01, momentum=0.9)
    loader = A.AugmentedLoader(src, cfg, 4, dev, dtype=torch.float32, training=True, seed=3)
    mwl.train()
    steps = 0
    for images, targets in loader:
        c, l, skipped = train_step(mwl, images, targets, anchors, opt)
        assert np.isfinite(float(c)) and np.isfinite(float(l)) and not bool(skipped)
        steps += 1
        if steps == 3:
            break
    assert steps == 3
    ev = A.AugmentedLoader(src, cfg, 5, dev, dtype=torch.float32, training=False)
    assert len(ev) == 5  # 24 images: four batches of five and one of four
    shapes = [tuple(t.shape) for _, t in ev]
    assert [s[0] for s in shapes] == [5, 5, 5, 5, 4] and all(s[2] == 5 for s in shapes)
    ev.set_epoch(0)
    o, e, h = ssds.SSD.add_extras([[5, 7, "Conv:S"], [96, 320, 64]], [6, 6, 6], 5)
    emodel = ssds.SSD(nets.MobileNetV2(outputs=o), e, h, 5).cuda().eval()
    eanchors = OrderedDict((s, box.generate_anchors(s, [1, 2, 0.5], [2.0, 2.828])) for s in (16, 32, 64))
    mAP, (prec, rec, ap) = eval_anchor_based_epoch(emodel, ev, Decoder(0.005, 0.5, 50, 200, False, False), eanchors, 5, dev)
    assert np.isfinite(float(mAP)) and 0.0 <= float(mAP) <= 1.0
