"""Host side of the training input pipeline (ssds/dataset/augment.py, tools/pack_dataset.py) and the argument checks of
``ssdk_augment`` -- no GPU: the sampler is numpy, and the library validates every descriptor before it touches a device."""
import ctypes
import importlib.util
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import augment_oracle as AO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PREPROC = {"MEAN": 0, "STD": 255, "CROP_SCALE": [0.3, 1.0], "CROP_ASPECT_RATIO": [0.5, 2.0], "CROP_ATTEMPTS": 50, "HUE_DELTA": 9,
           "BRI_DELTA": 16, "CONTRAST_RANGE": [0.75, 1.25], "SATURATION_RANGE": [0.75, 1.25], "MAX_EXPAND_RATIO": 2.0}
SIZE = (300, 512)  # (height, width): not square, so a swapped axis shows


def _pack_tool():
    spec = importlib.util.spec_from_file_location("pack_dataset", os.path.join(ROOT, "tools", "pack_dataset.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def draw_inputs(rs, n, max_boxes=16):
    """The distribution the fallback cap is stated for: width U{200..1333}, height U{200..800}, 0..16 boxes, each side
    U(5 %, 95 %) of the image side, position uniform where it fits."""
    shapes = np.stack([rs.integers(200, 801, n), rs.integers(200, 1334, n)], 1)
    boxes = []
    for h, w in shapes:
        k = int(rs.integers(0, max_boxes + 1))
        bw, bh = rs.uniform(0.05, 0.95, k) * w, rs.uniform(0.05, 0.95, k) * h
        l, t = rs.uniform(0, 1, k) * (w - bw), rs.uniform(0, 1, k) * (h - bh)
        boxes.append(np.stack([l, t, l + bw, t + bh, rs.integers(0, 80, k).astype(np.float64)], 1))
    return shapes, boxes


def _sample_many(seed, rank, n_batches=32, B=64):
    from ssds.dataset import augment as A

    rs = np.random.default_rng(99)
    out = []
    for b in range(n_batches):
        shapes, boxes = draw_inputs(rs, B)
        descs, targets, info = A.sample_batch(A.batch_rng(seed, rank, 0, b), shapes, boxes, PREPROC, SIZE, True)
        out.append((shapes, boxes, descs, targets, info))
    return out


def test_sampler_invariants_and_fallback_share():
    """2 048 seeded images (32 batches of 64) of the distribution of ``draw_inputs``.  The same seed gives identical
    descriptors and targets, another rank different ones; every kept box had its centre strictly inside the crop and
    IoU >= the chosen threshold with it; targets lie inside the network input with positive size, labels unchanged; crop
    inside the image, paste inside the canvas, canvas <= MAX_EXPAND_RATIO x crop; padding rows are -1 and maxG follows
    the contract.  "No crop" and the thresholds 0 .. 0.7 each occur.

    A condition, not a measurement: at most 2 % of the images may end in the 8-round fallback (option -1).  The sampler as
    specified reaches 0.73 % on these inputs (15 of 2 048; no crop 554 = 27 %, thresholds 0 / 0.1 / 0.3 / 0.5 / 0.7 accepted
    526 / 511 / 323 / 77 / 26 times, 0.9 16 times -- all of them images without boxes, which accept the first
    aspect-valid rectangle whatever the option)."""
    from ssds.dataset import augment as A

    runs = _sample_many(5, 0)
    again = _sample_many(5, 0)
    other = _sample_many(5, 1)
    H, W = SIZE
    options = []
    differ = 0
    for (shapes, boxes, descs, targets, info), (_, _, d2, t2, _), (_, _, d3, t3, _) in zip(runs, again, other):
        assert descs.tobytes() == d2.tobytes() and targets.tobytes() == t2.tobytes()
        differ += descs.tobytes() != d3.tobytes()
        B = len(shapes)
        options.extend(info["option"].tolist())
        assert ((info["round"] >= 0) & (info["round"] <= A.CROP_ROUNDS)).all()
        assert ((info["option"] == -1) == (info["round"] == A.CROP_ROUNDS)).all()
        counts = []
        for i in range(B):
            d, (sh, sw) = descs[i], shapes[i]
            cx, cy, cw, ch = int(d["crop_x"]), int(d["crop_y"]), int(d["crop_w"]), int(d["crop_h"])
            assert (int(d["src_h"]), int(d["src_w"])) == (sh, sw)
            assert cw >= 1 and ch >= 1 and cx >= 0 and cy >= 0 and cx + cw <= sw and cy + ch <= sh
            assert int(d["paste_x"]) >= 0 and int(d["paste_x"]) + cw <= int(d["canvas_w"])
            assert int(d["paste_y"]) >= 0 and int(d["paste_y"]) + ch <= int(d["canvas_h"])
            assert cw <= int(d["canvas_w"]) <= PREPROC["MAX_EXPAND_RATIO"] * cw and ch <= int(d["canvas_h"]) <= PREPROC["MAX_EXPAND_RATIO"] * ch
            assert int(d["flip"]) in (0, 1)
            opt = int(info["option"][i])
            if opt <= 0:
                assert (cx, cy, cw, ch) == (0, 0, sw, sh)
            keep = info["keep"][i][:len(boxes[i])]
            assert not info["keep"][i][len(boxes[i]):].any()
            if opt > 0:
                thr = A.CROP_THRESHOLDS[opt - 1]
                assert len(boxes[i]) == 0 or keep.any()
                for box, k in zip(boxes[i], keep):
                    bx, by = (box[0] + box[2]) / 2, (box[1] + box[3]) / 2
                    inside = cx < bx < cx + cw and cy < by < cy + ch
                    assert bool(k) == inside
                    if k:
                        assert AO.iou_with_rect(box, cx, cy, cw, ch) >= thr
            else:
                assert keep.all()
            rows = targets[i][targets[i][:, 4] >= 0]
            counts.append(len(rows))
            assert len(rows) == int(keep.sum())
            np.testing.assert_array_equal(rows[:, 4], boxes[i][keep][:, 4].astype(np.float32))
            assert (rows[:, 2] > 0).all() and (rows[:, 3] > 0).all()
            eps = 1e-3  # float32 targets of fp64 geometry
            assert (rows[:, 0] >= -eps).all() and (rows[:, 1] >= -eps).all()
            assert (rows[:, 0] + rows[:, 2] <= W + eps).all() and (rows[:, 1] + rows[:, 3] <= H + eps).all()
            pad = targets[i][len(rows):]
            assert (pad == -1).all() and (targets[i][:len(rows), 4] >= 0).all()
        assert targets.shape == (B, max(1, max(counts)), 5) and targets.dtype == np.float32
    assert differ == len(runs), "another rank must draw another stream"
    options = np.array(options)
    n = len(options)
    assert n >= 2000
    share = float((options == -1).sum()) / n
    hist = {k: int((options == k).sum()) for k in range(-1, 7)}
    print("fallback {} of {} = {:.2%}; options {}".format(hist[-1], n, share, hist))
    assert share <= 0.02, hist
    for k in range(0, 6):  # no crop, thresholds 0, 0.1, 0.3, 0.5, 0.7
        assert hist[k] >= 1, hist


def test_threshold_09_is_reachable():
    """One box covering the whole image and CROP_SCALE = [0.9, 1.0]: a crop's IoU with the box is its relative area, so the
    option 0.9 is accepted within a few hundred seeded images -- and every crop it accepts holds that IoU."""
    from ssds.dataset import augment as A

    pre = dict(PREPROC, CROP_SCALE=[0.9, 1.0])
    shapes = np.tile([[480, 640]], (64, 1))
    boxes = [np.array([[0, 0, 640, 480, 3.0]])] * 64
    hits = 0
    for b in range(5):
        descs, targets, info = A.sample_batch(A.batch_rng(11, 0, 0, b), shapes, boxes, pre, SIZE, True)
        for d, o in zip(descs, info["option"]):
            if o == 6:
                hits += 1
                assert int(d["crop_w"]) * int(d["crop_h"]) >= 0.9 * 640 * 480
        assert (targets[:, 0, 4] == 3).all()
    assert hits >= 1


def test_all_empty_batch_and_max_gt():
    from ssds.dataset import augment as A

    shapes = np.array([[200, 300], [240, 200], [333, 517]])
    none = [np.zeros((0, 5))] * 3
    descs, targets, info = A.sample_batch(A.batch_rng(1, 0, 0, 0), shapes, none, PREPROC, SIZE, True)
    assert targets.shape == (3, 1, 5) and (targets == -1).all() and (info["option"] >= 0).all()
    # max_gt: exactly that many rows; more boxes -> the largest by area stay, in order, and the rest are counted
    big = np.array([[0, 0, 100, 100, 1], [10, 10, 20, 20, 2], [0, 0, 150, 120, 3], [5, 5, 50, 50, 4.0]])
    descs, targets, info = A.sample_batch(A.batch_rng(1, 0, 0, 0), shapes[:1], [big], PREPROC, SIZE, False, max_gt=2)
    assert targets.shape == (1, 2, 5) and info["dropped"] == 2 and targets[0, :, 4].tolist() == [1, 3]
    descs, targets, info = A.sample_batch(A.batch_rng(1, 0, 0, 0), shapes[:1], [big], PREPROC, SIZE, False, max_gt=7)
    assert targets.shape == (1, 7, 5) and info["dropped"] == 0 and (targets[0, 4:] == -1).all()


def test_geometry_round_trip():
    """Targets mapped back through the inverse of resize, paste, flip and the crop's shift are the source boxes, within 1
    source pixel.  No crop loss by construction: CROP_SCALE = [1, 1] makes every crop the whole image, so nothing is clipped
    or dropped and flip / paste / resize are what is inverted."""
    from ssds.dataset import augment as A

    pre = dict(PREPROC, CROP_SCALE=[1.0, 1.0])
    rs = np.random.default_rng(3)
    flips = set()
    for b in range(6):
        shapes, boxes = draw_inputs(rs, 32)
        descs, targets, info = A.sample_batch(A.batch_rng(2, 0, 0, b), shapes, boxes, pre, SIZE, True)
        for i in range(len(shapes)):
            flips.add(int(descs[i]["flip"]))
            back = AO.targets_to_source(targets[i], descs[i], *SIZE)
            want = boxes[i][info["keep"][i][:len(boxes[i])]]
            assert back.shape == want.shape
            if len(want):
                assert np.abs(back[:, :4] - want[:, :4]).max() <= 1.0
                np.testing.assert_array_equal(back[:, 4], want[:, 4])
    assert flips == {0, 1}


def test_color_matrix():
    from ssds.dataset import augment as A

    ident = A.color_matrix(0.0, 1.0, 1.0, 1.0)
    assert np.abs(ident - np.eye(3, 4)).max() < 1e-6
    grey = A.color_matrix(4.0, 0.0, 1.03, 0.9)
    px = np.random.default_rng(0).uniform(0, 255, (1000, 3))
    out = px @ grey[:, :3].T + grey[:, 3]
    assert np.abs(out - out[:, :1]).max() < 1e-9
    rs = np.random.default_rng(1)
    for _ in range(50):
        hue, sat, bri, con = rs.uniform(-9, 9), rs.uniform(0.75, 1.25), rs.uniform(1 - 1 / 16, 1 + 1 / 16), rs.uniform(0.75, 1.25)
        m = A.color_matrix(hue, sat, bri, con)
        assert np.abs(px @ m[:, :3].T + m[:, 3] - AO.color_steps(px, hue, sat, bri, con)).max() < 1e-9
        # the bound the kernel's tolerance is derived with: |row| sums <= 2.19, offset <= 34
        assert np.abs(m[:, :3]).sum(1).max() <= 2.19 and np.abs(m[:, 3]).max() <= 34.0
    # broadcasting over a batch is the scalar fold
    hs = rs.uniform(-9, 9, 5)
    np.testing.assert_array_equal(A.color_matrix(hs, 1.1, 0.97, 1.2)[3], A.color_matrix(hs[3], 1.1, 0.97, 1.2))


def test_eval_mode_is_resize_only():
    from ssds.dataset import augment as A

    rs = np.random.default_rng(4)
    shapes, boxes = draw_inputs(rs, 16)
    descs, targets, info = A.sample_batch(A.batch_rng(0, 0, 0, 0), shapes, boxes, dict(PREPROC, MEAN=[104, 117, 123]), SIZE, False)
    for i, (h, w) in enumerate(shapes):
        d = descs[i]
        assert [int(d[k]) for k in ("crop_x", "crop_y", "crop_w", "crop_h", "canvas_w", "canvas_h", "paste_x", "paste_y", "flip")] == [
            0, 0, w, h, w, h, 0, 0, 0]
        assert d["color"].tobytes() == np.eye(3, 4, dtype=np.float32).tobytes()
        assert d["fill"].tolist() == [104, 117, 123]
        assert info["keep"][i][:len(boxes[i])].all()
        rows = targets[i][:len(boxes[i])]
        want = boxes[i] * [SIZE[1] / w, SIZE[0] / h, SIZE[1] / w, SIZE[0] / h, 1]
        np.testing.assert_allclose(rows[:, :2], want[:, :2], rtol=1e-6, atol=1e-4)
        np.testing.assert_allclose(rows[:, 2:4], want[:, 2:4] - want[:, :2], rtol=1e-6, atol=1e-4)


# ---- C-ABI ----------------------------------------------------------------------------------------------------------------
def _good(N, B=2):
    d = (N.AugmentDesc * B)()
    for i in range(B):
        d[i].src_offset, d[i].src_h, d[i].src_w = i * 300, 10, 10
        d[i].crop_x, d[i].crop_y, d[i].crop_w, d[i].crop_h = 1, 2, 8, 7
        d[i].canvas_w, d[i].canvas_h, d[i].paste_x, d[i].paste_y, d[i].flip = 12, 9, 4, 2, 1
        for k in range(12):
            d[i].color[k] = float(k % 5 == 0)
    return d


def _call(N, d, B=2, pixels=0x1000, nbytes=600, H=8, W=8, mean=True, std=True, y=0x2000, dtype=0, ws=0x3000, ws_bytes=None):
    f3 = ctypes.c_float * 3
    if ws_bytes is None:
        ws_bytes = int(N.lib.ssdk_augment_workspace_bytes(B))
    return N.lib.ssdk_augment(pixels, nbytes, d, B, H, W, f3(0, 0, 0) if mean else None, f3(1, 1, 1) if std else None, y, dtype, ws,
                              ws_bytes, None)


def test_cabi_descriptor_size():
    """ssdk_augment_desc_bytes() == the ctypes mirror == the numpy record == sizeof as gcc sees the header (compiled as C)."""
    from ssds import _native as N
    from ssds.dataset import augment as A

    size = int(N.lib.ssdk_augment_desc_bytes())
    assert size == ctypes.sizeof(N.AugmentDesc) == A.DESC_DTYPE.itemsize
    for (name, _), f in zip(N.AugmentDesc._fields_, A.DESC_DTYPE.names):
        assert name == f and getattr(N.AugmentDesc, name).offset == A.DESC_DTYPE.fields[f][1]
    src = '#include <stdio.h>\n#include "ssdk.h"\nint main(void){printf("%zu\\n", sizeof(ssdk_augment_desc)); return 0;}\n'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(src)
        subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), os.path.join(d, "s.c"), "-o", os.path.join(d, "s")], check=True)
        assert int(subprocess.run([os.path.join(d, "s")], check=True, capture_output=True, text=True).stdout) == size
    assert N.lib.ssdk_augment_workspace_bytes(64) >= 64 * size and N.lib.ssdk_augment_workspace_bytes(0) == 0
    assert N.lib.ssdk_version() == 245 and N.lib.ssdk_struct_size(8) == 0


@pytest.mark.parametrize("case, word", [
    ("pixels", "null"), ("descs", "null"), ("mean", "null"), ("std", "null"), ("y", "null"), ("workspace", "null"),
    ("past_end", "pixels_bytes"), ("negative_offset", "src_offset"), ("crop_x", "crop"), ("crop_h", "crop"), ("crop_zero", "crop_w"),
    ("paste_x", "paste"), ("paste_y", "paste"), ("canvas_small", "canvas"), ("flip", "flip"), ("nan_color", "color"),
    ("src_zero", "src_h"), ("B0", "B ="), ("H0", "H ="), ("short_ws", "workspace_bytes"), ("dtype_u8", "dst_dtype"), ("dtype_9", "dst_dtype")])
def test_cabi_bad_arguments(case, word):
    """Every bad argument is SSDK_E_BADARG with a message naming the field; the pointers handed over are not addresses of
    anything, so a library that launched (or copied) before checking would not return an error code at all."""
    from ssds import _native as N

    d = _good(N)
    kw = {}
    if case in ("pixels", "y"):
        kw[case] = None
    elif case == "workspace":
        kw["ws"] = None
    elif case in ("mean", "std"):
        kw[case] = False
    elif case == "descs":
        d = None
    elif case == "past_end":
        kw["nbytes"] = 599  # the second image ends at byte 600
    elif case == "negative_offset":
        d[0].src_offset = -1
    elif case == "crop_x":
        d[1].crop_x = 3  # 3 + 8 > 10
    elif case == "crop_h":
        d[1].crop_h = 9  # 2 + 9 > 10
    elif case == "crop_zero":
        d[0].crop_w = 0
    elif case == "paste_x":
        d[1].paste_x = 5  # 5 + 8 > 12
    elif case == "paste_y":
        d[0].paste_y = -1
    elif case == "canvas_small":
        d[0].canvas_h = 0
    elif case == "flip":
        d[0].flip = 2
    elif case == "nan_color":
        d[1].color[7] = float("nan")
    elif case == "src_zero":
        d[0].src_h = 0
    elif case == "B0":
        kw.update(B=0, ws_bytes=4096)
    elif case == "H0":
        kw["H"] = 0
    elif case == "short_ws":
        kw["ws_bytes"] = int(N.lib.ssdk_augment_workspace_bytes(2)) - 1
    elif case == "dtype_u8":
        kw["dtype"] = N.U8
    elif case == "dtype_9":
        kw["dtype"] = 9
    assert _call(N, d, **kw) == -1
    msg = N.lib.ssdk_last_error().decode()
    assert msg.startswith("augment:") and word in msg, msg


# ---- dataset plumbing -------------------------------------------------------------------------------------------------------
def test_pack_tool_and_source_round_trip(tmp_path):
    from ssds.dataset import augment as A

    out = str(tmp_path / "toy")
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "pack_dataset.py"), "--synthetic", "37", "--seed", "3", "--out", out,
                    "--per-shard", "16"], check=True, env=dict(os.environ, PYTHONNOUSERSITE="1"))
    assert sorted(os.listdir(out)) == ["shard_00000.npz", "shard_00001.npz", "shard_00002.npz"]
    src = A.PackedDetectionSource(out)
    images, boxes = _pack_tool().synthetic_set(37, seed=3)
    assert len(src) == 37
    sizes = set()
    for i in range(37):
        np.testing.assert_array_equal(src.image(i), images[i])
        np.testing.assert_array_equal(src.boxes(i), boxes[i])
        assert src.pixels(i).dtype == np.uint8 and src.pixels(i).size == images[i].size
        sizes.add(src.shape(i))
        b = src.boxes(i)
        assert (b[:, 0] >= 0).all() and (b[:, 2] <= images[i].shape[1]).all() and (b[:, 3] <= images[i].shape[0]).all()
    assert len(sizes) > 10, "the toy set mixes image sizes"
    with pytest.raises(FileNotFoundError):
        A.PackedDetectionSource(str(tmp_path / "nothing"))
    np.savez(str(tmp_path / "bad.npz"), pixels=np.zeros(10, np.uint8), offsets=[0], shapes=[[2, 2]], boxes=np.zeros((0, 5)), box_offsets=[0, 0])
    with pytest.raises(ValueError):  # 2 x 2 x 3 bytes do not fit into 10
        A.PackedDetectionSource(str(tmp_path))


def test_batches_shard_over_ranks(tmp_path):
    """Two ranks: no image twice, eval covers the set exactly, training leaves fewer than world * batch images out, another
    epoch another order; the loader's host half needs no device."""
    from ssds.dataset import augment as A

    n, bs = 203, 8
    for training in (False, True):
        seen = [np.concatenate(A.epoch_batches(n, bs, r, 2, training, 7, 0)) for r in (0, 1)]
        both = np.concatenate(seen)
        assert len(np.unique(both)) == len(both)
        if training:
            assert len(seen[0]) == len(seen[1]) == 96 and n - len(both) < 2 * bs
            assert all(len(b) == bs for r in (0, 1) for b in A.epoch_batches(n, bs, r, 2, True, 7, 0))
            other = np.concatenate(A.epoch_batches(n, bs, 0, 2, True, 7, 1))
            assert not np.array_equal(other, seen[0])
            np.testing.assert_array_equal(np.concatenate(A.epoch_batches(n, bs, 0, 2, True, 7, 0)), seen[0])
        else:
            assert sorted(both.tolist()) == list(range(n))
    pk = _pack_tool()
    images, boxes = pk.synthetic_set(20, seed=1)
    pk.write_shards(str(tmp_path), images, boxes, per_shard=8)
    src = A.PackedDetectionSource(str(tmp_path))
    cfg = {"IMAGE_SIZE": [64, 96], "PREPROC": PREPROC}
    loaders = [A.AugmentedLoader(src, cfg, 4, "cpu", training=True, seed=3, rank=r, world_size=2, max_gt=8) for r in (0, 1)]
    assert len(loaders[0]) == len(loaders[1]) == 2
    d0, t0, _, nbytes = loaders[0].describe(0, 0, loaders[0].batches(0)[0])
    d1, t1, _, _ = loaders[1].describe(0, 0, loaders[1].batches(0)[0])
    assert t0.shape == t1.shape == (4, 8, 5) and d0.tobytes() != d1.tobytes()
    idx = loaders[0].batches(0)[0]
    assert nbytes == sum(src.pixels(int(i)).size for i in idx) and d0["src_offset"][0] == 0
    assert (np.diff(d0["src_offset"]) == [src.pixels(int(i)).size for i in idx[:-1]]).all()
    with pytest.raises(ValueError):
        A.AugmentedLoader(src, cfg, 64, "cpu", training=True)


def test_train_ddp_selects_the_loader():
    """--data / DATASET.DATASET == 'packed' choose the packed loader; every shipped config says 'synthetic' and sets no directory."""
    import glob

    from ssds.core import config
    from ssds.utils import train_ddp

    for f in sorted(glob.glob(os.path.join(ROOT, "experiments", "cfgs", "*.yml"))):
        cfg = config.cfg_from_file(f)
        assert cfg.DATASET.DATASET == "synthetic" and cfg.DATASET.DATASET_DIR == ""
        assert train_ddp.data_dir(cfg, None) is None
        assert train_ddp.data_dir(cfg, "/some/dir") == "/some/dir"
    cfg.DATASET.DATASET, cfg.DATASET.DATASET_DIR = "packed", "/data/toy"
    try:
        assert train_ddp.data_dir(cfg, None) == "/data/toy"
        cfg.DATASET.DATASET_DIR = ""
        with pytest.raises(ValueError):
            train_ddp.data_dir(cfg, None)
    finally:
        cfg.DATASET.DATASET, cfg.DATASET.DATASET_DIR = "synthetic", ""
