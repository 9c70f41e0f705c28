"""The COCO summary without a device: the oracle (tests/cocoeval_oracle.py) on hand-worked cases, the conditions of its seeded
generator, the shard arrays ``box_crowd`` / ``box_area``, the loader's ``eval_extras`` and the header of the new entry points."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "ssds.pytorch_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import cocoeval_oracle as CO  # noqa: E402

F32 = np.float32
IGN = 1 << 16  # the ignored bit of threshold 0


def _one(dets, gts, crowd=None, ranges=CO.ALL_AREAS, thr=(0.5,), max_dets=(100,), C=1, **kw):
    """One image: dets = [(score, l, t, r, b, class)], gts = [(l, t, r, b, class)] -> (flags [D, A], npig, ap, recall, counters)."""
    d = np.array(dets, F32).reshape(1, -1, 6)
    det = (d[:, :, 0], d[:, :, 1:5], d[:, :, 5])
    tg = np.array(gts, F32).reshape(1, -1, 5)
    counters = CO.new_counters()
    cr = None if crowd is None else np.array([crowd], np.int32)
    cls, rank, flags, npig = CO.evaluate(det, tg, C, 0.01, np.array(thr, F32), ranges, crowd=cr, counters=counters, **kw)
    ap, recall = CO.accumulate(cls, det[0], rank, flags, npig, C, len(thr), max_dets)
    return flags[0], npig, ap, recall, counters


def test_a_crowd_box_is_taken_twice_and_its_detections_are_ignored():
    """K = [0,0,100,100] is a crowd region, A = [200,200,220,220] an ordinary box.  d1 = [10,10,30,30] (0.9) and d2 = [40,40,60,60]
    (0.8) lie inside K: intersection / detection area = 400 / 400 = 1 >= 0.5, so both take K (the second time it is already
    taken) and inherit its ignore flag: matched | ignored.  d3 = A (0.7) is the only record that counts: npig = 1 (K is ignored),
    precision 1 at recall 1: AP = recall = 1.
    Without the crowd flag the IoU of d1 and d2 with K is 400 / 10000 = 0.04: two false positives before the true positive d3,
    npig = 2: precision 1/3 from recall 0 to 0.5, 0 beyond: AP = 51 * (1/3) / 101 = 17/101, recall 1/2."""
    dets = [(0.9, 10, 10, 30, 30, 0), (0.8, 40, 40, 60, 60, 0), (0.7, 200, 200, 220, 220, 0)]
    gts = [(0, 0, 100, 100, 0), (200, 200, 220, 220, 0)]
    flags, npig, ap, recall, counters = _one(dets, gts, crowd=[1, 0])
    assert flags[:, 0].tolist() == [1 | IGN, 1 | IGN, 1] and npig.tolist() == [[1]]
    assert counters["crowd_retake"] == 1
    assert ap[0, 0, 0, 0] == pytest.approx(1.0, abs=1e-12) and recall[0, 0, 0, 0] == 1.0
    flags, npig, ap, recall, counters = _one(dets, gts)
    assert flags[:, 0].tolist() == [0, 0, 1] and npig.tolist() == [[2]] and counters["crowd_retake"] == 0
    assert ap[0, 0, 0, 0] == pytest.approx(17.0 / 101.0, abs=1e-12) and recall[0, 0, 0, 0] == 0.5


def test_a_detection_prefers_a_non_ignored_box_of_lower_iou_and_an_out_of_range_box_absorbs_the_next():
    """A = [0,0,30,30] (area 900: small), Bb = [0,0,30,36] (area 1080 > 32^2: ignored under "small").  d1 = [0,0,30,35] (0.9): IoU
    900 / 1050 = 0.857 with A, 1050 / 1080 = 0.972 with Bb; d2 = [0,0,30,36] (0.8): 0.833 with A, 1 with Bb.
    "all": d1 takes Bb (the higher IoU), d2 finds A free: two true positives, flags [1, 1].
    "small": the boxes are ordered A, Bb.  d1 takes A and STOPS at Bb (the break: it holds a non-ignored match); d2 skips A (taken)
    and takes Bb, whose ignore flag it inherits: flags [1, 1 | IGN] -- the out-of-range box absorbed d2, which is no false positive.
    npig: 2 under "all", 1 under "small"; AP = recall = 1 under both."""
    dets = [(0.9, 0, 0, 30, 35, 0), (0.8, 0, 0, 30, 36, 0)]
    gts = [(0, 0, 30, 30, 0), (0, 0, 30, 36, 0)]
    flags, npig, ap, recall, counters = _one(dets, gts, ranges=CO.COCO_AREAS[:2])
    assert flags.tolist() == [[1, 1], [1, 1 | IGN]] and npig.tolist() == [[2], [1]]
    assert counters["break"] == 1 and counters["ignored_absorption"] == 1
    np.testing.assert_allclose(ap[:, 0, 0, 0], [1.0, 1.0], rtol=0, atol=1e-12)
    assert recall[:, 0, 0, 0].tolist() == [1.0, 1.0]


def test_an_unmatched_small_detection_is_ignored_under_large_and_a_false_positive_under_all():
    """L = [0,0,100,100] (large).  d1 = [200,200,210,210] (0.95, area 100, overlaps nothing), d2 = L (0.9).
    "all": d1 is a false positive before the true positive: precision 1/2 at recall 1: AP = 1/2.
    "large": d1's area is < 96^2 and it is unmatched: ignored (flags IGN); only d2 counts: AP = 1."""
    dets = [(0.95, 200, 200, 210, 210, 0), (0.9, 0, 0, 100, 100, 0)]
    flags, npig, ap, recall, counters = _one(dets, [(0, 0, 100, 100, 0)], ranges=CO.COCO_AREAS[[0, 3]])
    assert flags.tolist() == [[0, IGN], [1, 1]] and npig.tolist() == [[1], [1]] and counters["unmatched_out_of_range"] == 1
    np.testing.assert_allclose(ap[:, 0, 0, 0], [0.5, 1.0], rtol=0, atol=1e-12)
    assert recall[:, 0, 0, 0].tolist() == [1.0, 1.0]


def test_ar1_against_ar10_with_two_detections_of_a_class_in_one_image():
    """Two disjoint boxes of one class, each found exactly.  maxDets = 1 keeps rank 0 per image and category: one true positive,
    recall 1/2, precision 1 up to recall 0.5: AP = 51/101.  maxDets = 10 keeps both: recall 1, AP 1.  The second class has one
    box and one detection: its rank is 0 again (the cut is per category), recall 1 at both."""
    dets = [(0.9, 0, 0, 10, 10, 0), (0.8, 20, 20, 30, 30, 0), (0.7, 50, 50, 60, 60, 1)]
    gts = [(0, 0, 10, 10, 0), (20, 20, 30, 30, 0), (50, 50, 60, 60, 1)]
    flags, npig, ap, recall, _ = _one(dets, gts, max_dets=(1, 10), C=2)
    assert flags[:, 0].tolist() == [1, 1, 1] and npig.tolist() == [[2, 1]]
    assert recall[0, :, 0, :].tolist() == [[0.5, 1.0], [1.0, 1.0]]
    np.testing.assert_allclose(ap[0, :, 0, :], [[51.0 / 101.0, 1.0], [1.0, 1.0]], rtol=0, atol=1e-12)
    s = CO.summarize(np.repeat(ap, 4, 0)[:, [0, 1, 1]], np.repeat(recall, 4, 0)[:, [0, 1, 1]], [0.5])
    assert list(s) == ["AP", "AP50", "AP75", "APs", "APm", "APl", "AR1", "AR10", "AR100", "ARs", "ARm", "ARl"]
    assert s["AR1"] == 0.75 and s["AR10"] == 1.0 and s["AP50"] == pytest.approx(1.0) and np.isnan(s["AP75"])


def test_area_scale_moves_a_box_across_the_boundaries_and_a_supplied_area_wins():
    """A 40 x 40 box (1600 network pixels: medium).  area_scale 0.25 -> 400 (small), 4 -> 6400 (medium), 8 -> 12800 (large); a
    supplied area of 500 makes it small whatever the scale."""
    box = [(0, 0, 40, 40, 0)]
    for scale, want in ((0.25, [1, 1, 0, 0]), (4.0, [1, 0, 1, 0]), (8.0, [1, 0, 0, 1])):
        _, npig, _, _, _ = _one([(0.9, 0, 0, 40, 40, 0)], box, ranges=CO.COCO_AREAS, area_scale=[scale])
        assert npig[:, 0].tolist() == want
    _, npig, _, _, _ = _one([(0.9, 0, 0, 40, 40, 0)], box, ranges=CO.COCO_AREAS, area_scale=[8.0], area=np.array([[500.0]], F32))
    assert npig[:, 0].tolist() == [1, 1, 0, 0]


def test_without_crowd_and_ranges_the_oracle_is_the_sweep_oracle():
    import apsweep_oracle as AO

    case = AO.make_case(5, 3, 60, 8, 4, AO.COCO_IOUS, clustered=True)[0]
    det, tg = case
    cls, mask, npos = AO.match(det, tg, 4, 0.06, AO.COCO_IOUS, "coco", 100)
    c2, rank, flags, npig = CO.evaluate(det, tg, 4, 0.06, AO.COCO_IOUS, CO.ALL_AREAS)
    np.testing.assert_array_equal(cls, c2)
    np.testing.assert_array_equal(flags[:, :, 0], mask)
    np.testing.assert_array_equal(npig[0], npos)
    assert int(np.count_nonzero(mask)) > 10


def test_the_generator_keeps_its_conditions_and_reaches_every_branch():
    cases = CO.make_case(3, 4, 60, 10, 4, CO.COCO_IOUS, batches=1, with_area=True, area_scale=[1.0, 0.25, 4.0])
    cond = CO.conditions(cases, CO.COCO_IOUS)
    assert cond["iou_margin"] >= CO.MARGIN and cond["distinct_scores"] and cond["area_margin"] >= CO.AREA_MARGIN
    assert cond["min_det_area"] > 0
    o = CO.Summary(4, 0.06)
    for c in cases:
        o(c["detections"], c["targets"], c["crowd"], c["area"], c["area_scale"])
    assert all(v >= 5 for v in o.counters.values()), o.counters
    AP, detail = o.get_results()
    assert 0.0 < AP < 1.0 and not any(np.isnan(v) for v in detail["summary"].values())


# ---- shards, loader, header ---------------------------------------------------------------------------------------------------
def _toy(n=5):
    from tools.pack_dataset import synthetic_set

    images, boxes = synthetic_set(n, seed=2, height=(40, 60), width=(50, 70), max_boxes=4, num_classes=3)
    rs = np.random.RandomState(0)
    crowd = [rs.randint(0, 2, len(b)).astype(np.int32) for b in boxes]
    area = [((b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1]) * rs.uniform(0.5, 1.0, len(b))).astype(F32) for b in boxes]
    return images, boxes, crowd, area


def test_shards_round_trip_with_and_without_crowd_and_area(tmp_path):
    from ssds.dataset.augment import PackedDetectionSource
    from tools.pack_dataset import write_shards

    images, boxes, crowd, area = _toy()
    assert sum(len(b) for b in boxes) > 4
    write_shards(str(tmp_path / "plain"), images, boxes, per_shard=2)
    write_shards(str(tmp_path / "extra"), images, boxes, per_shard=2, crowd=crowd, area=area)
    plain, extra = PackedDetectionSource(str(tmp_path / "plain")), PackedDetectionSource(str(tmp_path / "extra"))
    with np.load(str(tmp_path / "plain" / "shard_00000.npz")) as z:
        assert sorted(z.files) == sorted(PackedDetectionSource.KEYS)  # what a shard always held, nothing more
    with np.load(str(tmp_path / "extra" / "shard_00000.npz")) as z:
        assert sorted(z.files) == sorted(PackedDetectionSource.KEYS + ("box_crowd", "box_area"))
    assert len(plain) == len(extra) == len(images)
    for i in range(len(images)):
        np.testing.assert_array_equal(plain.boxes(i), boxes[i])
        np.testing.assert_array_equal(extra.boxes(i), boxes[i])
        np.testing.assert_array_equal(extra.image(i), images[i])
        np.testing.assert_array_equal(extra.crowd(i), crowd[i])
        np.testing.assert_array_equal(extra.area(i), area[i])
        assert plain.crowd(i) is None and plain.area(i) is None
    with pytest.raises(ValueError):
        write_shards(str(tmp_path / "bad"), images, boxes, crowd=crowd[:-1])
    with pytest.raises(ValueError):
        write_shards(str(tmp_path / "bad"), images, boxes, area=[a[:-1] if len(a) else np.ones(1, F32) for a in area])


_DATASET = {"IMAGE_SIZE": [32, 48], "PREPROC": {"MEAN": [123.0, 117.0, 104.0], "STD": [58.0, 57.0, 57.0]}}


def test_eval_extras_describe_the_rows_of_the_targets(tmp_path):
    """(no device: the host half of a batch)  crowd and area follow the rows of ``targets`` -- also when max_gt keeps only the
    largest boxes -- area falls back to the source box area, padding rows are 0, and area_scale = (Ws / W) * (Hs / H)."""
    from ssds.dataset.augment import AugmentedLoader, PackedDetectionSource
    from tools.pack_dataset import write_shards

    images, boxes, crowd, area = _toy()
    write_shards(str(tmp_path / "plain"), images, boxes)
    write_shards(str(tmp_path / "extra"), images, boxes, crowd=crowd, area=area)
    for name, max_gt in (("extra", None), ("extra", 2), ("plain", None)):
        src = PackedDetectionSource(str(tmp_path / name))
        ld = AugmentedLoader(src, _DATASET, 5, None, training=False, eval_extras=True, max_gt=max_gt)
        idx = ld.batches(0)[0]
        descs, targets, info, _ = ld.describe(0, 0, idx)
        ex = ld.extras(idx, targets, info)
        G = targets.shape[1]
        assert ex["crowd"].shape == (5, G) and ex["area"].shape == (5, G) and ex["area_scale"].shape == (5,)
        assert ex["crowd"].dtype == np.int32 and ex["area"].dtype == F32 and ex["area_scale"].dtype == F32
        for b, i in enumerate(idx):
            h, w = src.shape(int(i))
            assert ex["area_scale"][b] == F32((w / 48.0) * (h / 32.0))
            rows = info["rows"][b]
            assert len(rows) == min(len(boxes[i]), G if max_gt else len(boxes[i]))
            bi = boxes[i][rows]
            np.testing.assert_allclose(targets[b, :len(rows), 2] * (w / 48.0), bi[:, 2] - bi[:, 0], rtol=1e-5)  # the rows ARE these boxes
            want_area = area[i][rows] if name == "extra" else ((bi[:, 2] - bi[:, 0]) * (bi[:, 3] - bi[:, 1])).astype(F32)
            np.testing.assert_array_equal(ex["area"][b, :len(rows)], want_area)
            np.testing.assert_array_equal(ex["crowd"][b, :len(rows)], crowd[i][rows] if name == "extra" else 0)
            assert (ex["crowd"][b, len(rows):] == 0).all() and (ex["area"][b, len(rows):] == 0).all()
            assert (targets[b, len(rows):, 4] == -1).all()
    assert AugmentedLoader(src, _DATASET, 5, None, training=False).eval_extras is False
    with pytest.raises(ValueError):
        AugmentedLoader(src, _DATASET, 5, None, training=True, eval_extras=True)


def test_the_header_of_the_coco_summary_parses_into_the_binding():
    from ssds import _native as N

    assert N.COCOEVAL_HEADER_PATH.endswith("ssdk_cocoeval.h")
    h = N.parse_header(open(N.COCOEVAL_HEADER_PATH).read())
    assert tuple(h.functions) == ("ssdk_cocoeval_match", "ssdk_cocoeval_accumulate") == N.COCOEVAL_EXPORTS and not h.structs
    assert (N.COCOEVAL_MAX_T, N.COCOEVAL_MAX_A, N.COCOEVAL_MAX_M) == (16, 4, 4)
    for name in N.COCOEVAL_EXPORTS:
        assert getattr(N.lib, name).argtypes == N._ABI.functions[name][1]
    assert len(N._ABI.functions["ssdk_cocoeval_match"][1]) == 21 and len(N._ABI.functions["ssdk_cocoeval_accumulate"][1]) == 12
    assert N.ABI_VERSION == 245  # the closed list of ssdk.h is untouched


def test_argument_errors_come_before_any_device_call():
    """(no device needed: every check precedes the launch)"""
    import ctypes

    from ssds import _native as N

    thr, rng, md = (ctypes.c_float * 2)(0.5, 0.75), (ctypes.c_float * 2)(0.0, 1e10), (ctypes.c_int * 2)(1, 10)
    p = ctypes.c_void_p(64)  # never dereferenced
    ok = dict(T=2, A=1, D=10, G=4, thr=thr, rng=rng)

    def match(**kw):
        a = dict(ok, **kw)
        return N.lib.ssdk_cocoeval_match(p, p, p, 1, a["D"], p, a["G"], None, None, None, 3, 0.05, a["thr"], a["T"], a["rng"], a["A"],
                                         p, p, p, p, None)

    bad_thr, bad_rng = (ctypes.c_float * 2)(0.75, 0.5), (ctypes.c_float * 2)(10.0, 1.0)
    for kw in (dict(T=0), dict(T=17), dict(A=0), dict(A=5), dict(D=2049), dict(G=N.MAX_GT + 1), dict(thr=bad_thr), dict(rng=bad_rng),
               dict(thr=None), dict(rng=None)):
        assert match(**kw) != 0, kw
        assert "cocoeval_match" in N.lib.ssdk_last_error().decode()

    def acc(T=2, A=1, M=2, md=md):
        return N.lib.ssdk_cocoeval_accumulate(p, p, p, p, 3, T, A, md, M, p, p, None)

    for kw in (dict(T=0), dict(A=5), dict(M=0), dict(M=5), dict(md=(ctypes.c_int * 2)(10, 1)), dict(md=(ctypes.c_int * 2)(0, 1)), dict(md=None)):
        assert acc(**kw) != 0, kw
        assert "cocoeval_accumulate" in N.lib.ssdk_last_error().decode()
