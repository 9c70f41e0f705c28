"""The COCO summary on the device (csrc/ssdk_cocoeval.hip, ssds.core.evaluation_metrics.CocoSummary) and the eval phase built on it.

1. ``ssdk_cocoeval_match`` / ``ssdk_cocoeval_accumulate`` against tests/cocoeval_oracle.py on seeded inputs that keep every IoU 1e-4
   from every threshold, every area a relative 1e-4 from 32^2 and 96^2 and have distinct scores (all asserted): keys, rank, flags
   and npig bit for bit, ap and recall within 1e-12 (the oracle has pycocotools' np.spacing(1) in the precision denominator: a
   relative 3e-16);
2. the seeded set reaches every branch of the rule (the oracle's counters) and every area range;
3. the anchor to tested code: without crowd, one range and maxDets 100 the flags are the masks of ``ssdk_apsweep_match`` (COCO rule)
   and ap the bits of ``ssdk_apsweep_average_precision``;
4. the same bits over two calls, two halves of a batch against the whole, guard bands around every buffer;
5. ``CocoSummary`` on ``Decoder`` outputs against the oracle, two ranks on one GPU against one process, ``Solver.eval_model`` on a
   directory of shards."""
import ctypes
import functools
import json
import os
import socket
import subprocess
import sys
from collections import OrderedDict

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "ssds.pytorch_amd"), os.path.join(ROOT, "tests")):  # (a rank of the two-rank test starts this file)
    if _p not in sys.path:
        sys.path.insert(0, _p)

import apsweep_oracle as AO  # noqa: E402
import cocoeval_oracle as CO  # noqa: E402
import guardband as G  # noqa: E402

F32 = np.float32
CONF = 0.06


def _dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _carr(ctype, v):
    v = [x for x in np.asarray(v).reshape(-1).tolist()]
    return (ctype * len(v))(*v)


def _ptr(t):
    return None if t is None else (t.data_ptr() if t.numel() else torch.empty(8, device="cuda").data_ptr())  # (G = 0: a pointer, never read)


def _match(det, targets, crowd, area, scale, C, thr, ranges, out=None, conf=CONF):
    """One raw ssdk_cocoeval_match on device tensors -> (keys [B, D], rank [B, D], flags [B, D, A], npig [A, C])."""
    from ssds import _native as N

    scores, boxes, classes = det
    B, D = scores.shape
    A = len(np.asarray(ranges).reshape(-1, 2))
    if out is None:
        out = (torch.empty((B, D), device="cuda", dtype=torch.int64), torch.empty((B, D), device="cuda", dtype=torch.int32),
               torch.empty((B, D, A), device="cuda", dtype=torch.int32), torch.zeros((A, C), device="cuda", dtype=torch.int32))
    keys, rank, flags, npig = out
    Gt = int(targets.shape[1])
    N.check(N.lib.ssdk_cocoeval_match(scores.data_ptr(), boxes.data_ptr(), classes.data_ptr(), B, D, _ptr(targets), Gt,
                                      _ptr(crowd) if Gt else None, _ptr(area) if Gt else None, _ptr(scale), C, conf,
                                      _carr(ctypes.c_float, thr), len(thr), _carr(ctypes.c_float, ranges), A, keys.data_ptr(),
                                      rank.data_ptr(), flags.data_ptr(), npig.data_ptr(), N.stream_ptr(scores.device)), "cocoeval_match")
    return keys, rank, flags, npig


def _sorted(keys, rank, flags, C):
    skeys, order = torch.sort(keys.reshape(-1), stable=True)
    seg = torch.searchsorted(skeys, torch.arange(C + 1, device="cuda", dtype=torch.int64) << 32).contiguous()
    return flags.reshape(-1, flags.shape[-1])[order].contiguous(), rank.reshape(-1)[order].contiguous(), seg


def _accumulate(flags_s, rank_s, seg, npig, C, T, max_dets, out=None):
    from ssds import _native as N

    A, M = int(npig.shape[0]), len(max_dets)
    ap, recall = out if out is not None else (torch.empty((A, M, T, C), device="cuda", dtype=torch.float64),
                                              torch.empty((A, M, T, C), device="cuda", dtype=torch.float64))
    N.check(N.lib.ssdk_cocoeval_accumulate(flags_s.data_ptr(), rank_s.data_ptr(), seg.data_ptr(), npig.data_ptr(), C, T, A,
                                           _carr(ctypes.c_int, max_dets), M, ap.data_ptr(), recall.data_ptr(),
                                           N.stream_ptr(npig.device)), "cocoeval_accumulate")
    return ap, recall


def _case_dev(case):
    return (tuple(_dev(x) for x in case["detections"]), _dev(case["targets"]), _dev(case["crowd"]), _dev(case["area"]),
            _dev(case["area_scale"]))


# ---- 1. against the oracle ------------------------------------------------------------------------------------------------------
CASES = OrderedDict((
    # name: (seed, B, D, G, C, thresholds, batches, generator options)
    ("base", (21, 6, 100, 12, 5, CO.COCO_IOUS, 2, dict())),
    ("sixteen_thresholds", (22, 6, 100, 12, 5, CO.SWEEP16, 1, dict(clustered=True))),
    # the capacity corners: every slot of an image, every box row, 85 boxes and ~680 detections of a class (several chunks of both)
    ("capacity", (23, 1, 2048, 256, 3, CO.COCO_IOUS, 1, dict(full=True))),
    ("one_slot", (24, 5, 1, 4, 2, CO.COCO_IOUS, 1, dict(full=True))),
    ("no_boxes", (25, 3, 20, 0, 3, CO.COCO_IOUS, 1, dict(crowd=0.0))),
    ("an_image_of_crowd_boxes_only", (26, 3, 40, 6, 2, CO.COCO_IOUS, 1, dict(all_crowd_image=1, full=True))),
    ("a_class_without_ground_truth", (27, 4, 60, 8, 4, CO.COCO_IOUS, 1, dict(no_gt_class=2))),
    ("area_scale", (28, 6, 60, 10, 3, CO.COCO_IOUS, 1, dict(area_scale=[0.25, 4.0, 1.0], full=True))),
    ("supplied_area", (29, 4, 60, 10, 3, CO.COCO_IOUS, 1, dict(with_area=True, area_scale=[4.0, 0.25], empty_image=2))),
))
MAX_DETS = (1, 10, 100)


@functools.lru_cache(maxsize=None)
def _case(name):
    seed, B, D, Gt, C, thr, batches, opts = CASES[name]
    return CO.make_case(seed, B, D, Gt, C, thr, batches=batches, **opts)


@functools.lru_cache(maxsize=None)
def _oracle(name):
    """Computed once per case, shared and left unchanged: (the oracle, [(cls, rank, flags)] per batch, (ap, recall))."""
    seed, B, D, Gt, C, thr, batches, opts = CASES[name]
    o = CO.Summary(C, CONF, thr, CO.COCO_AREAS, MAX_DETS)
    per_batch = []
    for c in _case(name):
        cls, rank, flags, _ = o(c["detections"], c["targets"], c["crowd"], c["area"], c["area_scale"])
        per_batch.append((cls, rank, flags))
    return o, per_batch, o.arrays()


def _assert_conditions(name):
    seed, B, D, Gt, C, thr, batches, opts = CASES[name]
    cond = CO.conditions(_case(name), thr)
    assert cond["iou_margin"] >= CO.MARGIN, "the generator must keep every IoU away from the thresholds"
    assert cond["distinct_scores"], "the generator must give distinct scores"
    assert cond["area_margin"] >= CO.AREA_MARGIN, "the generator must keep every area away from 32^2 and 96^2"
    assert cond["min_det_area"] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_match_and_accumulate_against_the_oracle(name):
    seed, B, D, Gt, C, thr, batches, opts = CASES[name]
    _assert_conditions(name)
    o, per_batch, (want_ap, want_recall) = _oracle(name)
    npig = torch.zeros((4, C), device="cuda", dtype=torch.int32)
    got = []
    for case, (want_cls, want_rank, want_flags) in zip(_case(name), per_batch):
        det, tg, crowd, area, scale = _case_dev(case)
        A = 4
        out = (torch.empty((B, D), device="cuda", dtype=torch.int64), torch.empty((B, D), device="cuda", dtype=torch.int32),
               torch.empty((B, D, A), device="cuda", dtype=torch.int32), npig)
        keys, rank, flags, _ = _match(det, tg, crowd, area, scale, C, thr, CO.COCO_AREAS, out=out)
        cls, score = AO.decode_keys(keys.cpu().numpy())
        np.testing.assert_array_equal(cls, want_cls)
        np.testing.assert_array_equal(score, case["detections"][0])
        np.testing.assert_array_equal(rank.cpu().numpy(), want_rank)
        np.testing.assert_array_equal(flags.cpu().numpy(), want_flags)
        got.append((keys, rank, flags))
    np.testing.assert_array_equal(npig.cpu().numpy(), o.npig)
    keys, rank, flags = (torch.cat([g[k].reshape(B * D, -1) for g in got]) for k in range(3))
    flags_s, rank_s, seg = _sorted(keys, rank, flags, C)
    ap, recall = _accumulate(flags_s, rank_s, seg, npig, C, len(thr), MAX_DETS)
    np.testing.assert_allclose(ap.cpu().numpy(), want_ap, rtol=0, atol=1e-12, equal_nan=True)
    np.testing.assert_allclose(recall.cpu().numpy(), want_recall, rtol=0, atol=1e-12, equal_nan=True)
    if Gt:
        assert int(np.count_nonzero(np.concatenate([w[2].ravel() for w in per_batch]) & 0xFFFF)) > 0
        assert np.nansum(want_ap) > 0
    else:
        assert np.isnan(want_ap).all() and np.isnan(want_recall).all()


# ---- 2. what the seeded cases reach (no device) -----------------------------------------------------------------------------------
def test_the_seeded_set_reaches_every_branch_and_every_area_range():
    o, per_batch, (ap, recall) = _oracle("base")
    assert all(v >= 5 for v in o.counters.values()), o.counters
    assert (o.npig.sum(1) > 0).all()  # a non-ignored box in every area range
    flags = np.concatenate([w[2].reshape(-1, 4) for w in per_batch]).view(np.uint32)
    tp = (flags & 0xFFFF) & ~(flags >> 16)
    assert (np.count_nonzero(tp, axis=0) > 0).all()  # ... and a true positive
    assert (np.concatenate([w[1].ravel() for w in per_batch]) >= 10).any()  # maxDets 10 cuts something
    assert recall[0, 0].tolist() != recall[0, 2].tolist()


def test_the_named_cases_are_what_they_are_named_for():
    c = _case("capacity")[0]
    assert c["detections"][0].shape == (1, 2048) and (c["detections"][0] > 0).all() and (c["targets"][0, :, 4] >= 0).all()
    assert (c["detections"][0] > CONF).sum() > 2000 and not (c["detections"][0][0, -1] > CONF)  # counted up to the last chunk, not all
    assert max((c["targets"][0, :, 4] == k).sum() for k in range(3)) > 64
    c = _case("an_image_of_crowd_boxes_only")[0]
    assert (c["crowd"][1] != 0).all() and (c["targets"][1, :, 4] >= 0).all()
    c = _case("a_class_without_ground_truth")[0]
    assert not (c["targets"][:, :, 4] == 2).any() and ((c["detections"][2] == 2) & (c["detections"][0] > CONF)).sum() > 5
    assert _case("no_boxes")[0]["targets"].shape == (3, 0, 5) and _case("one_slot")[0]["detections"][0].shape == (5, 1)
    # area_scale 0.25 and 4 move boxes across both boundaries: the range of a box under its image's scale differs from the range
    # of the same box at scale 1, in both directions over each boundary
    c = _case("area_scale")[0]
    bucket = lambda a: np.digitize(a, [32.0 ** 2, 96.0 ** 2])  # noqa: E731
    moves = set()
    for b in range(6):
        real = c["targets"][b, :, 4] >= 0
        plain, scaled = CO.box_area(c["targets"][b, real, :4], 1.0), CO.box_area(c["targets"][b, real, :4], c["area_scale"][b])
        moves |= set(zip(bucket(plain).tolist(), bucket(scaled).tolist()))
    assert {(1, 0), (2, 1), (0, 1), (1, 2)} <= moves, moves
    c = _case("supplied_area")[0]
    assert c["area"] is not None and (c["targets"][2, :, 4] < 0).all()


# ---- 3. the anchor to tested code -----------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("T", [10, 16])
def test_without_crowd_and_ranges_the_flags_and_ap_are_those_of_the_sweep_bit_for_bit(T):
    from ssds import _native as N

    thr = {10: AO.COCO_IOUS, 16: AO.SWEEP16}[T]
    B, D, Gt, C = 4, 100, 7, 5
    det, tg = AO.make_case(11, B, D, Gt, C, thr, clustered=True)[0]
    det, tg = tuple(_dev(x) for x in det), _dev(tg)
    keys0 = torch.empty((B, D), device="cuda", dtype=torch.int64)
    mask0 = torch.empty((B, D), device="cuda", dtype=torch.int32)
    npos0 = torch.zeros(C, device="cuda", dtype=torch.int32)
    N.check(N.lib.ssdk_apsweep_match(det[0].data_ptr(), det[1].data_ptr(), det[2].data_ptr(), B, D, tg.data_ptr(), Gt, C, CONF,
                                     _carr(ctypes.c_float, thr), T, N.AP_RULE["coco"], 100, keys0.data_ptr(), mask0.data_ptr(),
                                     npos0.data_ptr(), N.stream_ptr(keys0.device)), "apsweep_match")
    keys, rank, flags, npig = _match(det, tg, None, None, None, C, thr, CO.ALL_AREAS)
    assert torch.equal(keys, keys0) and torch.equal(npig[0], npos0)
    assert torch.equal(flags[:, :, 0] & 0xFFFF, mask0) and int((flags >> 16).abs().sum()) == 0 and int(mask0.sum()) > 0
    order = torch.sort(keys0.view(-1), stable=True)[1]
    seg = torch.searchsorted(keys0.view(-1)[order], torch.arange(C + 1, device="cuda", dtype=torch.int64) << 32).contiguous()
    ap0 = torch.empty((T, C), device="cuda", dtype=torch.float64)
    mask_s = mask0.view(-1)[order].contiguous()
    N.check(N.lib.ssdk_apsweep_average_precision(mask_s.data_ptr(), seg.data_ptr(), npos0.data_ptr(), C, T, N.AP_RULE["coco"],
                                                 ap0.data_ptr(), N.stream_ptr(keys0.device)), "apsweep_average_precision")
    flags_s, rank_s, seg2 = _sorted(keys, rank, flags, C)
    ap, recall = _accumulate(flags_s, rank_s, seg2, npig, C, T, (100,))
    assert torch.equal(seg, seg2) and G.same_bits(ap[0, 0], ap0) and float(torch.nansum(ap0)) > 0


# ---- 4. reproducibility, halves, guard bands --------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_two_calls_give_the_same_bits_and_two_halves_equal_the_whole():
    seed, B, D, Gt, C, thr, batches, opts = CASES["base"]
    case = _case("base")[0]
    det, tg, crowd, area, scale = _case_dev(case)
    runs = []
    for _ in range(2):
        keys, rank, flags, npig = _match(det, tg, crowd, area, scale, C, thr, CO.COCO_AREAS)
        runs.append((keys, rank, flags, npig) + _accumulate(*_sorted(keys, rank, flags, C), npig, C, len(thr), MAX_DETS))
    for a, b in zip(*runs):
        assert G.same_bits(a, b)
    h = B // 2
    npig = torch.zeros((4, C), device="cuda", dtype=torch.int32)
    parts = []
    for lo, hi in ((0, h), (h, B)):
        cut = lambda x: None if x is None else x[lo:hi].contiguous()  # noqa: E731
        parts.append(_match(tuple(cut(x) for x in det), cut(tg), cut(crowd), cut(area), cut(scale), C, thr, CO.COCO_AREAS,
                            out=(torch.empty((hi - lo, D), device="cuda", dtype=torch.int64),
                                 torch.empty((hi - lo, D), device="cuda", dtype=torch.int32),
                                 torch.empty((hi - lo, D, 4), device="cuda", dtype=torch.int32), npig)))
    for k in range(3):
        assert torch.equal(torch.cat([p[k] for p in parts]), runs[0][k])
    assert torch.equal(npig, runs[0][3]) and int(npig.sum()) > 0


@pytest.mark.gpu
def test_guard_bands_around_every_buffer_of_both_entry_points():
    seed, B, D, Gt, C, thr, batches, opts = CASES["supplied_area"]
    case = _case("supplied_area")[0]
    clean = _match(*_case_dev(case), C, thr, CO.COCO_AREAS)
    gs = G.GuardSet("cuda")
    g_det = tuple(gs.inp(n, torch.from_numpy(x)) for n, x in zip(("scores", "boxes", "classes"), case["detections"]))
    g_in = [gs.inp(n, torch.from_numpy(np.ascontiguousarray(case[n]))) for n in ("targets", "crowd", "area", "area_scale")]
    g_keys, g_rank = gs.out("keys", (B, D), torch.int64), gs.out("rank", (B, D), torch.int32)
    g_flags = gs.out("flags", (B, D, 4), torch.int32)
    g_npig = gs.zeros("npig", 4 * 4 * C).view(torch.int32).view(4, C)
    gs.arm()
    _match(g_det, *g_in, C, thr, CO.COCO_AREAS, out=(g_keys, g_rank, g_flags, g_npig))
    torch.cuda.synchronize()
    assert gs.problems() == []
    for got, want in zip((g_keys, g_rank, g_flags, g_npig), clean):  # every slot written
        assert torch.equal(got, want)

    T, M = len(thr), len(MAX_DETS)
    flags_s, rank_s, seg = _sorted(clean[0], clean[1], clean[2], C)
    clean_out = _accumulate(flags_s, rank_s, seg, clean[3], C, T, MAX_DETS)
    gs = G.GuardSet("cuda")
    g_f, g_r, g_seg, g_np = gs.inp("flags_sorted", flags_s), gs.inp("rank_sorted", rank_s), gs.inp("seg_offsets", seg), gs.inp("npig", clean[3])
    g_ap, g_rc = gs.out("ap", (4, M, T, C), torch.float64), gs.out("recall", (4, M, T, C), torch.float64)
    gs.arm()
    _accumulate(g_f, g_r, g_seg, g_np, C, T, MAX_DETS, out=(g_ap, g_rc))
    torch.cuda.synchronize()
    assert gs.problems() == [] and G.same_bits(g_ap, clean_out[0]) and G.same_bits(g_rc, clean_out[1])


# ---- 5. CocoSummary, two ranks, Solver.eval_model -----------------------------------------------------------------------------------
@pytest.mark.gpu
def test_coco_summary_on_seeded_batches_does_not_synchronise_and_equals_the_oracle():
    from ssds.core.evaluation_metrics import CocoSummary

    seed, B, D, Gt, C, thr, batches, opts = CASES["base"]
    o, _, _ = _oracle("base")
    want_AP, want = o.get_results()
    m = CocoSummary(C, CONF)
    devs = [_case_dev(c) for c in _case("base")]
    m(devs[0][0], devs[0][1], crowd=devs[0][2], area=devs[0][3], area_scale=devs[0][4])  # (the first call creates the counters)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        m(devs[1][0], devs[1][1], crowd=devs[1][2], area=devs[1][3], area_scale=devs[1][4])
    finally:
        torch.cuda.set_sync_debug_mode("default")
    AP, detail = m.get_results()
    assert list(detail["summary"]) == list(want["summary"]) == ["AP", "AP50", "AP75", "APs", "APm", "APl", "AR1", "AR10", "AR100",
                                                                "ARs", "ARm", "ARl"]
    for k, v in want["summary"].items():
        assert abs(detail["summary"][k] - v) <= 1e-12 and 0.0 < v < 1.0, k
    assert AP == detail["summary"]["AP"]
    np.testing.assert_allclose(detail["ap"], want["ap"], rtol=0, atol=1e-12, equal_nan=True)
    np.testing.assert_allclose(detail["recall"], want["recall"], rtol=0, atol=1e-12, equal_nan=True)
    empty = CocoSummary(C, CONF).get_results()
    assert np.isnan(empty[0]) and all(np.isnan(v) for v in empty[1]["summary"].values())


def _detector(seed=0):
    """The 128-pixel MobileNetV2 SSD of tests/test_gpu_apsweep.py."""
    from ssds.modeling import nets, ssds
    from ssds.modeling.layers import box
    from ssds.modeling.layers.decoder import Decoder

    torch.manual_seed(seed)
    o, e, h = ssds.SSD.add_extras([[5, 7, "Conv:S"], [96, 320, 64]], [6, 6, 6], 5)
    model = ssds.SSD(nets.MobileNetV2(outputs=o), e, h, 5)
    for mod in model.modules():  # the heads start at the focal prior (every score 0.01): spread them out
        if isinstance(mod, torch.nn.Conv2d) and mod.out_channels in (30, 24):
            torch.nn.init.normal_(mod.weight, std=1.0)
    anchors = OrderedDict((s, box.generate_anchors(s, [1, 2, 0.5], [2.0, 2.828])) for s in (16, 32, 64))
    return model.cuda().eval(), anchors, Decoder(0.005, 0.5, 50, 200, False, False)


def _images(n, seed=3):
    from ssds.dataset.synthetic import SyntheticDetectionLoader

    return SyntheticDetectionLoader(n, (128, 128), 5, steps=1, device=torch.device("cpu"), max_gt=6, seed=seed).batch()


def _extras(targets, lo, hi):
    """Seeded crowd flags, areas of 0.6 .. 1 of the box area and an area_scale per image for images lo .. hi of ``_images``."""
    rs = np.random.RandomState(7)
    n, g = targets.shape[0], targets.shape[1]
    crowd = (rs.random_sample((n, g)) < 0.25).astype(np.int32)
    scale = np.array([0.25, 1.0, 4.0], F32)[rs.randint(0, 3, n)]
    t = targets.numpy().astype(F32)
    area = (t[:, :, 2] * t[:, :, 3] * scale[:, None] * rs.uniform(0.6, 1.0, (n, g))).astype(F32)
    return dict(crowd=torch.from_numpy(crowd[lo:hi]), area=torch.from_numpy(area[lo:hi]), area_scale=torch.from_numpy(scale[lo:hi]))


RANK_SPLIT = ((0, 6), (6, 10))  # 10 images: rank 0 evaluates six (batches of 4 and 2), rank 1 four: unequal record counts


def _rank_batches(images, targets, lo, hi):
    return [(images[i:min(i + 4, hi)], targets[i:min(i + 4, hi)], _extras(targets, i, min(i + 4, hi))) for i in range(lo, hi, 4)]


def _metrics():
    from ssds.core.evaluation_metrics import AveragePrecisionSweep, CocoSummary

    return [AveragePrecisionSweep(5, 0.005), CocoSummary(5, 0.005)]


@pytest.mark.gpu
def test_coco_summary_in_the_eval_epoch_on_decoder_outputs_equals_the_oracle():
    """The epoch hands the extras of a batch to ``CocoSummary`` and the same targets as ever to ``AveragePrecisionSweep``."""
    from ssds.pipeline.pipeline_anchor_ddp import eval_anchor_based_epoch

    model, anchors, decoder = _detector()
    images, targets = _images(10)
    batches = _rank_batches(images, targets, 0, 10)
    (s_AP, s_detail), (AP, detail) = eval_anchor_based_epoch(model, batches, decoder, anchors, 5, torch.device("cuda"), metrics=_metrics())
    plain = eval_anchor_based_epoch(model, [b[:2] for b in batches], decoder, anchors, 5, torch.device("cuda"), metrics=_metrics()[:1])
    assert plain[0][0] == s_AP and np.array_equal(plain[0][1]["ap"], s_detail["ap"], equal_nan=True)
    o = CO.Summary(5, 0.005)
    with torch.no_grad():
        for im, tg, ex in batches:
            scores, boxes, classes = (x.float() for x in decoder(*model(im.cuda()), anchors))
            scores, order = torch.sort(scores, dim=1, descending=True, stable=True)
            boxes, classes = torch.gather(boxes, 1, order.unsqueeze(-1).expand(-1, -1, 4)), torch.gather(classes, 1, order)
            t = tg.float().clone()
            t[:, :, 2:4] = t[:, :, :2] + t[:, :, 2:4]
            o((scores.cpu().numpy(), boxes.cpu().numpy(), classes.cpu().numpy()), t.numpy(), ex["crowd"].numpy(), ex["area"].numpy(),
              ex["area_scale"].numpy())
    want_AP, want = o.get_results()
    for k, v in want["summary"].items():
        assert abs(detail["summary"][k] - v) <= 1e-12 or (np.isnan(v) and np.isnan(detail["summary"][k])), k
    np.testing.assert_allclose(detail["ap"], want["ap"], rtol=0, atol=1e-12, equal_nan=True)
    np.testing.assert_allclose(detail["recall"], want["recall"], rtol=0, atol=1e-12, equal_nan=True)
    assert np.nansum(want["recall"]) > 0 and sum(o.counters.values()) > 0


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _results_to_save(results):
    (s_AP, s_detail), (AP, detail) = results
    return {"s_ap": s_detail["ap"], "ap": detail["ap"], "recall": detail["recall"], "summary": list(detail["summary"].values())}


def _rank_main(rank, world, port, out_dir):
    """One rank of the two-rank test (a fresh process; both ranks on cuda:0, gloo: the merge is staged through the host)."""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist

    from ssds.pipeline.pipeline_anchor_ddp import eval_anchor_based_epoch

    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    model, anchors, decoder = _detector()
    images, targets = _images(10)
    metrics = _metrics()
    results = eval_anchor_based_epoch(model, _rank_batches(images, targets, *RANK_SPLIT[rank]), decoder, anchors, 5,
                                      torch.device("cuda", 0), metrics=metrics)
    out = _results_to_save(results)
    out["records"] = tuple(metrics[1]._tp[0].shape)
    torch.save(out, os.path.join(out_dir, "rank%d.pt" % rank))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_two_ranks_on_one_gpu_equal_one_process_bit_for_bit(tmp_path):
    """The merged summary of two ranks against ONE process that runs the same batches, rank 0's then rank 1's (the rank-major
    arrival order ``merge_records`` produces, so that detections of equal score rank alike on both sides)."""
    from ssds.pipeline.pipeline_anchor_ddp import eval_anchor_based_epoch

    world, port = 2, _free_port()
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    procs = [subprocess.Popen(["timeout", "-k", "10", "180", sys.executable, os.path.abspath(__file__), "--rank", str(r), str(world),
                               str(port), str(tmp_path)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
             for r in range(world)]
    try:
        for r, p in enumerate(procs):
            out, _ = p.communicate(timeout=200)
            assert p.returncode == 0, "rank %d exited with %d:\n%s" % (r, p.returncode, out[-4000:])
    finally:
        for p in procs:  # (a rank left waiting for a failed peer)
            if p.poll() is None:
                p.kill()
                p.wait()
    r0, r1 = (torch.load(os.path.join(str(tmp_path), "rank%d.pt" % r), weights_only=False) for r in range(world))
    model, anchors, decoder = _detector()
    images, targets = _images(10)
    batches = _rank_batches(images, targets, *RANK_SPLIT[0]) + _rank_batches(images, targets, *RANK_SPLIT[1])
    one = _results_to_save(eval_anchor_based_epoch(model, batches, decoder, anchors, 5, torch.device("cuda"), metrics=_metrics()))
    assert r0["records"] == r1["records"] == (2 * 6 * 50, 5)  # both hold all records: rank 1's four images padded to rank 0's six
    for r in (r0, r1):
        for k in ("s_ap", "ap", "recall"):
            assert np.array_equal(r[k], one[k], equal_nan=True), k
        assert np.array_equal(np.array(r["summary"]), np.array(one["summary"]), equal_nan=True)
    assert np.nansum(one["recall"]) > 0


_EVAL_CFG = """
MODEL:
  SSDS: SSD
  NETS: MobileNetV2
  IMAGE_SIZE: [96, 96]
  NUM_CLASSES: 4
  FEATURE_LAYER: [[5, 7, 'Conv:S'], [96, 320, 64]]
  SIZES: [[2.0, 2.828], [2.0, 2.828], [2.0, 2.828]]
  ASPECT_RATIOS: [[1, 2, 0.5], [1, 2, 0.5], [1, 2, 0.5]]
TRAIN:
  RESUME_SCOPE: ''
TEST:
  BATCH_SIZE: 8
  TEST_SCOPE: [1, 1]
POST_PROCESS:
  SCORE_THRESHOLD: 0.005
  IOU_THRESHOLD: 0.5
  MAX_DETECTIONS: 50
  MAX_DETECTIONS_PER_LEVEL: 200
  USE_DIOU: False
  RESCORE_CENTER: False
DATASET:
  DATASET: 'packed'
  DATASET_DIR: '%(data)s'
EXP_DIR: '%(exp)s'
LOG_DIR: '%(exp)s'
PHASE: ['eval']
"""


@pytest.mark.gpu
def test_solver_eval_model_on_shards_writes_the_nine_new_keys_and_keeps_the_old_ones(tmp_path):
    """A directory of synthetic shards with crowd flags and areas: the record holds the nine new keys, equal to a stand-alone
    ``CocoSummary`` over the loader with ``eval_extras``; the keys it always held equal a run with the two metrics it always had
    over the loader as it always was.  (The network is untrained: the numbers themselves are zeros; that they are right on
    ``Decoder`` outputs is the business of the eval-epoch test above.)"""
    from ssds.core import checkpoint, config
    from ssds.core.evaluation_metrics import AveragePrecisionSweep, CocoSummary, MeanAveragePrecision
    from ssds.dataset.augment import AugmentedLoader, PackedDetectionSource
    from ssds.modeling import model_builder
    from ssds.pipeline.pipeline_anchor_ddp import eval_anchor_based_epoch
    from ssds.utils.train_ddp import COCO_SUMMARY_KEYS, Solver
    from tools.pack_dataset import synthetic_set, write_shards

    images, boxes = synthetic_set(20, seed=4, height=(200, 260), width=(220, 300), max_boxes=5, num_classes=4)
    rs = np.random.RandomState(1)
    crowd = [(rs.random_sample(len(b)) < 0.3).astype(np.int32) for b in boxes]
    area = [((b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1]) * rs.uniform(0.5, 1.0, len(b))).astype(F32) for b in boxes]
    data, exp = tmp_path / "data", tmp_path / "exp"
    write_shards(str(data), images, boxes, per_shard=8, crowd=crowd, area=area)
    cfg_path = tmp_path / "eval.yml"
    cfg_path.write_text(_EVAL_CFG % {"exp": str(exp), "data": str(data)})
    config.reset_cfg()
    cfg = config.cfg_from_file(str(cfg_path))
    dev = torch.device("cuda", 0)
    torch.manual_seed(101)
    model = model_builder.create_model(cfg.MODEL)
    with torch.no_grad():  # seeded head biases: scores, classes and boxes of an untrained network that differ
        for mod in model.modules():
            if isinstance(mod, torch.nn.Conv2d) and mod.bias is not None and mod.out_channels == 6 * 4:
                mod.bias.add_(torch.randn_like(mod.bias))
    path = checkpoint.save_checkpoints(model, str(exp), cfg.CHECKPOINTS_PREFIX, 1)
    records = Solver(cfg, 0, dev, phase="eval").eval_model()
    lines = [json.loads(l) for l in open(str(exp / "eval_results.jsonl")).read().splitlines()]
    assert lines == records and len(lines) == 1 and lines[0]["checkpoint"] == path and lines[0]["images"] == 20
    line = lines[0]
    assert COCO_SUMMARY_KEYS == ("APs", "APm", "APl", "AR1", "AR10", "AR100", "ARs", "ARm", "ARl")
    assert list(line) == ["epoch", "checkpoint", "mAP_reference", "AP", "AP50", "AP75", "images", "seconds"] + list(COCO_SUMMARY_KEYS)

    def run(metrics, extras):
        model = model_builder.create_model(cfg.MODEL)
        checkpoint.resume_checkpoint(model, path, "")
        model.eval().to(dev, torch.bfloat16)
        anchors = model_builder.create_anchors(cfg.MODEL, model, cfg.MODEL.IMAGE_SIZE)
        decoder = model_builder.create_decoder(cfg.POST_PROCESS)
        loader = AugmentedLoader(PackedDetectionSource(str(data)), cfg.DATASET, 8, dev, dtype=torch.bfloat16, training=False,
                                 image_size=cfg.MODEL.IMAGE_SIZE, eval_extras=extras)
        if not extras:
            assert all(len(b) == 2 for b in loader)  # what it always yielded
        return eval_anchor_based_epoch(model, loader, decoder, anchors, 4, dev, metrics=metrics(decoder))

    (ref, _), (ap, detail) = run(lambda d: [MeanAveragePrecision(4, d.conf_threshold, d.nms_threshold),
                                            AveragePrecisionSweep(4, d.conf_threshold)], False)
    as_json = lambda v: None if np.isnan(v) else float(v)  # noqa: E731
    assert line["mAP_reference"] == as_json(ref) and line["AP"] == as_json(ap)
    assert line["AP50"] == as_json(detail["mAP_per_iou"][0]) and line["AP75"] == as_json(detail["mAP_per_iou"][5])
    ((_, coco),) = run(lambda d: [CocoSummary(4, d.conf_threshold)], True)
    for key in COCO_SUMMARY_KEYS:
        assert line[key] == as_json(coco["summary"][key]), key
    # the extras reach the metric: in source pixels the set has large boxes (an area above 96^2), in the pixels of the 96 x 96 input
    # -- what the metric sees without area and area_scale -- no box can be large, and ARl has nothing to average
    assert sum(int((a > 96.0 ** 2).sum()) for a in area) > 3
    ((_, bare),) = run(lambda d: [CocoSummary(4, d.conf_threshold)], False)
    assert line["ARl"] is not None and line["APl"] is not None and np.isnan(bare["summary"]["ARl"]) and np.isnan(bare["summary"]["APl"])
    config.reset_cfg()


if __name__ == "__main__" and len(sys.argv) == 6 and sys.argv[1] == "--rank":
    _rank_main(int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), sys.argv[5])
