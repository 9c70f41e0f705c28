"""The average-precision sweep on the device (csrc/ssdk_apsweep.hip, ssds.core.evaluation_metrics.AveragePrecisionSweep) and the
eval phase built on it (pipeline_anchor_ddp.eval_anchor_based_epoch(metrics=...), train_ddp.Solver.eval_model).

1. the reference's rule at one threshold IS ssdk_map_match / ssdk_map_average_precision: keys, flags, counts and AP bit for bit;
2. both rules at 10 and 16 thresholds against tests/apsweep_oracle.py on seeded inputs that keep every IoU 1e-4 away from every
   threshold and have distinct scores per class (both asserted): keys, masks and counts bit for bit, AP within 1e-12;
3. the hand case; guard bands around every buffer of both entry points; no host synchronisation in ``__call__``; the same bits over
   three calls;
4. the eval epoch with a list of metrics against both oracles, two ranks on one GPU against one process, and
   ``Solver.eval_model`` over the checkpoints of an EXP_DIR."""
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
for _p in (ROOT, os.path.join(ROOT, "ssds.pytorch_amd")):  # (a rank of the two-rank test starts this file without pytest)
    if _p not in sys.path:
        sys.path.insert(0, _p)

import apsweep_oracle as AO  # noqa: E402
import guardband as G  # noqa: E402

F32 = np.float32
RULES = {"reference": 0, "coco": 1}


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _thr(v):
    return (ctypes.c_float * len(v))(*[float(t) for t in v])


def _targets_ptr(t):
    return t.data_ptr() if t.numel() else torch.empty(8, device="cuda").data_ptr()  # (G = 0: never read, but a pointer)


def _sweep_match(det, targets, C, conf, thr, rule, max_dets=100, npos=None, keys=None, mask=None):
    """One raw ssdk_apsweep_match on device tensors -> (keys, mask, npos)."""
    from ssds import _native as N

    scores, boxes, classes = det
    B, D = scores.shape
    keys = torch.empty((B, D), device="cuda", dtype=torch.int64) if keys is None else keys
    mask = torch.empty((B, D), device="cuda", dtype=torch.int32) if mask is None else mask
    npos = torch.zeros(C, device="cuda", dtype=torch.int32) if npos is None else npos
    N.check(N.lib.ssdk_apsweep_match(scores.data_ptr(), boxes.data_ptr(), classes.data_ptr(), B, D, _targets_ptr(targets),
                                     int(targets.shape[1]), C, conf, _thr(thr), len(thr), RULES[rule], max_dets, keys.data_ptr(),
                                     mask.data_ptr(), npos.data_ptr(), N.stream_ptr(scores.device)), "apsweep_match")
    return keys, mask, npos


def _sorted(keys, tp, C):
    skeys, order = torch.sort(keys.view(-1), stable=True)
    seg = torch.searchsorted(skeys, torch.arange(C + 1, device="cuda", dtype=torch.int64) << 32).contiguous()
    return tp.view(-1)[order].contiguous(), seg


def _sweep_ap(mask_sorted, seg, npos, C, T, rule, ap=None):
    from ssds import _native as N

    ap = torch.empty((T, C), device="cuda", dtype=torch.float64) if ap is None else ap
    N.check(N.lib.ssdk_apsweep_average_precision(mask_sorted.data_ptr(), seg.data_ptr(), npos.data_ptr(), C, T, RULES[rule],
                                                 ap.data_ptr(), N.stream_ptr(npos.device)), "apsweep_average_precision")
    return ap


# ---- 1. the reference's rule at T = 1 -----------------------------------------------------------------------------------------
def _random_batch(seed, B, D, Gt, C):
    """Vectorised: jittered copies of the ground truth and random boxes, scores descending and distinct, some rows of padding,
    a few classes out of range."""
    rs = np.random.RandomState(seed)
    tg = np.full((B, max(Gt, 0), 5), -1, F32)
    sc, bx, cl = np.zeros((B, D), F32), np.zeros((B, D, 4), F32), np.zeros((B, D), F32)
    pool = rs.permutation(1 << 20)[:B * D].reshape(B, D)
    for b in range(B):
        g = Gt if b == 0 else rs.randint(0, Gt + 1)
        xy = rs.random_sample((g, 2)) * 400
        tg[b, :g] = np.concatenate([xy, xy + 20 + rs.random_sample((g, 2)) * 150, rs.randint(0, C, (g, 1))], 1)
        n = D if b == 0 else rs.randint(0, D + 1)
        src = rs.randint(0, max(g, 1), n)
        hit = (rs.random_sample(n) < 0.7) & (g > 0)
        rnd_xy = rs.random_sample((n, 2)) * 400
        rnd = np.concatenate([rnd_xy, rnd_xy + 20 + rs.random_sample((n, 2)) * 150], 1)
        jit = (rs.random_sample((n, 4)) - 0.5) * 30
        bx[b, :n] = np.where(hit[:, None], (tg[b, src, :4] if g else rnd) + jit, rnd)
        cl[b, :n] = np.where(hit, tg[b, src, 4] if g else 0, rs.randint(-1, C + 1, n))
        sc[b, :n] = np.sort((0.02 + 0.97 * (pool[b, :n] + 1) / float((1 << 20) + 1)).astype(F32))[::-1]
    return (sc, bx, cl), tg


@pytest.mark.gpu
@pytest.mark.parametrize("B,D,Gt,C", [(3, 37, 5, 4), (1, 2048, 256, 3), (2, 1, 0, 2)])
def test_reference_rule_at_one_threshold_is_ssdk_map_match_bit_for_bit(B, D, Gt, C):
    from ssds import _native as N

    det, tg = _random_batch(B + D, B, D, Gt, C)
    det, tg = tuple(_dev(x) for x in det), _dev(tg)
    conf, iou = 0.05, 0.5
    keys0 = torch.empty((B, D), device="cuda", dtype=torch.int64)
    tp0 = torch.empty((B, D), device="cuda", dtype=torch.uint8)
    npos0 = torch.zeros(C, device="cuda", dtype=torch.int32)
    N.check(N.lib.ssdk_map_match(det[0].data_ptr(), det[1].data_ptr(), det[2].data_ptr(), B, D, _targets_ptr(tg), Gt, C, conf, iou,
                                 keys0.data_ptr(), tp0.data_ptr(), npos0.data_ptr(), N.stream_ptr(keys0.device)), "map_match")
    keys, mask, npos = _sweep_match(det, tg, C, conf, [iou], "reference", max_dets=1)  # (max_dets is ignored under this rule)
    assert torch.equal(keys, keys0) and torch.equal(mask, tp0.to(torch.int32)) and torch.equal(npos, npos0)
    if Gt:
        assert int(tp0.sum()) > 0
    tp_s, seg = _sorted(keys0, tp0, C)
    ap0 = torch.empty(C, device="cuda", dtype=torch.float64)
    N.check(N.lib.ssdk_map_average_precision(tp_s.data_ptr(), seg.data_ptr(), npos0.data_ptr(), C, ap0.data_ptr(),
                                             N.stream_ptr(keys0.device)), "map_average_precision")
    mask_s, seg2 = _sorted(keys, mask, C)
    ap = _sweep_ap(mask_s, seg2, npos, C, 1, "reference")
    assert G.same_bits(ap[0], ap0)


# ---- 2. both rules against the oracle -------------------------------------------------------------------------------------------
SWEEP_CASES = OrderedDict((
    # name: (seed, B, D, G, C, max_dets, generator options)
    ("clustered", (11, 4, 100, 7, 5, 100, dict(clustered=True))),
    ("max_dets_100_of_150", (12, 2, 150, 9, 3, 100, dict(full_gt=True))),
    ("many_per_class_max_dets_256", (13, 2, 300, 40, 2, 256, dict(full_gt=True))),  # 150 detections of a class: several chunks
    ("more_than_64_boxes_of_a_class", (14, 1, 130, 150, 2, 120, dict(clustered=True))),  # a lane holds boxes of two chunks
    ("edges", (15, 4, 40, 6, 3, 100, dict(empty_image=1, no_det_image=2, bad_class=0.15))),  # + padded target rows (images 1 .. 3)
))
THRESHOLDS = {10: AO.COCO_IOUS, 16: AO.SWEEP16}


@functools.lru_cache(maxsize=None)
def _case(name, T):
    seed, B, D, Gt, C, max_dets, opts = SWEEP_CASES[name]
    return AO.make_case(seed, B, D, Gt, C, THRESHOLDS[T], batches=2, **opts)


@functools.lru_cache(maxsize=None)
def _oracle(name, T, rule):
    """Computed once per (case, thresholds, rule), shared and left unchanged: ([(cls, mask)] per batch, npos, ap [T, C])."""
    seed, B, D, Gt, C, max_dets, opts = SWEEP_CASES[name]
    o = AO.Sweep(C, 0.06, THRESHOLDS[T], rule, max_dets)
    per_batch = []
    for det, tg in _case(name, T):
        o(det, tg)
        per_batch.append((o.cls[-1].copy(), o.mask[-1].copy()))
    return per_batch, o.npos.copy(), o.get_results()


@pytest.mark.gpu
@pytest.mark.parametrize("T", [10, 16])
@pytest.mark.parametrize("rule", ["coco", "reference"])
@pytest.mark.parametrize("name", list(SWEEP_CASES))
def test_sweep_against_the_oracle(name, rule, T):
    from ssds.core.evaluation_metrics import AveragePrecisionSweep

    seed, B, D, Gt, C, max_dets, opts = SWEEP_CASES[name]
    case, thr = _case(name, T), THRESHOLDS[T]
    assert AO.iou_margin(case, thr) >= AO.MARGIN, "the generator must keep every IoU away from the thresholds"
    assert AO.distinct_scores(case), "the generator must give distinct scores"
    per_batch, want_npos, (want_mAP, want_ap) = _oracle(name, T, rule)
    m = AveragePrecisionSweep(C, 0.06, thr, rule, max_dets)
    for (det, tg), (want_cls, want_mask) in zip(case, per_batch):
        m(tuple(_dev(x) for x in det), _dev(tg))
        cls, score = AO.decode_keys(m._keys[-1].cpu().numpy())
        np.testing.assert_array_equal(cls, want_cls)
        np.testing.assert_array_equal(score, det[0].ravel())
        np.testing.assert_array_equal(m._tp[-1].cpu().numpy(), want_mask)
    np.testing.assert_array_equal(m._npos.cpu().numpy(), want_npos)
    tps = sum(int(np.count_nonzero(w[1])) for w in per_batch)
    if name != "edges":
        assert tps > 20 and len(set(int(v) for w in per_batch for v in w[1])) > 4  # masks that differ over the thresholds
    mAP, detail = m.get_results()
    np.testing.assert_allclose(detail["ap"], want_ap, rtol=0, atol=1e-12, equal_nan=True)
    assert abs(mAP - want_mAP) <= 1e-12 and 0.0 < mAP < 1.0
    np.testing.assert_allclose(detail["mAP_per_iou"], np.nanmean(want_ap, 1), rtol=0, atol=1e-12)
    np.testing.assert_array_equal(detail["iou_thresholds"], thr)


def test_the_seeded_cases_exercise_what_they_are_named_for():
    """(no device) the two rules give different masks, max_dets cuts, and a class has more than 64 boxes."""
    a, b = _oracle("clustered", 10, "coco"), _oracle("clustered", 10, "reference")
    assert any((x[1] != y[1]).any() for x, y in zip(a[0], b[0]))
    for name in ("max_dets_100_of_150", "many_per_class_max_dets_256"):
        seed, B, D, Gt, C, max_dets, opts = SWEEP_CASES[name]
        (scores, _, classes), _ = _case(name, 10)[0]
        assert ((scores > 0.06) & (classes >= 0) & (classes < C)).sum(1).max() > max_dets, name
    seed, B, D, Gt, C, max_dets, opts = SWEEP_CASES["more_than_64_boxes_of_a_class"]
    tg = _case("more_than_64_boxes_of_a_class", 10)[0][1]
    assert max((tg[0, :, 4] == c).sum() for c in range(C)) > 64
    (scores, _, classes), _ = _case("many_per_class_max_dets_256", 10)[0]
    assert max((classes[0][scores[0] > 0.06] == c).sum() for c in range(2)) > 64


# ---- 3. hand case, guard bands, no synchronisation, reproducibility ----------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("rule", ["coco", "reference"])
def test_hand_case_on_the_device(rule):
    from ssds.core.evaluation_metrics import AveragePrecisionSweep

    det, targets, thr, want = AO.hand_case()
    m = AveragePrecisionSweep(1, 0.01, thr, rule)
    m(tuple(_dev(x) for x in det), _dev(targets))
    cls, score, mask, npos = m.records()
    assert mask.tolist() == want[rule][0] and cls.tolist() == [0, 0] and npos.tolist() == [2] and score.tolist() == [F32(0.9), F32(0.8)]
    mAP, detail = m.get_results()
    np.testing.assert_allclose(detail["ap"][:, 0], want[rule][1], rtol=0, atol=1e-15)
    # two identical boxes (0, 1) and a third inside them.  d1 and d3 are the same box, IoU 0.95 with boxes 0 and 1: under the COCO
    # rule d1 takes box 1 (the highest index among equals) and d3 finds box 0 free; under the reference's both look at box 0 (the
    # first maximum) and d3 is a false positive.  d2 is box 2 itself (IoU 1.0; 0.8 with the others): a true positive everywhere.
    tg = _dev(np.array([[[0, 0, 10, 10, 0], [0, 0, 10, 10, 0], [0, 0, 10, 8, 0]]], F32))
    three = tuple(_dev(x) for x in (np.array([[0.9, 0.8, 0.7]], F32), np.array([[[0, 0, 10, 9.5], [0, 0, 10, 8], [0, 0, 10, 9.5]]], F32),
                                    np.zeros((1, 3), F32)))
    thr3 = [0.5, 0.9, 0.99]
    _, mask, _ = _sweep_match(three, tg, 1, 0.01, thr3, rule)
    assert mask.tolist() == [[0b011, 0b111, 0b011 if rule == "coco" else 0b000]]
    assert mask.tolist() == AO.match(tuple(x.cpu().numpy() for x in three), tg.cpu().numpy(), 1, 0.01, thr3, rule)[1].tolist()


@pytest.mark.gpu
@pytest.mark.parametrize("rule", ["coco", "reference"])
def test_guard_bands_around_every_buffer_of_both_entry_points(rule):
    (det, tg), thr = _case("clustered", 16)[0], THRESHOLDS[16]
    seed, B, D, Gt, C, max_dets, opts = SWEEP_CASES["clustered"]
    clean = _sweep_match(tuple(_dev(x) for x in det), _dev(tg), C, 0.06, thr, rule, max_dets)
    gs = G.GuardSet("cuda")
    g_det = tuple(gs.inp(n, torch.from_numpy(x)) for n, x in zip(("scores", "boxes", "classes"), det))
    g_tg = gs.inp("targets", torch.from_numpy(tg))
    g_keys, g_mask = gs.out("keys", (B, D), torch.int64), gs.out("tp_mask", (B, D), torch.int32)
    g_npos = gs.zeros("npos", 4 * C).view(torch.int32)
    gs.arm()
    _sweep_match(g_det, g_tg, C, 0.06, thr, rule, max_dets, npos=g_npos, keys=g_keys, mask=g_mask)
    torch.cuda.synchronize()
    assert gs.problems() == []
    assert torch.equal(g_keys, clean[0]) and torch.equal(g_mask, clean[1]) and torch.equal(g_npos, clean[2])  # every slot written

    T = len(thr)
    mask_s, seg = _sorted(clean[0], clean[1], C)
    clean_ap = _sweep_ap(mask_s, seg, clean[2], C, T, rule)
    gs = G.GuardSet("cuda")
    g_m, g_seg, g_np = gs.inp("tp_mask_sorted", mask_s), gs.inp("seg_offsets", seg), gs.inp("npos", clean[2])
    g_ap = gs.out("ap", (T, C), torch.float64)
    gs.arm()
    _sweep_ap(g_m, g_seg, g_np, C, T, rule, ap=g_ap)
    torch.cuda.synchronize()
    assert gs.problems() == [] and G.same_bits(g_ap, clean_ap)


@pytest.mark.gpu
@pytest.mark.parametrize("rule", ["coco", "reference"])
def test_call_does_not_synchronise_and_three_calls_give_the_same_bits(rule):
    from ssds.core.evaluation_metrics import AveragePrecisionSweep, MeanAveragePrecision

    seed, B, D, Gt, C, max_dets, opts = SWEEP_CASES["many_per_class_max_dets_256"]
    batches = [(tuple(_dev(x) for x in det), _dev(tg)) for det, tg in _case("many_per_class_max_dets_256", 10)]
    torch.cuda.synchronize()
    runs = []
    for _ in range(3):
        m, ref = AveragePrecisionSweep(C, 0.06, AO.COCO_IOUS, rule, max_dets), MeanAveragePrecision(C, 0.06, 0.5)
        m(*batches[0])  # (the first call creates the counters)
        torch.cuda.set_sync_debug_mode("error")
        try:
            m(*batches[1])
            ref(*batches[1])
        finally:
            torch.cuda.set_sync_debug_mode("default")
        runs.append((torch.cat(m._keys), torch.cat(m._tp), m._npos.clone(), m.average_precision()))
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert G.same_bits(a, b)


# ---- 4. the eval epoch, two ranks, Solver.eval_model ----------------------------------------------------------------------------
def _detector(seed=0):
    """The 128-pixel MobileNetV2 SSD of tests/test_gpu_train.py::test_eval_epoch_on_device_matches_oracle_metric."""
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
    """``n`` seeded images with targets (xywh + label, -1 padding), on the CPU."""
    from ssds.dataset.synthetic import SyntheticDetectionLoader

    return SyntheticDetectionLoader(n, (128, 128), 5, steps=1, device=torch.device("cpu"), max_gt=6, seed=seed).batch()


def _metrics():
    from ssds.core.evaluation_metrics import AveragePrecisionSweep, MeanAveragePrecision

    return [MeanAveragePrecision(5, 0.005, 0.5), AveragePrecisionSweep(5, 0.005, max_dets=40),
            AveragePrecisionSweep(5, 0.005, AO.SWEEP16, "reference")]


@pytest.mark.gpu
def test_eval_epoch_with_a_list_of_metrics_matches_both_oracles():
    from oracle import map_oracle as MO
    from ssds.pipeline.pipeline_anchor_ddp import eval_anchor_based_epoch

    model, anchors, decoder = _detector()
    images, targets = _images(10)
    dev = torch.device("cuda")
    batches = [(images[i:i + 4], targets[i:i + 4]) for i in (0, 4, 8)]  # (on the CPU: the epoch moves them; the last one is short)
    (mAP, (prec, rec, ap)), (c_mAP, c_detail), (r_mAP, r_detail) = eval_anchor_based_epoch(model, batches, decoder, anchors, 5, dev,
                                                                                          metrics=_metrics())
    plain = eval_anchor_based_epoch(model, batches, decoder, anchors, 5, dev)  # metrics=None: what it always returned
    assert plain[0] == mAP and plain[1][2] == ap and len(plain) == 2 and len(plain[1]) == 3
    assert all(np.array_equal(a, b) for a, b in zip(plain[1][0], prec)) and all(np.array_equal(a, b) for a, b in zip(plain[1][1], rec))

    orc = [MO.MeanAveragePrecision(5, 0.005, 0.5), AO.Sweep(5, 0.005, AO.COCO_IOUS, "coco", 40), AO.Sweep(5, 0.005, AO.SWEEP16, "reference")]
    with torch.no_grad():
        for im, tg in batches:
            det = decoder(*model(im.cuda()), anchors)
            t = tg.float().clone()
            t[:, :, 2:4] = t[:, :, :2] + t[:, :, 2:4]
            for o in orc:
                o(tuple(x.cpu().numpy() for x in det), t.numpy())
    omAP, oap = orc[0].get_results()
    assert sum(len(x) for x in orc[0].score) > 0
    np.testing.assert_allclose(np.array(ap), np.array(oap), rtol=1e-12, atol=1e-15, equal_nan=True)
    for (got_mAP, detail), o in ((c_mAP, c_detail), orc[1]), ((r_mAP, r_detail), orc[2]):
        want_mAP, want_ap = o.get_results()
        np.testing.assert_allclose(detail["ap"], want_ap, rtol=0, atol=1e-12, equal_nan=True)
        assert abs(got_mAP - want_mAP) <= 1e-12
    assert int(sum(np.count_nonzero(m) for m in orc[1].mask)) > 0


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


RANK_SPLIT = ((0, 6), (6, 10))  # 10 images: rank 0 evaluates six (batches of 4 and 2), rank 1 four: unequal record counts


def _rank_batches(images, targets, lo, hi):
    return [(images[i:min(i + 4, hi)], targets[i:min(i + 4, hi)]) for i in range(lo, hi, 4)]


def _results_to_save(results):
    (mAP, (_, _, ap)), (c_mAP, c_detail), (r_mAP, r_detail) = results
    return {"mAP": mAP, "ap": np.array(ap), "c_mAP": c_mAP, "c_ap": c_detail["ap"], "r_mAP": r_mAP, "r_ap": r_detail["ap"]}


def _rank_main(rank, world, port, out_dir):
    """One rank of the two-rank test (a fresh process; both ranks on cuda:0, gloo: the merge is staged through the host)."""
    sys.path[:0] = [ROOT, os.path.join(ROOT, "ssds.pytorch_amd"), os.path.join(ROOT, "tests")]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist

    from ssds.pipeline.pipeline_anchor_ddp import eval_anchor_based_epoch

    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    model, anchors, decoder = _detector()
    images, targets = _images(10)
    metrics = _metrics()
    results = eval_anchor_based_epoch(model, _rank_batches(images, targets, *RANK_SPLIT[rank]), decoder, anchors, 5, torch.device("cuda", 0),
                                      metrics=metrics)
    out = _results_to_save(results)
    out["records"] = int(metrics[1]._keys[0].numel())
    torch.save(out, os.path.join(out_dir, "rank%d.pt" % rank))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_two_ranks_on_one_gpu_equal_one_process_bit_for_bit(tmp_path):
    """The merged result of two ranks against ONE process that evaluates the same ten images.  The one process runs the same
    batches, rank 0's then rank 1's: what a forward computes for an image may depend on the batch it is in, which is not the
    metric's business -- and that order is the rank-major arrival order ``merge_records`` produces, so detections of equal score
    (the untrained heads give many: all scores lie within 1e-5 of the prior) rank alike on both sides."""
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
    metrics = _metrics()
    batches = _rank_batches(images, targets, *RANK_SPLIT[0]) + _rank_batches(images, targets, *RANK_SPLIT[1])
    one = _results_to_save(eval_anchor_based_epoch(model, batches, decoder, anchors, 5, torch.device("cuda"), metrics=metrics))
    assert int((metrics[1].records()[0] < 5).sum()) > 0
    # both ranks hold all records: the longest rank's count from each (rank 1's four images padded to rank 0's six)
    assert r0["records"] == r1["records"] == 2 * 6 * 50 and int(metrics[1]._keys[0].numel()) == 4 * 50
    for r in (r0, r1):
        for k in ("ap", "c_ap", "r_ap"):
            assert np.array_equal(r[k], one[k], equal_nan=True), k
        for k in ("mAP", "c_mAP", "r_mAP"):
            assert r[k] == one[k] or (np.isnan(r[k]) and np.isnan(one[k])), k
    assert np.nansum(one["c_ap"]) > 0


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
  TEST_SCOPE: [2, 3]
POST_PROCESS:
  SCORE_THRESHOLD: 0.005
  IOU_THRESHOLD: 0.5
  MAX_DETECTIONS: 50
  MAX_DETECTIONS_PER_LEVEL: 200
  USE_DIOU: False
  RESCORE_CENTER: False
DATASET:
  DATASET: 'synthetic'
EXP_DIR: '%(exp)s'
LOG_DIR: '%(exp)s'
PHASE: ['eval']
"""


@pytest.mark.gpu
def test_solver_eval_model_evaluates_every_checkpoint_in_scope_with_its_own_weights(tmp_path):
    """Three checkpoints of different weights, two inside TEST_SCOPE: each line of eval_results.jsonl equals a stand-alone
    evaluation of that checkpoint, and the two lines differ (a plan recorded for the first checkpoint must not answer for the
    second)."""
    from ssds.core import checkpoint, config
    from ssds.core.evaluation_metrics import AveragePrecisionSweep, MeanAveragePrecision
    from ssds.dataset.synthetic import SyntheticDetectionLoader
    from ssds.modeling import model_builder
    from ssds.pipeline.pipeline_anchor_ddp import eval_anchor_based_epoch
    from ssds.utils.train_ddp import Solver

    exp = tmp_path / "exp"
    cfg_path = tmp_path / "eval.yml"
    cfg_path.write_text(_EVAL_CFG % {"exp": str(exp)})
    config.reset_cfg()
    cfg = config.cfg_from_file(str(cfg_path))
    dev = torch.device("cuda", 0)
    paths = {}
    for epoch in (1, 2, 3):
        torch.manual_seed(100 + epoch)
        model = model_builder.create_model(cfg.MODEL)
        with torch.no_grad():  # the features of an untrained network vanish in eval mode, so what the heads return is their bias:
            for mod in model.modules():  # seeded biases give every checkpoint its own scores, classes and boxes
                if isinstance(mod, torch.nn.Conv2d) and mod.bias is not None and mod.out_channels == 6 * 4:  # loc and conf: A = 6, C = 4
                    mod.bias.add_(torch.randn_like(mod.bias))
        paths[epoch] = checkpoint.save_checkpoints(model, str(exp), cfg.CHECKPOINTS_PREFIX, epoch)
    records = Solver(cfg, 0, dev, steps_per_epoch=2, phase="eval").eval_model()
    lines = [json.loads(l) for l in open(str(exp / "eval_results.jsonl")).read().splitlines()]
    assert lines == records and [l["epoch"] for l in lines] == [2, 3] and [l["checkpoint"] for l in lines] == [paths[2], paths[3]]
    for line in lines:
        model = model_builder.create_model(cfg.MODEL)
        checkpoint.resume_checkpoint(model, paths[line["epoch"]], "")
        model.eval().to(dev, torch.bfloat16)
        anchors = model_builder.create_anchors(cfg.MODEL, model, cfg.MODEL.IMAGE_SIZE)
        decoder = model_builder.create_decoder(cfg.POST_PROCESS)
        loader = SyntheticDetectionLoader(8, (96, 96), 4, 2, dev, seed=1234, dtype=torch.bfloat16)
        (ref, _), (ap, detail) = eval_anchor_based_epoch(
            model, loader, decoder, anchors, 4, dev,
            metrics=[MeanAveragePrecision(4, decoder.conf_threshold, decoder.nms_threshold), AveragePrecisionSweep(4, decoder.conf_threshold)])
        assert line["images"] == 16 and line["seconds"] > 0
        assert line["mAP_reference"] == ref and line["AP"] == ap
        assert line["AP50"] == float(detail["mAP_per_iou"][0]) and line["AP75"] == float(detail["mAP_per_iou"][5])
    assert (lines[0]["mAP_reference"], lines[0]["AP"], lines[0]["AP50"]) != (lines[1]["mAP_reference"], lines[1]["AP"], lines[1]["AP50"])
    assert lines[0]["AP50"] > 0 or lines[1]["AP50"] > 0
    config.reset_cfg()


if __name__ == "__main__" and len(sys.argv) == 6 and sys.argv[1] == "--rank":
    _rank_main(int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), sys.argv[5])
