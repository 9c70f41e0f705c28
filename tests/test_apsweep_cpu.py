"""The average-precision sweep without a device: the oracle itself (tests/apsweep_oracle.py) on hand-made cases and against the
one-threshold oracle, the C-ABI of include/ssdk_apsweep.h (header, exports, every argument error before any device call), the
checkpoint selection of ``Solver.eval_model`` and ``merge_records`` under two gloo ranks."""
import ctypes
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import apsweep_oracle as AO
import cases
from oracle import map_oracle as MO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


# ---- the oracle ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", ["coco", "reference"])
def test_hand_case(rule):
    det, targets, thr, want = AO.hand_case()
    iou = MO.matrix_iou(det[1][0], targets[0, :, :4])
    np.testing.assert_allclose(iou, [[9 / 11, 7 / 13], [8.5 / 11.5, 7.5 / 12.5]], rtol=1e-6)  # 0.818 0.538 / 0.739 0.600
    cls, mask, npos = AO.match(det, targets, 1, 0.01, thr, rule)
    assert mask[0].tolist() == want[rule][0] and cls[0].tolist() == [0, 0] and npos.tolist() == [2]
    o = AO.Sweep(1, 0.01, thr, rule)
    o(det, targets)
    mAP, ap = o.get_results()
    np.testing.assert_allclose(ap[:, 0], want[rule][1], rtol=0, atol=1e-15)
    assert abs(mAP - np.mean(want[rule][1])) < 1e-15


def test_identical_boxes_coco_takes_the_second_reference_the_first():
    targets = np.array([[[0, 0, 10, 10, 0], [0, 0, 10, 10, 0]]], F32)
    det = (np.array([[0.9]], F32), np.array([[[0, 0, 10, 9]]], F32), np.zeros((1, 1), F32))
    took = {}
    assert AO.match(det, targets, 1, 0.01, [0.5], "coco", assigned=took)[1].tolist() == [[1]] and took == {(0, 0, 0): 1}
    took = {}
    assert AO.match(det, targets, 1, 0.01, [0.5], "reference", assigned=took)[1].tolist() == [[1]] and took == {(0, 0, 0): 0}
    # what follows from it: a second, identical detection finds the other box free under the COCO rule; under the reference's it
    # looks at the same first box again and is a false positive
    two = (np.array([[0.9, 0.8]], F32), np.repeat(det[1], 2, 1), np.zeros((1, 2), F32))
    took = {}
    assert AO.match(two, targets, 1, 0.01, [0.5], "coco", assigned=took)[1].tolist() == [[1, 1]] and took == {(0, 0, 0): 1, (0, 1, 0): 0}
    assert AO.match(two, targets, 1, 0.01, [0.5], "reference")[1].tolist() == [[1, 0]]


def test_coco_ap_leading_true_positives_of_a_hundred():
    """npos = 100 with k leading true positives: recall k / 100 against the recall point r_k = k * 0.01.  At k = 7 the two are the
    same fp64 number (0.07), so the seventh true positive answers r_0 .. r_7; the points where the product is LARGER than the
    quotient are k = 35, 41, 47, ...: r_35 = 0.35000000000000003 > 35 / 100, and the 35th true positive answers r_0 .. r_34 only."""
    r = np.linspace(0.0, 1.0, 101)
    assert all(r[k] == k * 0.01 for k in range(100)) and r[100] == 1.0
    assert 7 * 0.01 == 7 / 100 and 35 * 0.01 > 35 / 100
    assert [k for k in range(101) if k * 0.01 > k / 100][:3] == [35, 41, 47] and not [k for k in range(101) if k * 0.01 < k / 100]
    assert AO.ap_coco([1] * 7, 100) == 8.0 / 101.0
    assert AO.ap_coco([1] * 7 + [0] * 5, 100) == 8.0 / 101.0
    assert AO.ap_coco([1] * 35, 100) == 35.0 / 101.0
    assert AO.ap_coco([1] * 36, 100) == 37.0 / 101.0
    assert AO.ap_coco([], 3) == 0.0 and np.isnan(AO.ap_coco([1], 0)) and AO.ap_coco([0, 0], 3) == 0.0
    assert AO.ap_coco([1, 1], 2) == 1.0
    np.testing.assert_allclose(AO.ap_coco([0, 1], 1), 0.5, rtol=0, atol=1e-15)  # the envelope reaches back over the false positive


@pytest.mark.parametrize("name", list(cases.MAP_CASES))
def test_reference_rule_at_one_threshold_is_the_map_oracle(name):
    d = cases.map_inputs(name)
    o = AO.Sweep(d["C"], d["conf_thr"], [d["iou_thr"]], "reference")
    m = MO.MeanAveragePrecision(d["C"], d["conf_thr"], d["iou_thr"])
    for bt in d["batches"]:
        det = tuple(bt[k] for k in ("scores", "boxes", "classes"))
        o(det, bt["targets"])
        m(det, bt["targets"])
    flags = AO.ranked_flags(np.concatenate(o.cls), np.concatenate(o.scores), np.concatenate(o.mask), d["C"], 1)
    for c in range(d["C"]):
        order = np.argsort(-np.asarray(m.score[c], dtype=np.float64), kind="stable")
        np.testing.assert_array_equal(flags[c][0], np.asarray(m.detect_ismatched[c], dtype=int)[order])
    np.testing.assert_array_equal(o.npos, m.npos)
    mAP, ap = o.get_results()
    wmAP, wap = m.get_results()
    np.testing.assert_array_equal(ap[0], np.array(wap))
    assert mAP == wmAP or (np.isnan(mAP) and np.isnan(wmAP))


def test_max_dets_counts_valid_detections_by_index():
    targets = np.array([[[0, 0, 10, 10, 0], [20, 0, 30, 10, 0], [40, 0, 50, 10, 1]]], F32)
    boxes = np.array([[[0, 0, 10, 10], [0, 0, 1, 1], [20, 0, 30, 10], [40, 0, 50, 10], [40, 0, 50, 10]]], F32)
    scores = np.array([[0.9, 0.001, 0.8, 0.7, 0.6]], F32)  # (the second one is below the score threshold: it does not count)
    classes = np.array([[0, 0, 0, 1, 7]], F32)  # (the last one is out of range)
    cls, mask, npos = AO.match((scores, boxes, classes), targets, 2, 0.01, [0.5], "coco", max_dets=2)
    assert cls.tolist() == [[0, 2, 0, 2, 2]] and mask.tolist() == [[1, 0, 1, 0, 0]] and npos.tolist() == [2, 1]
    cls, mask, _ = AO.match((scores, boxes, classes), targets, 2, 0.01, [0.5], "coco", max_dets=3)
    assert cls.tolist() == [[0, 2, 0, 1, 2]] and mask.tolist() == [[1, 0, 1, 1, 0]]
    cls, mask, _ = AO.match((scores, boxes, classes), targets, 2, 0.01, [0.5], "reference", max_dets=1)  # ignored
    assert cls.tolist() == [[0, 2, 0, 1, 2]] and mask.tolist() == [[1, 0, 1, 1, 0]]


def test_generated_cases_meet_their_conditions():
    for thr in (AO.COCO_IOUS, AO.SWEEP16):
        case = AO.make_case(3, 2, 40, 6, 3, thr, batches=2, clustered=True, bad_class=0.1)
        assert AO.iou_margin(case, thr) >= AO.MARGIN and AO.distinct_scores(case)
        o = AO.Sweep(3, 0.01, thr, "coco")
        for det, tg in case:
            o(det, tg)
        mAP, ap = o.get_results()
        assert 0.05 < mAP < 0.95 and (np.diff(np.nanmean(ap, 1)) <= 1e-12).all()  # AP falls as the threshold rises
    tie = [((np.array([[0.5, 0.5]], F32), np.zeros((1, 2, 4), F32), np.zeros((1, 2), F32)), np.full((1, 1, 5), -1, F32))]
    assert not AO.distinct_scores(tie)
    near = [((np.array([[0.5]], F32), np.array([[[0, 0, 10, 5.00001]]], F32), np.zeros((1, 1), F32)), np.array([[[0, 0, 10, 10, 0]]], F32))]
    assert AO.iou_margin(near, [0.5]) < AO.MARGIN


# ---- the C-ABI ----------------------------------------------------------------------------------------------------------------
def test_header_parses_and_the_library_exports_exactly_its_two_names():
    from ssds import _native as N

    assert N.APSWEEP_HEADER_PATH.endswith("ssdk_apsweep.h")
    h = N.parse_header(open(N.APSWEEP_HEADER_PATH).read())
    assert tuple(h.functions) == ("ssdk_apsweep_match", "ssdk_apsweep_average_precision") == N.APSWEEP_EXPORTS and not h.structs
    assert h.constants == {"SSDK_APSWEEP_MAX_T": 16, "SSDK_AP_RULE_REFERENCE": 0, "SSDK_AP_RULE_COCO": 1}
    main = open(N.HEADER_PATH).read()
    for name in N.APSWEEP_EXPORTS:
        assert hasattr(N.lib, name) and name not in N.EXPORTS and name not in main
    assert len(N.EXPORTS) == 127 and N.lib.ssdk_version() == 245 and N.ABI_VERSION == 245
    assert N.APSWEEP_MAX_T == 16 and N.AP_RULE == {"reference": 0, "coco": 1}
    rt, args = h.functions["ssdk_apsweep_match"]
    assert rt is ctypes.c_int and len(args) == 17 and args[3] is ctypes.c_int and args[8] is ctypes.c_float and args[9] is ctypes.c_void_p
    assert len(h.functions["ssdk_apsweep_average_precision"][1]) == 8


def _thr(*v):
    return (ctypes.c_float * len(v))(*v)


def test_every_argument_error_is_badarg_with_a_message_and_without_a_device():
    """The pointers are never dereferenced on the way to the error (1 is not an address), and no device exists here."""
    from ssds import _native as N

    L, p, ok = N.lib, 1, _thr(0.5, 0.75)

    def match(scores=p, boxes=p, classes=p, B=2, D=10, targets=p, G=3, C=4, conf=0.1, thr=ok, T=2, rule=1, max_dets=100, keys=p,
              mask=p, npos=p):
        return L.ssdk_apsweep_match(scores, boxes, classes, B, D, targets, G, C, conf, thr, T, rule, max_dets, keys, mask, npos, None)

    def ap(mask=p, seg=p, npos=p, C=4, T=2, rule=1, out=p):
        return L.ssdk_apsweep_average_precision(mask, seg, npos, C, T, rule, out, None)

    bad = [("null", lambda: match(scores=None)), ("null", lambda: match(boxes=None)), ("null", lambda: match(classes=None)),
           ("null", lambda: match(targets=None)), ("null", lambda: match(thr=None)), ("null", lambda: match(keys=None)),
           ("null", lambda: match(mask=None)), ("null", lambda: match(npos=None)),
           ("T=0", lambda: match(T=0)), ("T=17", lambda: match(thr=_thr(*np.linspace(0.1, 0.9, 17)), T=17)),
           ("ascend", lambda: match(thr=_thr(0.5, 0.5))), ("ascend", lambda: match(thr=_thr(0.6, 0.5))),
           ("(0, 1]", lambda: match(thr=_thr(0.0, 0.5))), ("(0, 1]", lambda: match(thr=_thr(0.5, 1.5))),
           ("(0, 1]", lambda: match(thr=_thr(float("nan"), 0.5))), ("(0, 1]", lambda: match(thr=_thr(-0.5, 0.5))),
           ("rule", lambda: match(rule=2)), ("rule", lambda: match(rule=-1)), ("max_dets", lambda: match(max_dets=0)),
           ("dims", lambda: match(B=0)), ("dims", lambda: match(D=0)), ("dims", lambda: match(D=2049)), ("dims", lambda: match(G=-1)),
           ("dims", lambda: match(G=N.MAX_GT + 1)), ("dims", lambda: match(C=0)),
           ("null", lambda: ap(mask=None)), ("null", lambda: ap(seg=None)), ("null", lambda: ap(npos=None)), ("null", lambda: ap(out=None)),
           ("classes", lambda: ap(C=0)), ("T=0", lambda: ap(T=0)), ("T=17", lambda: ap(T=17)), ("rule", lambda: ap(rule=5))]
    for what, call in bad:
        N.lib.ssdk_apsweep_match(None, None, None, 1, 1, None, 0, 1, 0.0, None, 1, 0, 1, None, None, None, None)  # (resets the message)
        assert N.lib.ssdk_last_error().decode() == "apsweep_match: null pointer"
        assert call() == -1, what
        msg = N.lib.ssdk_last_error().decode()
        assert msg.startswith("apsweep_") and what in msg, (what, msg)


def test_python_wrapper_refuses_an_unknown_rule_and_a_cpu_tensor():
    from ssds import _native as N
    from ssds.core.evaluation_metrics import COCO_IOUS, AveragePrecisionSweep

    np.testing.assert_array_equal(COCO_IOUS, AO.COCO_IOUS)
    assert COCO_IOUS.dtype == np.float32 and len(COCO_IOUS) == 10 and COCO_IOUS[0] == 0.5 and COCO_IOUS[5] == F32(0.75)
    with pytest.raises(ValueError):
        AveragePrecisionSweep(3, 0.01, rule="voc")
    m = AveragePrecisionSweep(3, 0.01)
    with pytest.raises(N.SsdkError):
        m((torch.zeros(1, 2), torch.zeros(1, 2, 4), torch.zeros(1, 2)), torch.zeros(1, 1, 5))
    mAP, detail = m.get_results()
    assert np.isnan(mAP) and detail["ap"].shape == (10, 3) and np.isnan(detail["ap"]).all() and len(detail["mAP_per_iou"]) == 10


# ---- Solver.eval_model: which checkpoints ---------------------------------------------------------------------------------------
def test_checkpoint_selection():
    from ssds.utils.train_ddp import select_checkpoints

    index = ([30, 10, 20, 40], ["c30", "c10", "c20", "c40"])
    assert select_checkpoints(index, [10, 30], "") == [(10, "c10"), (20, "c20"), (30, "c30")]  # inclusive, ascending
    assert select_checkpoints(index, [15, 25], "resume.pth") == [(20, "c20")]
    assert select_checkpoints(index, [41, 50], "resume.pth") == [(0, "resume.pth")]
    assert select_checkpoints(False, [0, 300], "resume.pth") == [(0, "resume.pth")]
    assert select_checkpoints(([], []), [0, 300], "resume.pth") == [(0, "resume.pth")]
    with pytest.raises(ValueError, match="RESUME_CHECKPOINT"):
        select_checkpoints(False, [0, 300], "")
    with pytest.raises(ValueError, match=r"TEST_SCOPE \[41, 50\]"):
        select_checkpoints(index, [41, 50], "")


def test_main_takes_dash_e(tmp_path, monkeypatch):
    """``-e`` reaches ``eval_model`` (and nothing of the training set-up) -- with nothing to evaluate it says so."""
    from ssds.core import config
    from ssds.utils import train_ddp

    config.reset_cfg()
    cfg = tmp_path / "e.yml"
    cfg.write_text("MODEL:\n  NUM_CLASSES: 3\nEXP_DIR: '%s'\nRESUME_CHECKPOINT: ''\n" % (tmp_path / "exp"))
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(ValueError, match="nothing to evaluate"):
        train_ddp.main(["-cfg", str(cfg), "-e"])
    config.reset_cfg()


# ---- merge_records under gloo --------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_records(rank):
    """Rank 0 holds 5 records, rank 1 holds 2; classes 0 .. 2 of C = 3, a sentinel among rank 0's."""
    if rank == 0:
        cls, score, tp = [0, 2, 3, 1, 0], [0.9, 0.8, 0.0, 0.7, 0.6], [1, 0, 0, 3, 2]
    else:
        cls, score, tp = [1, 0], [0.95, 0.5], [1, 1]
    bits = np.array(score, F32).view(np.uint32).astype(np.int64)
    ordered = np.where(bits & 0x80000000, ~bits & 0xFFFFFFFF, bits | 0x80000000)
    keys = (np.array(cls, np.int64) << 32) | (~ordered & 0xFFFFFFFF)
    return torch.from_numpy(keys), torch.tensor(tp, dtype=torch.int32), torch.tensor([2, 1, 1 + rank], dtype=torch.int32)


def _merge_worker(rank, world, port, out_dir):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "ssds.pytorch_amd")]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist

    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from ssds.core.evaluation_metrics import MeanAveragePrecision, merge_records

    keys, tp, npos = _rank_records(rank)
    out = merge_records(keys, tp, npos)
    m = MeanAveragePrecision(3, 0.01, 0.5)  # the method on the class, uint8 flags (and a rank's npos stays its own tensor)
    m._keys, m._tp, m._npos = [keys], [(tp > 0).to(torch.uint8)], npos.clone()
    m.merge()
    torch.save({"keys": out[0], "tp": out[1], "npos": out[2], "mine": npos, "m_keys": m._keys[0], "m_tp": m._tp[0], "m_npos": m._npos},
               os.path.join(out_dir, "merged%d.pt" % rank))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_merge_records_two_gloo_ranks_unequal_counts(tmp_path):
    from ssds.core.evaluation_metrics import merge_records

    k0, t0, n0 = _rank_records(0)
    same = merge_records(k0, t0, n0)  # no process group: the records as they are
    assert same[0] is k0 and same[1] is t0 and same[2] is n0
    mp.start_processes(_merge_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True, start_method="spawn")
    r0, r1 = (torch.load(os.path.join(str(tmp_path), "merged%d.pt" % r)) for r in range(2))
    for k in ("keys", "tp", "npos", "m_keys", "m_tp", "m_npos"):
        assert torch.equal(r0[k], r1[k]), k  # every rank holds the same records
    k1, t1, n1 = _rank_records(1)
    assert torch.equal(r0["mine"], n0) and torch.equal(r1["mine"], n1)  # (the caller's tensor is not reduced in place)
    sentinel = (3 << 32) | 0xFFFFFFFF
    want_keys = torch.cat([k0, k1, torch.full((3,), sentinel, dtype=torch.int64)])  # rank order, rank 1 padded to 5
    want_tp = torch.cat([t0, t1, torch.zeros(3, dtype=torch.int32)])
    assert torch.equal(r0["keys"], want_keys) and torch.equal(r0["tp"], want_tp) and r0["tp"].dtype == torch.int32
    assert torch.equal(r0["npos"], n0 + n1) and r0["npos"].dtype == torch.int32
    assert torch.equal(r0["m_keys"], want_keys) and torch.equal(r0["m_tp"], (want_tp > 0).to(torch.uint8)) and torch.equal(r0["m_npos"], n0 + n1)
    # the padding sorts behind every class, after the batch's own sentinel record too, and the classes keep rank-major order
    skeys, order = torch.sort(r0["keys"], stable=True)
    assert (skeys >> 32).tolist() == [0, 0, 0, 1, 1, 2, 3, 3, 3, 3] and (skeys[-3:] == sentinel).all()
    assert order[:6].tolist() == [0, 4, 6, 5, 3, 1]  # class 0: 0.9, 0.6 (rank 0), 0.5 (rank 1); class 1: 0.95 (rank 1), 0.7; class 2
    assert r0["tp"][order][-4:].tolist() == [0, 0, 0, 0]
