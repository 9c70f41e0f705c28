"""The fused loss kernels (csrc/ssdk_match.hip behind ssds/core/fused_loss.py::match_loss) judged per anchor against fp64 by
tests/lossjudge.py: every case forward and backward with the scale 0.37 / #foreground, bit-reproducible; the tail geometries
through the C-ABI entry points between guard bands; the contract edges of the ground-truth tensor ([B, 0, 5], [B, 257, 5])."""
import collections
import ctypes

import pytest

import guardband as G
import lossjudge as J

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _ratios():
    yield
    J.flush_records()


def run(case, ops):
    """match_loss forward + backward with the scale s on the device -> lossjudge.Out"""
    import torch
    from ssds.core.fused_loss import match_loss

    B, Gt, A, C, H, W, stride = J.GEOS[case.geo]
    conf = ops.conf.cuda().requires_grad_(True)
    loc = ops.loc.cuda().requires_grad_(True)
    targets = torch.from_numpy(ops.targets).cuda()
    cls_sum, loc_sum, fg = match_loss(conf, loc, targets, ops.anchors, C, stride, ops.match, ops.radius, J.ALPHA, case.gamma, J.BETA,
                                      case.loc_loss, case.ratio if case.cls == "multibox" else None)
    s = J.scale_of(ops.asg)
    (s * cls_sum + s * loc_sum).backward()
    return J.Out(conf.grad.cpu(), loc.grad.cpu(), float(cls_sum.detach()), float(loc_sum.detach()), float(fg))


@pytest.mark.parametrize("case", J.ALL_CASES, ids=J.cid)
def test_match_loss_passes_the_judge(case):
    ops = J.operands(case)
    J.check_left_out(case, ops)  # from the reference alone, before any device output exists
    out = run(case, ops)
    problems = J.judge(case, ops, out)
    assert not problems, "\n".join(problems)
    again = run(case, ops)
    assert G.same_bits(again.gc, out.gc) and G.same_bits(again.gl, out.gl), "the gradients differ between two calls"
    assert (again.cls_sum, again.loc_sum, again.fg) == (out.cls_sum, out.loc_sum, out.fg), "the sums differ between two calls"


def _abi_call(case, ops, ws_fill):
    """one call of ssdk_match_loss / ssdk_match_multibox_loss with every buffer between guard bands and a workspace of exactly the
    queried size holding ``ws_fill`` -> (problems, d_conf, d_loc, sums)"""
    import torch
    from ssds import _native as N
    from ssds.modeling.layers.box import _anchor_array

    B, Gt, A, C, H, W, stride = J.GEOS[case.geo]
    dt = J.DTYPES[case.dtype]
    multibox = case.cls == "multibox"
    query = N.lib.ssdk_match_multibox_loss_workspace_bytes if multibox else N.lib.ssdk_match_loss_workspace_bytes
    need = int(query(B, A, H, W))
    assert need > 0
    gs = G.GuardSet("cuda")
    targets = gs.inp("targets", torch.from_numpy(ops.targets))
    conf, loc = gs.inp("conf", ops.conf), gs.inp("loc", ops.loc)
    d_conf, d_loc = gs.out("d_conf", conf.shape, dt), gs.out("d_loc", loc.shape, dt)
    sums = gs.out("sums", (3,), torch.float32)
    ws = gs.out("workspace", (need,), torch.uint8, fill=0xFF)
    ws.fill_(ws_fill)
    gs.arm()
    anc = _anchor_array(ops.anchors, stride)
    anc_p = anc.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    dev = conf.device
    with torch.cuda.device(dev):
        if multibox:
            rc = N.lib.ssdk_match_multibox_loss(
                targets.data_ptr(), B, Gt, anc_p, A, C, H, W, stride, 0, J.IOU_MATCH[0], J.IOU_MATCH[1], float(ops.radius),
                conf.data_ptr(), loc.data_ptr(), J.CODES[case.dtype], float(case.ratio), J.BETA, 0, d_conf.data_ptr(),
                d_loc.data_ptr(), sums.data_ptr(), ws.data_ptr(), need, N.stream_ptr(dev))
        else:
            rc = N.lib.ssdk_match_loss(
                targets.data_ptr(), B, Gt, anc_p, A, C, H, W, stride, 0, J.IOU_MATCH[0], J.IOU_MATCH[1], float(ops.radius),
                conf.data_ptr(), loc.data_ptr(), J.CODES[case.dtype], J.ALPHA, case.gamma, J.BETA, 0, d_conf.data_ptr(),
                d_loc.data_ptr(), sums.data_ptr(), ws.data_ptr(), need, N.stream_ptr(dev))
    N.check(rc, "match_loss")
    torch.cuda.synchronize()
    return gs.problems(), d_conf.clone(), d_loc.clone(), sums.clone()


@pytest.mark.parametrize("cls", ["focal", "multibox"])
@pytest.mark.parametrize("geo", J.GUARD_GEOS)
def test_the_entry_points_stay_inside_their_buffers(geo, cls):
    """d_conf, d_loc, sums and a workspace of exactly the queried size between guard bands; the results do not depend on what the
    workspace held (the two queries and run_match_loss lay the three regions of the multibox workspace out separately)"""
    case = J._case(geo, cls=cls, ratio=3 if cls == "multibox" else None)
    ops = J.operands(case)
    runs = [_abi_call(case, ops, fill) for fill in (0xFF, 0x00)]
    for problems, d_conf, d_loc, sums in runs:
        assert not problems, problems
        assert not G.has_nan(d_conf) and not G.has_nan(d_loc) and not G.has_nan(sums), "an output element was never written"
        assert float(sums[2]) == float(ops.asg.fg)
    for a, b in zip(runs[0][1:], runs[1][1:]):
        assert G.same_bits(a, b), "the result depends on what the workspace held"
    # ... and are what match_loss returns before its backward scales them
    s = J.scale_of(ops.asg)
    import torch
    out = J.Out(runs[0][1].cpu() * torch.tensor(s), runs[0][2].cpu() * torch.tensor(s), float(runs[0][3][0]), float(runs[0][3][1]),
                float(runs[0][3][2]))
    problems = _judge_unrecorded(case, ops, out)
    assert not problems, "\n".join(problems)


def _judge_unrecorded(case, ops, out):
    """(the ratios file holds one line per case of the case lists and quantity: from test_match_loss_passes_the_judge alone)"""
    n = len(J.RECORDS)
    try:
        return J.judge(case, ops, out)
    finally:
        del J.RECORDS[n:]


@pytest.mark.parametrize("cls", ["focal", "multibox"])
@pytest.mark.parametrize("geo", J.EDGE_GEOS)
def test_ground_truth_of_no_row_and_of_257_rows(geo, cls):
    """targets [B, 0, 5] (an empty tensor has no storage to point at) and [B, 257, 5] with at most SSDK_MAX_GT valid rows per image
    (the 257th wins an anchor) give the oracle's answer, through match_loss and through ModelWithLossBasic.forward"""
    import torch
    from ssds.core import criterion
    from ssds.pipeline.pipeline_anchor_ddp import ModelWithLossBasic

    B, Gt, A, C, H, W, stride = J.GEOS[geo]
    case = J._case(geo, dtype="f32", cls=cls, ratio=3 if cls == "multibox" else None)
    ops = J.operands(case)
    assert ops.targets.shape == (B, Gt, 5)
    if Gt > 256:
        import numpy as np
        cut = ops.targets.copy()
        cut[:, 256:, 4] = -1
        assert not np.array_equal(J._oracle(geo, "iou", cut)[1], ops.asg.lt.numpy()), "no row beyond the 256th wins an anchor"
        assert int((ops.targets[:, :, 4] > -1).sum(1).max()) <= 256
    out = run(case, ops)
    problems = _judge_unrecorded(case, ops, out)
    assert not problems, "\n".join(problems)

    class Heads(torch.nn.Module):
        def __init__(self, loc, conf):
            super().__init__()
            self.loc, self.conf = torch.nn.Parameter(loc), torch.nn.Parameter(conf)

        def forward(self, images):
            return [self.loc], [self.conf]

    cc = criterion.FocalLoss(J.ALPHA, 2.0) if cls == "focal" else criterion.MultiBoxLoss(3)
    m = ModelWithLossBasic(Heads(ops.loc.cuda(), ops.conf.cuda()), cc, criterion.SmoothL1Loss(J.BETA), C, ops.match, ops.radius)
    level = collections.OrderedDict([(stride, ops.anchors[stride])])
    cls_loss, loc_loss, _, _ = m(None, torch.from_numpy(ops.targets).cuda(), level)
    fg = max(ops.asg.fg, 1)
    assert float(cls_loss.detach()) == float(torch.tensor(out.cls_sum) / fg)
    assert float(loc_loss.detach()) == float(torch.tensor(out.loc_sum) / fg)


def test_more_valid_rows_than_the_kernels_stage_is_an_error_before_any_launch():
    import torch
    from ssds import _native as N
    from ssds.core.fused_loss import match_loss

    geo = J.EDGE_GEOS[1]
    B, Gt, A, C, H, W, stride = J.GEOS[geo]
    ops = J.operands(J._case(geo, dtype="f32"))
    full = ops.targets.copy()
    full[0, :, 4] = 0  # 257 valid rows in one image
    before = N.last_kernel()
    with pytest.raises(ValueError, match="SSDK_MAX_GT = 256"):
        match_loss(ops.conf.cuda(), ops.loc.cuda(), torch.from_numpy(full).cuda(), ops.anchors, C, stride, ops.match, 0)
    assert N.last_kernel() == before
