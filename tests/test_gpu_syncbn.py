"""Synchronised BatchNorm on the HIP kernels (csrc/ssdk_bntrain.hip, "synchronised BatchNorm"; batchnorm.use_fast_sync_batchnorm).

1. emulated ranks in one process: unequal shards of one batch (one of them empty) through the split entry points, against fp64
   torch on the whole batch (one max-norm per tensor; per channel against derived bars: tests/test_gpu_bntrain.py);
2. one rank IS the local path: the split entry points at W = 1 give the bits of ssdk_bn_act_train_fwd / _stats / _bwd;
3. two real ranks (gloo, both on cuda:0): against torch.nn.SyncBatchNorm and fp64, identical statistics on both ranks, and two
   DDP steps of the training Solver with --sync-bn end with identical replicas;
4. Solver(sync_bn=True) at world size 1 trains on the same kernels as the default (torch takes plain BatchNorm there too);
5. no host synchronisation: the forced split path of a layer captured as a hipGraph replays the eager bits."""
import copy
import os
import socket
import subprocess
import sys

import pytest
import torch

from bnjudge import split_path as _split_path  # (moved there: tests/test_gpu_bntrain.py judges the same path per channel)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = {"float32": 2e-4, "bfloat16": 2e-2, "float16": 4e-3}

_TINY_CFG = """
MODEL:
  SSDS: SSD
  NETS: MobileNetV2
  IMAGE_SIZE: [96, 96]
  NUM_CLASSES: 4
  FEATURE_LAYER: [[5, 7, 'Conv:S'], [96, 320, 64]]
  SIZES: [[2.0, 2.828], [2.0, 2.828], [2.0, 2.828]]
  ASPECT_RATIOS: [[1, 2, 0.5], [1, 2, 0.5], [1, 2, 0.5]]
TRAIN:
  MAX_EPOCHS: 1
  CHECKPOINTS_EPOCHS: 1
  BATCH_SIZE: 2
  TRAINABLE_SCOPE: 'backbone,extras,loc,conf'
  RESUME_SCOPE: ''
  OPTIMIZER:
    OPTIMIZER: sgd
    LEARNING_RATE: 0.01
    MOMENTUM: 0.9
    WEIGHT_DECAY: 0.0001
  LR_SCHEDULER:
    SCHEDULER: exponential
    GAMMA: 0.5
    WARM_UP_EPOCHS: 0
DATASET:
  DATASET: 'synthetic'
EXP_DIR: '%(exp)s'
LOG_DIR: '%(exp)s'
PHASE: ['train']
"""


def _close(a, b, tol, what):
    a, b = a.double(), b.double()
    err = float((a - b).abs().max()) / max(float(b.abs().max()), 1e-6)
    assert err < tol, "%s: rel err %.3g" % (what, err)


def _batch(n, c, h, w, seed):
    """randn * 2 + 3 per channel, channel 0 at mean 50 / std 0.1 (the shards' pivots differ by a few of its std)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, c, h, w, generator=g) * 2 + 3
    x[:, 0] = 50 + 0.1 * torch.randn(n, h, w, generator=g)
    return x, torch.randn(n, c, h, w, generator=g)


def _act_ref(pre, act):
    return pre if act == 0 else (pre.clamp(0, 6) if act == 1 else pre.clamp(min=0))


def _open(y, act):  # the activation's pass-through mask, on the stored output (hardtanh_backward / threshold_backward)
    y = y.double()
    return torch.ones_like(y, dtype=torch.bool) if act == 0 else ((y > 0) & (y < 6) if act == 1 else y > 0)


def _ws(n, c):
    from ssds import _native as N

    need = int(N.lib.ssdk_bn_workspace_bytes(max(n, 1), c))
    return torch.zeros(need, dtype=torch.uint8, device="cuda"), need  # (zero ticket words: include/ssdk.h)


def _ptr(t):
    return t.data_ptr() if t.numel() else None


@pytest.mark.gpu
@pytest.mark.parametrize("h,w", [(32, 32), (19, 19)])
@pytest.mark.parametrize("dtype_name", ["float32", "bfloat16", "float16"])
def test_emulated_ranks_match_fp64_batchnorm_of_the_whole_batch(dtype_name, h, w):
    dtype, tol, c, momentum, eps = getattr(torch, dtype_name), TOL[dtype_name], 5, 0.1, 1e-5
    xc, gc = _batch(11, c, h, w, seed=h)
    x, dy = xc.cuda().to(dtype), gc.cuda().to(dtype)
    gen = torch.Generator().manual_seed(7)
    weight = (torch.rand(c, generator=gen) + 0.5).cuda()
    bias = (torch.randn(c, generator=gen) * 0.3 + 1.0).cuda()
    rm0, rv0 = (torch.randn(c, generator=gen) * 0.2).cuda(), (torch.rand(c, generator=gen) + 0.5).cuda()
    for sizes in ([4, 0, 1, 6], [11]):
        for act in (0, 1, 2):
            shards = list(torch.split(x, sizes))
            dys = list(torch.split(dy, sizes))
            rm, rv = rm0.clone(), rv0.clone()
            got = _split_path([s.contiguous() for s in shards], [d.contiguous() for d in dys], weight, bias, rm, rv, momentum, eps, act)
            # fp64 reference on the whole (rounded) batch
            x64 = x.double().requires_grad_(True)
            rm64, rv64 = rm0.double().clone(), rv0.double().clone()
            w64, b64 = weight.double().requires_grad_(True), bias.double().requires_grad_(True)
            pre = torch.nn.functional.batch_norm(x64, rm64, rv64, w64, b64, True, momentum, eps)
            y_ref = _act_ref(pre, act)
            y = torch.cat(got["y"])
            (pre * (dy.double() * _open(y, act))).sum().backward()  # mask from the stored output, as the kernels do
            what = "%s %s act %d" % (sizes, dtype_name, act)
            _close(y, y_ref, tol, "y " + what)
            mean_ref = x.double().mean((0, 2, 3))
            var_ref = x.double().var((0, 2, 3), unbiased=False)
            _close(got["mean"], mean_ref, 2e-6, "save_mean " + what)
            _close(got["invstd"], 1 / torch.sqrt(var_ref + eps), 2e-4, "save_invstd " + what)
            _close(rm, rm64, 2e-6, "running_mean " + what)
            _close(rv, rv64, 2e-4, "running_var " + what)
            _close(torch.cat(got["dx"]), x64.grad, tol, "dx " + what)
            _close(torch.stack(got["dw"]).sum(0), w64.grad, tol, "dweight " + what)
            _close(torch.stack(got["db"]).sum(0), b64.grad, tol, "dbias " + what)
            if 0 in sizes:  # the empty rank's record: count 0, no gradient
                assert float(got["dw"][1].abs().max()) == 0 and float(got["db"][1].abs().max()) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("dtype_name", ["float32", "bfloat16", "float16"])
@pytest.mark.parametrize("n,c,h,w", [(6, 24, 16, 16), (3, 17, 9, 7)])
def test_one_rank_is_the_local_path_bit_for_bit(n, c, h, w, dtype_name):
    from ssds import _native as N

    L, st = N.lib, N.stream_ptr(torch.device("cuda"))
    dtype, hw, momentum, eps = getattr(torch, dtype_name), h * w, 0.1, 1e-5
    xc, gc = _batch(n, c, h, w, seed=c)
    x, dy = xc.cuda().to(dtype), gc.cuda().to(dtype)
    weight, bias = torch.rand(c, device="cuda") + 0.5, torch.randn(c, device="cuda") + 1
    rm0, rv0 = torch.randn(c, device="cuda") * 0.2, torch.rand(c, device="cuda") + 0.5
    x32 = x.float()
    sums = torch.stack([x32.sum((0, 2, 3)), (x32 * x32).sum((0, 2, 3))], 1).contiguous()  # (a producer's raw sums)
    dc = N.dtype_code(x)
    for use_sums in (False, True):
        for act in (0, 1, 2):
            rm, rv = rm0.clone(), rv0.clone()
            got = _split_path([x], [dy], weight, bias, rm, rv, momentum, eps, act, sums=[sums] if use_sums else None)
            # the local path: forward with apply, forward statistics only, backward
            rm_l, rv_l, y_l = rm0.clone(), rv0.clone(), torch.empty_like(x)
            mean_l, invstd_l = torch.empty(c, device="cuda"), torch.empty(c, device="cuda")
            ws, need = _ws(n, c)
            if use_sums:
                rc = L.ssdk_bn_act_train_fwd_sums(x.data_ptr(), sums.data_ptr(), weight.data_ptr(), bias.data_ptr(), rm_l.data_ptr(),
                                                  rv_l.data_ptr(), y_l.data_ptr(), mean_l.data_ptr(), invstd_l.data_ptr(),
                                                  ws.data_ptr(), need, n, c, hw, momentum, eps, act, dc, st)
            else:
                rc = L.ssdk_bn_act_train_fwd(x.data_ptr(), weight.data_ptr(), bias.data_ptr(), rm_l.data_ptr(), rv_l.data_ptr(),
                                             y_l.data_ptr(), mean_l.data_ptr(), invstd_l.data_ptr(), ws.data_ptr(), need, n, c, hw,
                                             momentum, eps, act, dc, st)
            N.check(rc, "fwd")
            coef_l, m2, i2 = torch.empty(c, 4, device="cuda"), torch.empty(c, device="cuda"), torch.empty(c, device="cuda")
            N.check(L.ssdk_bn_act_train_stats(x.data_ptr(), sums.data_ptr() if use_sums else None, weight.data_ptr(), bias.data_ptr(),
                                              None, None, m2.data_ptr(), i2.data_ptr(), coef_l.data_ptr(), ws.data_ptr(), need, n, c,
                                              hw, momentum, eps, dc, st), "stats")
            dx_l, dw_l, db_l = torch.empty_like(x), torch.empty(c, device="cuda"), torch.empty(c, device="cuda")
            N.check(L.ssdk_bn_act_train_bwd(x.data_ptr(), dy.data_ptr(), weight.data_ptr(), bias.data_ptr(), mean_l.data_ptr(),
                                            invstd_l.data_ptr(), dx_l.data_ptr(), dw_l.data_ptr(), db_l.data_ptr(), ws.data_ptr(),
                                            need, n, c, hw, act, dc, st), "bwd")
            what = "sums %s act %d" % (use_sums, act)
            for name, a, b in (("y", got["y"][0], y_l), ("save_mean", got["mean"], mean_l), ("save_invstd", got["invstd"], invstd_l),
                               ("running_mean", rm, rm_l), ("running_var", rv, rv_l), ("coef", got["coef"][:, :3], coef_l[:, :3]),
                               ("dx", got["dx"][0], dx_l), ("dweight", got["dw"][0], dw_l), ("dbias", got["db"][0], db_l)):
                assert torch.equal(a, b), "%s differs from the local path (%s)" % (name, what)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_main(rank, world, port, out_dir):
    """One rank of the two-rank test (a fresh process; both ranks on cuda:0, gloo)."""
    sys.path[:0] = [ROOT, os.path.join(ROOT, "ssds.pytorch_amd")]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist
    import torch.nn as nn

    from ssds.modeling.layers import batchnorm as B

    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    res = {}
    # (a) one layer (BN + ReLU6 folded), each rank its part of a common batch of 9 (5 | 4)
    c = 6
    xc, gc = _batch(9, c, 13, 13, seed=3)
    lo, hi = (0, 5) if rank == 0 else (5, 9)
    for dtype_name in ("float32", "bfloat16"):
        dtype = getattr(torch, dtype_name)
        torch.manual_seed(0)
        fast = nn.Sequential(nn.BatchNorm2d(c), nn.ReLU6())
        fast[0].weight.data.uniform_(0.5, 1.5)
        fast[0].bias.data.normal_(1.0, 0.3)
        ref = nn.SyncBatchNorm.convert_sync_batchnorm(copy.deepcopy(fast)).cuda().train()
        B.use_fast_sync_batchnorm(fast)
        assert B.fuse_bn_activations(fast) == 1
        fast = fast.cuda().train()
        x = xc[lo:hi].cuda().to(dtype).requires_grad_(True)
        y = fast(x)
        y.backward(gc[lo:hi].cuda().to(dtype))
        out = dict(y=y.detach().float().cpu(), dx=x.grad.float().cpu(), dw=fast[0].weight.grad.cpu(), db=fast[0].bias.grad.cpu(),
                   rm=fast[0].running_mean.cpu(), rv=fast[0].running_var.cpu())
        if dtype_name == "float32":  # torch's SyncBatchNorm on the same shards (fp32 only)
            xr = xc[lo:hi].cuda().requires_grad_(True)
            yr = ref(xr)
            yr.backward(gc[lo:hi].cuda())
            out.update(ref_y=yr.detach().cpu(), ref_dx=xr.grad.cpu(), ref_dw=ref[0].weight.grad.cpu(), ref_db=ref[0].bias.grad.cpu(),
                       ref_rm=ref[0].running_mean.cpu(), ref_rv=ref[0].running_var.cpu())
        xs = xc[lo:hi].cuda().to(dtype).contiguous()
        bn = fast[0]
        mean, invstd, _, _ = B._sync_forward_stats(xs, bn.weight, bn.bias, bn.running_mean.clone(), bn.running_var.clone(), 0.1,
                                                   bn.eps, None, None, world)
        out.update(mean=mean.cpu(), invstd=invstd.cpu())
        res[dtype_name] = out
    # (b) the training Solver with --sync-bn under DDP (gloo on cuda:0), two steps of a tiny configuration
    from ssds.core import config
    from ssds.dataset.synthetic import SyntheticDetectionLoader
    from ssds.modeling import model_builder
    from ssds.pipeline.pipeline_anchor_ddp import train_step
    from ssds.utils.train_ddp import Solver

    cfg_path = os.path.join(out_dir, "tiny%d.yml" % rank)
    with open(cfg_path, "w") as f:
        f.write(_TINY_CFG % {"exp": os.path.join(out_dir, "exp%d" % rank)})
    cfg = config.cfg_from_file(cfg_path)
    torch.manual_seed(0)
    dev = torch.device("cuda", 0)
    solver = Solver(cfg, 0, dev, steps_per_epoch=2, sync_bn=True)
    syncs = [m for m in solver.model.modules() if type(m) is B.FastBatchNorm2d and m._ssdk_sync]
    assert len(syncs) > 30
    mwl = solver.wrap()
    assert type(mwl).__name__ == "DistributedDataParallel"
    inner = mwl.module.model
    anchors = model_builder.create_anchors(cfg.MODEL, inner, cfg.MODEL.IMAGE_SIZE)
    loader = SyntheticDetectionLoader(2, cfg.MODEL.IMAGE_SIZE, cfg.MODEL.NUM_CLASSES, 2, dev, seed=1234 + rank)
    for images, targets in loader:
        c_, l_, _ = train_step(mwl, images, targets, anchors, solver.optimizer)
    torch.cuda.synchronize()
    res["params"] = torch.cat([p.detach().float().flatten() for p in inner.parameters()]).cpu()
    res["stats"] = torch.cat([b.detach().float().flatten() for n, b in inner.named_buffers() if "running" in n]).cpu()
    res["loss_finite"] = bool(torch.isfinite(c_ + l_))
    torch.save(res, os.path.join(out_dir, "rank%d.pt" % rank))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_two_ranks_on_one_gpu_match_torch_syncbatchnorm_and_stay_identical(tmp_path):
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
    r0, r1 = (torch.load(os.path.join(str(tmp_path), "rank%d.pt" % r)) for r in range(world))
    xc, gc = _batch(9, 6, 13, 13, seed=3)
    for dtype_name in ("float32", "bfloat16"):
        a, b = r0[dtype_name], r1[dtype_name]
        assert torch.equal(a["mean"], b["mean"]) and torch.equal(a["invstd"], b["invstd"]), "ranks merged different statistics"
        assert torch.equal(a["rm"], b["rm"]) and torch.equal(a["rv"], b["rv"])
        tol = TOL[dtype_name]
        # the fp64 BatchNorm (+ ReLU6) of the full batch
        dtype = getattr(torch, dtype_name)
        x64 = xc.to(dtype).double().requires_grad_(True)
        torch.manual_seed(0)
        bn = torch.nn.BatchNorm2d(6)
        bn.weight.data.uniform_(0.5, 1.5)
        bn.bias.data.normal_(1.0, 0.3)
        bn = bn.double()
        pre = bn(x64)
        y_all = torch.cat([a["y"], b["y"]])
        (pre * (gc.to(dtype).double() * _open(y_all, 1))).sum().backward()
        what = " (%s)" % dtype_name
        _close(y_all, pre.clamp(0, 6), tol, "y" + what)
        _close(torch.cat([a["dx"], b["dx"]]), x64.grad, tol, "dx" + what)
        _close(a["dw"] + b["dw"], bn.weight.grad, tol, "dweight (sum over ranks)" + what)
        _close(a["db"] + b["db"], bn.bias.grad, tol, "dbias (sum over ranks)" + what)
        _close(a["rm"], bn.running_mean, 2e-6, "running_mean" + what)
        _close(a["rv"], bn.running_var, 2e-4, "running_var" + what)
        _close(a["mean"], xc.to(dtype).double().mean((0, 2, 3)), 2e-6, "save_mean" + what)
        if dtype_name == "float32":  # torch.nn.SyncBatchNorm in the same group, rank by rank
            for r in (a, b):
                for k in ("y", "dx", "dw", "db", "rm", "rv"):
                    ref = r["ref_" + k]
                    if k == "y":
                        ref = ref.clamp(0, 6)
                    _close(r[k], ref, tol, "%s vs torch.nn.SyncBatchNorm" % k)
    assert r0["loss_finite"] and r1["loss_finite"]
    assert torch.equal(r0["params"], r1["params"]), "DDP replicas diverged under --sync-bn"
    assert torch.equal(r0["stats"], r1["stats"]), "running statistics differ between the ranks"


def _solver_step(tmp_path, sync_bn, images, targets):
    from ssds.core import config
    from ssds.modeling import model_builder
    from ssds.pipeline.pipeline_anchor_ddp import train_step
    from ssds.utils.train_ddp import Solver

    cfg_path = tmp_path / "tiny.yml"
    cfg_path.write_text(_TINY_CFG % {"exp": str(tmp_path / ("exp%d" % sync_bn))})
    cfg = config.cfg_from_file(str(cfg_path))
    torch.manual_seed(0)
    solver = Solver(cfg, 0, torch.device("cuda", 0), steps_per_epoch=1, sync_bn=sync_bn)
    mwl = solver.wrap()
    inner = mwl.model
    anchors = model_builder.create_anchors(cfg.MODEL, inner, cfg.MODEL.IMAGE_SIZE)
    c, l, _ = train_step(mwl, images, targets, anchors, solver.optimizer)
    torch.cuda.synchronize()
    grads = torch.cat([p.grad.float().flatten() for p in inner.parameters() if p.grad is not None])
    stats = torch.cat([b.float().flatten() for n, b in inner.named_buffers() if "running" in n])
    return inner, torch.stack([c.float(), l.float()]), grads, stats


@pytest.mark.gpu
def test_sync_bn_at_one_rank_trains_on_the_same_kernels(tmp_path):
    from ssds.dataset.synthetic import SyntheticDetectionLoader
    from ssds.modeling.layers.batchnorm import FastBatchNorm2d

    images, targets = SyntheticDetectionLoader(2, (96, 96), 4, 1, torch.device("cuda"), seed=5).batch()
    m_sync, loss_s, grads_s, stats_s = _solver_step(tmp_path, True, images, targets)
    m_loc, loss_l, grads_l, stats_l = _solver_step(tmp_path, False, images, targets)
    _, loss_l2, grads_l2, stats_l2 = _solver_step(tmp_path, False, images, targets)
    assert all(type(m) is FastBatchNorm2d for m in m_sync.modules() if isinstance(m, torch.nn.modules.batchnorm._BatchNorm))
    for what, s, l, l2 in (("loss", loss_s, loss_l, loss_l2), ("running statistics", stats_s, stats_l, stats_l2),
                           ("gradients", grads_s, grads_l, grads_l2)):
        if torch.equal(l, l2):  # the step is bit-reproducible: so is --sync-bn against it
            assert torch.equal(s, l), what
        else:  # (a kernel with atomics in the step: the twin's own scatter is the bar)
            assert float((s - l).abs().max()) <= 2 * float((l2 - l).abs().max()), what


@pytest.mark.gpu
@pytest.mark.parametrize("dtype_name", ["float32", "bfloat16"])
def test_forced_split_path_captures_as_a_graph_and_replays_the_eager_bits(dtype_name):
    import torch.nn as nn

    from ssds.modeling.layers.batchnorm import fuse_bn_activations, use_fast_sync_batchnorm

    dtype = getattr(torch, dtype_name)
    torch.manual_seed(0)
    layer = nn.Sequential(nn.BatchNorm2d(24), nn.ReLU6())
    layer[0].weight.data.uniform_(0.5, 1.5)
    layer[0].bias.data.normal_(1.0, 0.5)
    use_fast_sync_batchnorm(layer)
    assert fuse_bn_activations(layer) == 1
    layer = layer.cuda().train()
    layer[0]._ssdk_force_sync = True
    xc, gc = _batch(4, 24, 19, 19, seed=9)
    x = xc.cuda().to(dtype).requires_grad_(True)
    g = gc.cuda().to(dtype)
    state = copy.deepcopy(layer.state_dict())

    def step():
        x.grad = None
        layer[0].weight.grad = layer[0].bias.grad = None
        y = layer(x)
        y.backward(g)
        return y

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y_g = step()
    grads_g = [x.grad, layer[0].weight.grad, layer[0].bias.grad]  # (the captured step's own tensors)
    layer.load_state_dict(state)
    y_e = step().detach().clone()
    eager = [y_e, x.grad.clone(), layer[0].weight.grad.clone(), layer[0].bias.grad.clone(), layer[0].running_mean.clone(),
             layer[0].running_var.clone()]
    layer.load_state_dict(state)  # (in place: the graph's buffers are the module's)
    graph.replay()
    torch.cuda.synchronize()
    replayed = [y_g] + grads_g + [layer[0].running_mean, layer[0].running_var]
    for name, a, b in zip(("y", "dx", "dweight", "dbias", "running_mean", "running_var"), replayed, eager):
        assert torch.equal(a, b), name


if __name__ == "__main__" and len(sys.argv) == 6 and sys.argv[1] == "--rank":
    _rank_main(int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), sys.argv[5])
