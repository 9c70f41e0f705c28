"""The N > 1 path on CPU: two processes, ``gloo`` backend, 127.0.0.1 rendezvous.

Checks the data-parallel semantics of the training step (ssds/pipeline/pipeline_anchor_ddp.py):
* replicas start identical (rank-0 broadcast) and stay identical after optimiser steps;
* the gradient every rank applies is the MEAN over ranks of the local gradients (Apex DDP / torch DDP
  averaging; each rank normalises its loss by its LOCAL foreground count like the reference);
* a non-finite loss on ONE rank makes EVERY rank skip the step (collective decision), nobody hangs.

Target assignment is a HIP kernel with no CPU path; here (test infrastructure only) it is substituted by
the numpy oracle so that the step can run without a GPU."""
import os
import socket
import sys
from collections import OrderedDict

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _oracle_extract_targets(targets, anchors, classes, stride, size, match=(0.5, 0.4), radius=0, is_centerness=False):
    from oracle import box_oracle as O

    anc = OrderedDict((k, v.numpy() if torch.is_tensor(v) else v) for k, v in anchors.items())
    out = O.extract_targets(targets.detach().cpu().numpy(), anc, classes, stride, tuple(size),
                            tuple(float(m) for m in match), radius)
    return tuple(torch.from_numpy(np.ascontiguousarray(o)) for o in out)


def _build(seed):
    from ssds.core import criterion
    from ssds.modeling import nets, ssds
    from ssds.pipeline.pipeline_anchor_ddp import ModelWithLossBasic

    torch.manual_seed(seed)
    o, e, h = ssds.SSD.add_extras([[5, 7, "Conv:S"], [96, 320, 64]], [2, 2, 2], 3)
    model = ssds.SSD(nets.MobileNetV2(outputs=o), e, h, 3)
    return ModelWithLossBasic(model, criterion.FocalLoss(), criterion.SmoothL1Loss(), 3, [0.5, 0.4], 0)


def _batch(rank, step):
    g = torch.Generator().manual_seed(100 + 10 * rank + step)
    images = torch.rand((2, 3, 64, 64), generator=g)
    t = torch.full((2, 3, 5), -1.0)
    for b in range(2):
        for j in range(1 + (b + rank) % 3):
            x, y = torch.rand(2, generator=g) * 30
            w, h = 16 + torch.rand(2, generator=g) * 30
            t[b, j] = torch.tensor([float(x.floor()), float(y.floor()), float(w.ceil()), float(h.ceil()),
                                    float(torch.randint(0, 3, (1,), generator=g))])
    return images, t


def _worker(rank, world, port, out_dir):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "ssds.pytorch_amd")]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from torch.nn.parallel import DistributedDataParallel as DDP

    from ssds.modeling import model_builder  # noqa: F401
    from ssds.modeling.layers import box
    from ssds.pipeline import pipeline_anchor_ddp as P

    box.extract_targets = _oracle_extract_targets  # test substitution (no GPU here)
    mwl = _build(seed=rank)  # different init per rank: DDP must broadcast rank 0's
    ddp = DDP(mwl, bucket_cap_mb=1)
    ref = _build(seed=0)
    same_init = all(torch.equal(a, b) for a, b in zip(ddp.module.state_dict().values(), ref.state_dict().values()))
    anchors = OrderedDict((s, box.generate_anchors(s, [1], [2.0, 2.828])) for s in (16, 32, 64))
    opt = torch.optim.SGD(ddp.parameters(), lr=0.05, momentum=0.9)

    # local gradient without DDP (same weights), to verify the averaging
    images, targets = _batch(rank, 0)
    local = _build(seed=0)
    local.load_state_dict(ddp.module.state_dict())
    local.train()
    c, l, _, _ = local(images, targets, anchors)
    (c + l).backward()
    local_grads = torch.cat([p.grad.flatten() for p in local.parameters() if p.grad is not None])
    gathered = [torch.zeros_like(local_grads) for _ in range(world)]
    dist.all_gather(gathered, local_grads)
    mean_grads = torch.stack(gathered).mean(0)

    ddp.train()
    opt.zero_grad()
    c, l, _, _ = ddp(images, targets, anchors)
    (c + l).backward()
    ddp_grads = torch.cat([p.grad.flatten() for p in ddp.parameters() if p.grad is not None])
    grad_err = float((ddp_grads - mean_grads).abs().max() / (mean_grads.abs().max() + 1e-12))

    # two real steps through train_step
    for step in (1, 2):
        images, targets = _batch(rank, step)
        c, l, skipped = P.train_step(ddp, images, targets, anchors, opt, autocast_dtype=None)
        assert not skipped and torch.isfinite(c) and torch.isfinite(l)
    after_steps = torch.cat([p.detach().flatten() for p in ddp.parameters()])
    g2 = [torch.zeros_like(after_steps) for _ in range(world)]
    dist.all_gather(g2, after_steps)
    replicas_equal = all(torch.equal(g2[0], t) for t in g2)

    # NaN on rank 1 only -> every rank skips
    images, targets = _batch(rank, 3)
    if rank == 1:
        images[0, 0, 0, 0] = float("nan")
    c, l, skipped = P.train_step(ddp, images, targets, anchors, opt, autocast_dtype=None)
    after_skip = torch.cat([p.detach().flatten() for p in ddp.parameters()])
    unchanged = bool(torch.equal(after_skip, after_steps))
    torch.save(dict(same_init=same_init, grad_err=grad_err, replicas_equal=replicas_equal, skipped=bool(skipped),
                    unchanged=unchanged, moved=float((after_steps - torch.cat([p.flatten() for p in ref.parameters()])).abs().max())),
               os.path.join(out_dir, "rank%d.pt" % rank))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_ddp_two_ranks_gloo(tmp_path):
    world, port = 2, _free_port()
    mp.start_processes(_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True, start_method="spawn")
    for r in range(world):
        res = torch.load(os.path.join(str(tmp_path), "rank%d.pt" % r))
        assert res["same_init"], "rank-0 parameters were not broadcast"
        assert res["grad_err"] < 1e-5, res
        assert res["replicas_equal"], "replicas diverged"
        assert res["moved"] > 0, "optimizer never stepped"
        assert res["skipped"] and res["unchanged"], "NaN on one rank must skip the step on every rank"


def test_synthetic_loader_contract():
    from ssds.dataset.synthetic import SyntheticDetectionLoader

    ld = SyntheticDetectionLoader(4, (64, 96), 80, steps=2, device=torch.device("cpu"), max_gt=8)
    batches = list(ld)
    assert len(batches) == 2
    images, t = batches[0]
    assert tuple(images.shape) == (4, 3, 64, 96) and tuple(t.shape) == (4, 8, 5)
    valid = t[..., 4] > -1
    assert valid.any() and (~valid).any()
    assert bool((t[~valid] == -1).all())
    v = t[valid]
    assert bool((v[:, 0] >= 0).all() and (v[:, 0] + v[:, 2] <= 96 + 1).all() and (v[:, 1] + v[:, 3] <= 64 + 1).all())
    assert bool(((v[:, 4] >= 0) & (v[:, 4] < 80)).all())


def test_optimizer_scopes():
    from ssds.core import config, optimizer

    mwl = _build(0)
    groups = optimizer.trainable_param(mwl.model, "backbone,extras;loc,conf")
    assert len(groups) == 2 and all(p.requires_grad for g in groups for p in g)
    with pytest.raises(ValueError, match="is not in the model"):
        optimizer.trainable_param(mwl.model, "base,norm")  # the reference default scope names nothing real
    config.reset_cfg()
    opt = optimizer.configure_optimizer(optimizer.trainable_param(mwl.model, ""), config.cfg.TRAIN.OPTIMIZER)
    assert isinstance(opt, torch.optim.SGD)
    sch = optimizer.configure_lr_scheduler(opt, config.cfg.TRAIN.LR_SCHEDULER)
    assert sch is not None


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
  MAX_EPOCHS: 2
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


def _main_worker(rank, world, port, cfg_path, out_dir):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "ssds.pytorch_amd")]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank), SSDK_FAST_BN="0")
    torch.set_num_threads(1)
    # main() takes RCCL and cuda:<local_rank> whenever a device is visible: on a one-GPU machine rank 1 would ask for a
    # second device.  This is the CPU / gloo launch on every machine, GPU or not.
    torch.cuda.is_available = lambda: False
    from ssds.modeling.layers import box
    from ssds.utils import train_ddp

    box.extract_targets = _oracle_extract_targets  # test substitution (no GPU here)
    seen = {}
    wrap = train_ddp.Solver.wrap

    def spy(self):  # remember the solver so that the test can look at what main() did
        seen["solver"] = self
        seen["mwl"] = wrap(self)
        return seen["mwl"]

    train_ddp.Solver.wrap = spy
    torch.manual_seed(10 + rank)  # different init per rank: DDP must broadcast rank 0's
    train_ddp.main(["-cfg", cfg_path, "--steps", "3", "--epochs", "1"])
    s = seen["solver"]
    inner = seen["mwl"].module.model
    flat = torch.cat([p.detach().flatten() for p in inner.parameters()])
    torch.save(dict(flat=flat, lr=s.optimizer.param_groups[0]["lr"], start_epoch=s.start_epoch,
                    is_ddp=type(seen["mwl"]).__name__), os.path.join(out_dir, "main_rank%d.pt" % rank))


@pytest.mark.timeout(900)
def test_train_ddp_main_end_to_end_two_ranks_gloo(tmp_path):
    """ssds.utils.train_ddp.main (reference train_ddp.py:36-121, 193-220: Solver, DDP wrap, epoch loop, checkpoint on
    rank 0, scheduler step) run as it is launched -- argv, env:// rendezvous, world_size 2 -- on the CPU with gloo.
    Checked: both ranks end with identical parameters, rank 0 alone wrote the reference-format checkpoint + index,
    the scheduler stepped, and a second launch RESUMES from that checkpoint (start_epoch 1) and writes epoch 2."""
    from ssds.core import checkpoint

    exp = tmp_path / "exp"
    cfg_path = tmp_path / "tiny.yml"
    cfg_path.write_text(_TINY_CFG % {"exp": str(exp)})
    world = 2
    mp.start_processes(_main_worker, args=(world, _free_port(), str(cfg_path), str(tmp_path)), nprocs=world, join=True,
                       start_method="spawn")
    r0, r1 = (torch.load(os.path.join(str(tmp_path), "main_rank%d.pt" % r)) for r in range(world))
    assert r0["is_ddp"] == "DistributedDataParallel"
    assert torch.equal(r0["flat"], r1["flat"]), "replicas diverged"
    assert abs(r0["lr"] - 0.005) < 1e-9, "the scheduler did not step once (exponential, gamma 0.5)"
    assert r0["start_epoch"] == 0
    epochs, paths = checkpoint.find_previous_checkpoint(str(exp))
    assert epochs == [1] and os.path.basename(paths[0]) == "SSD_MobileNetV2_synthetic_epoch_1.pth"  # config.py prefix rule
    sd = torch.load(paths[0])
    assert all(not k.startswith("module.") for k in sd) and any(k.startswith("backbone.") for k in sd)
    saved = torch.cat([sd[k].flatten() for k in sd if not k.endswith(("running_mean", "running_var", "num_batches_tracked"))])
    assert saved.numel() == r0["flat"].numel() and torch.equal(saved, r0["flat"]), "rank 0 saved other weights"
    # second launch: resumes epoch 1, trains epoch 2
    mp.start_processes(_main_worker, args=(world, _free_port(), str(cfg_path), str(tmp_path)), nprocs=world, join=True,
                       start_method="spawn")
    r0b = torch.load(os.path.join(str(tmp_path), "main_rank0.pt"))
    assert r0b["start_epoch"] == 1
    assert checkpoint.find_previous_checkpoint(str(exp))[0] == [1, 2]
    assert not torch.equal(r0b["flat"], r0["flat"])


def _json_lines(text):
    import json

    out = []
    for ln in text.splitlines():
        ln = ln.strip()
        if ln.startswith("{") and ln.endswith("}"):
            try:
                out.append(json.loads(ln))
            except ValueError:
                pass
    return out


@pytest.mark.timeout(600)
def test_bench_py_gpus_2_rank_logic_under_gloo():
    """`python bench.py --gpus 2` with no launcher: re-executes itself under torch.distributed.run with 2 ranks on
    127.0.0.1 (bench.relaunch_under_torchrun), reads RANK / WORLD_SIZE / MASTER_* from the env, brackets exactly K steps
    with barriers, takes the MAX over ranks and prints ONE JSON line on rank 0 -- exercised here on CPU under gloo with
    the stub step of --stub-cpu (rank r sleeps 2 (r + 1) ms per step).  No N > 1 GPU number exists in this repository;
    this test is why the first 8-GPU run can be `bench.py --gpus 8` unchanged."""
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "5", "--warmup", "1",
                        "--batch", "64", "--stub-cpu", "1"], env=env, capture_output=True, text=True, timeout=500)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = _json_lines(r.stdout)
    assert len(lines) == 1, "exactly one JSON line (rank 0 only): %r" % r.stdout
    j = lines[0]
    assert j["n_gpus"] == 2 and j["steps"] == 5 and j["warmup"] == 1 and j["scaling"] == "weak" and j["data"] == "stub"
    assert j["config"]["global_batch"] == 128
    assert j["ms_per_step"] >= 4.0, "the slower rank (4 ms per step) bounds the step: MAX over ranks"
    assert abs(j["value"] - 2 * 64 * 5 / (j["ms_per_step"] * 5e-3)) / j["value"] < 1e-3  # whole-job rate over all ranks
    # the driver's own launch line (a launcher is present: no re-exec)
    port = _free_port()
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.join(root, "bench.py"),
                        "--gpus", "2", "--steps", "3", "--warmup", "1", "--stub-cpu", "1"], env=env, capture_output=True,
                       text=True, timeout=500)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = _json_lines(r.stdout)
    assert len(lines) == 1 and lines[0]["n_gpus"] == 2 and lines[0]["steps"] == 3


@pytest.mark.timeout(900)
def test_bench_train_py_gpus_2_under_gloo():
    """tools/bench_train.py --gpus 2 (self-spawn under torch.distributed.run) with --cpu 1: the script's launcher / env /
    barrier / MAX-over-ranks / rank-0-print logic on two gloo ranks with a stub step (sleep + a real all-reduce; the
    training step itself needs a HIP device and is covered by test_train_ddp_main_end_to_end_two_ranks_gloo with the
    oracle substituted for the target kernel): one JSON line, n_gpus = 2, the slower rank bounds the step."""
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    env["OMP_NUM_THREADS"] = "2"
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "bench_train.py"), "--gpus", "2", "--steps", "2",
                        "--warmup", "1", "--batch", "2", "--size", "128", "--cpu", "1"], env=env, capture_output=True,
                       text=True, timeout=800)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = _json_lines(r.stdout)
    assert len(lines) == 1, r.stdout
    j = lines[0]
    assert j["n_gpus"] == 2 and j["batch_per_gpu"] == 2 and j["data"].startswith("stub")
    assert j["ms_per_step"] >= 4.0 and abs(j["value"] - 2 * 2 * 2 / (j["ms_per_step"] * 2e-3)) / j["value"] < 2e-2
