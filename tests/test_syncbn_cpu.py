"""Synchronised BatchNorm (``--sync-bn``) on the kernel-backed layers, the parts that need no GPU: the module conversion
(``batchnorm.use_fast_sync_batchnorm``) keeps the state and every fusion, the CPU / eval forward is plain BatchNorm, the
training Solver picks the sync layers, and the new C entry points (csrc/ssdk_bntrain.hip, "synchronised BatchNorm") refuse bad
arguments with an error code and a message.  The kernels themselves: tests/test_gpu_syncbn.py."""
import copy
import ctypes
import os

import pytest
import torch
import torch.nn as nn

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


def _model(seed=0):
    from ssds.modeling import nets, ssds

    torch.manual_seed(seed)
    o, e, h = ssds.SSD.add_extras([[5, 7, "Conv:S"], [96, 320, 64]], [2, 2, 2], 3)
    return ssds.SSD(nets.MobileNetV2(outputs=o), e, h, 3)


def _fuse_all(model):
    from ssds.modeling.layers.batchnorm import fuse_bn_activations, fuse_bn_into_depthwise
    from ssds.modeling.layers.pointwise import fuse_conv_bn_statistics, use_pointwise_gemm

    use_pointwise_gemm(model)
    return fuse_bn_activations(model), fuse_bn_into_depthwise(model), fuse_conv_bn_statistics(model)


def _bns(model):
    return [m for m in model.modules() if isinstance(m, nn.modules.batchnorm._BatchNorm)]


def test_use_fast_sync_batchnorm_converts_in_place_and_keeps_the_state():
    from ssds.modeling.layers.batchnorm import FastBatchNorm2d, use_fast_sync_batchnorm

    model = _model()
    for i, m in enumerate(_bns(model)):  # statistics that are not the initial ones
        m.running_mean.uniform_(-1, 1)
        m.running_var.uniform_(0.5, 2)
        m.num_batches_tracked.fill_(i)
    before = copy.deepcopy(model.state_dict())
    n = len(_bns(model))
    assert n > 30 and all(type(m) is nn.BatchNorm2d for m in _bns(model))
    assert use_fast_sync_batchnorm(model) is model
    bns = _bns(model)
    assert len(bns) == n and all(type(m) is FastBatchNorm2d and m._ssdk_sync and m.process_group is None for m in bns)
    after = model.state_dict()
    assert list(after) == list(before)
    assert all(torch.equal(after[k], before[k]) for k in before)


def test_use_fast_sync_batchnorm_takes_a_model_that_torch_converted_and_its_group():
    from ssds.modeling.layers.batchnorm import FastBatchNorm2d, use_fast_sync_batchnorm

    model = nn.SyncBatchNorm.convert_sync_batchnorm(_model(), process_group="group-A")  # (any object: it is only carried)
    sd = copy.deepcopy(model.state_dict())
    assert all(type(m) is nn.SyncBatchNorm for m in _bns(model))
    use_fast_sync_batchnorm(model)
    assert all(type(m) is FastBatchNorm2d and m._ssdk_sync and m.process_group == "group-A" for m in _bns(model))
    assert all(torch.equal(model.state_dict()[k], v) for k, v in sd.items())
    use_fast_sync_batchnorm(model, process_group="group-B")  # an explicit group wins
    assert all(m.process_group == "group-B" for m in _bns(model))
    # layers the kernels cannot serve stay synchronised on torch's module
    seq = nn.Sequential(nn.BatchNorm2d(4, affine=False), nn.BatchNorm2d(4, track_running_stats=False), nn.BatchNorm2d(4))
    use_fast_sync_batchnorm(seq)
    assert [type(m) for m in seq] == [nn.SyncBatchNorm, nn.SyncBatchNorm, FastBatchNorm2d]


def test_the_fusions_find_the_same_pairs_on_the_sync_model():
    from ssds.modeling.layers.batchnorm import use_fast_batchnorm, use_fast_sync_batchnorm

    local = use_fast_batchnorm(_model())
    sync = use_fast_sync_batchnorm(_model())
    pairs_local, pairs_sync = _fuse_all(local), _fuse_all(sync)
    assert all(p > 0 for p in pairs_local)
    assert pairs_sync == pairs_local
    assert sum(1 for m in sync.modules() if "_ssdk_defer_to" in m.__dict__) == pairs_local[1]


@pytest.mark.parametrize("affine", [True, False])
def test_cpu_and_eval_forward_is_plain_batchnorm(affine):
    from ssds.modeling.layers.batchnorm import use_fast_sync_batchnorm

    torch.manual_seed(1)
    ref = nn.Sequential(nn.Conv2d(3, 8, 1), nn.BatchNorm2d(8, affine=affine), nn.ReLU6())
    if affine:
        ref[1].weight.data.uniform_(0.5, 1.5)
        ref[1].bias.data.normal_(0, 0.3)
    sync = use_fast_sync_batchnorm(copy.deepcopy(ref))
    sync[1]._ssdk_force_sync = True  # (the split path needs a HIP tensor: on the CPU it is never taken)
    x = torch.randn(5, 3, 7, 9) * 2 + 1
    for train in (True, False):
        ref.train(train)
        sync.train(train)
        assert torch.equal(sync(x), ref(x))
        assert torch.equal(sync[1].running_mean, ref[1].running_mean) and torch.equal(sync[1].running_var, ref[1].running_var)


def _solver(tmp_path, sync_bn, monkeypatch, fast_bn="1"):
    from ssds.core import config
    from ssds.utils import train_ddp

    monkeypatch.setenv("SSDK_FAST_BN", fast_bn)
    cfg_path = tmp_path / "tiny.yml"
    cfg_path.write_text(_TINY_CFG % {"exp": str(tmp_path / "exp")})
    cfg = config.cfg_from_file(str(cfg_path))
    return train_ddp.Solver(cfg, 0, torch.device("cpu"), steps_per_epoch=1, sync_bn=sync_bn)


def test_solver_sync_bn_takes_the_sync_kernel_layers(tmp_path, monkeypatch):
    from ssds.modeling.layers.batchnorm import FastBatchNorm2d

    sync = _solver(tmp_path, True, monkeypatch).model
    local = _solver(tmp_path, False, monkeypatch).model
    sb, lb = _bns(sync), _bns(local)
    assert len(sb) == len(lb) > 30
    assert all(type(m) is FastBatchNorm2d and m._ssdk_sync for m in sb)
    assert not any(m._ssdk_sync for m in lb)
    # the fusions are on exactly as on the local model: folded activations, deferred BatchNorms, producer statistics
    assert [m._ssdk_act for m in sb] == [m._ssdk_act for m in lb] and any(m._ssdk_act for m in sb)
    assert ["_ssdk_defer_to" in m.__dict__ for m in sb] == ["_ssdk_defer_to" in m.__dict__ for m in lb]
    follows = lambda model: [bool(getattr(m, "_ssdk_bn_follows", False)) for m in model.modules()]  # noqa: E731
    assert follows(sync) == follows(local) and any(follows(sync))


def test_solver_sync_bn_without_the_kernels_is_torch_syncbatchnorm(tmp_path, monkeypatch):
    bns = _bns(_solver(tmp_path, True, monkeypatch, fast_bn="0").model)
    assert bns and all(type(m) is nn.SyncBatchNorm for m in bns)


def test_sync_entry_points_refuse_bad_arguments():
    from ssds import _native as N

    lib = N.lib
    buf = (ctypes.c_float * 1024)()
    p = ctypes.addressof(buf)
    aligned = (p + 15) & ~15
    ws = ctypes.create_string_buffer(1 << 16)
    wp = (ctypes.addressof(ws) + 15) & ~15

    def refused(rc, what):
        assert rc == -1, rc
        assert what.encode() in lib.ssdk_last_error(), lib.ssdk_last_error()

    # local statistics: bad shape / dtype, null record, null x, too small a workspace
    refused(lib.ssdk_bn_sync_local_stats(aligned, None, aligned, wp, 4096, 2, 0, 4, 0, None), "bn_sync_local_stats")
    refused(lib.ssdk_bn_sync_local_stats(aligned, None, aligned, wp, 4096, 2, 4, 4, 7, None), "bn_sync_local_stats")
    refused(lib.ssdk_bn_sync_local_stats(aligned, None, None, wp, 4096, 2, 4, 4, 0, None), "bn_sync_local_stats")
    refused(lib.ssdk_bn_sync_local_stats(None, None, aligned, wp, 4096, 2, 4, 4, 0, None), "bn_sync_local_stats")
    refused(lib.ssdk_bn_sync_local_stats(aligned, None, aligned, wp, 4, 2, 4, 4, 0, None), "bn_sync_local_stats")
    refused(lib.ssdk_bn_sync_local_stats(aligned, None, aligned, wp, 4096, 1 << 20, 4, 1 << 13, 0, None), "bn_sync_local_stats")
    # merge: W < 1, null gathered, misaligned coef, one running buffer without the other
    args = lambda W, g, coef, rm, rv: (g, W, None, None, rm, rv, aligned, aligned, coef, 4, 0.1, 1e-5, None)  # noqa: E731
    refused(lib.ssdk_bn_sync_fwd_finalize(*args(0, aligned, aligned, None, None)), "bn_sync_fwd_finalize")
    refused(lib.ssdk_bn_sync_fwd_finalize(*args(2, None, aligned, None, None)), "bn_sync_fwd_finalize")
    refused(lib.ssdk_bn_sync_fwd_finalize(*args(2, aligned, aligned + 4, None, None)), "bn_sync_fwd_finalize")
    refused(lib.ssdk_bn_sync_fwd_finalize(*args(2, aligned, aligned, aligned, None)), "bn_sync_fwd_finalize")
    # apply from coef: bad act, misaligned coef
    refused(lib.ssdk_bn_act_apply(aligned, aligned, aligned, 2, 4, 4, 3, 0, None), "bn_act_apply")
    refused(lib.ssdk_bn_act_apply(aligned, aligned + 4, aligned, 2, 4, 4, 1, 0, None), "bn_act_apply")
    # backward halves: null record, bad act, W < 1, null forward records
    refused(lib.ssdk_bn_sync_bwd_local(aligned, aligned, None, None, aligned, aligned, None, None, None, wp, 4096, 2, 4, 4, 0, 0,
                                       None), "bn_sync_bwd_local")
    refused(lib.ssdk_bn_sync_bwd_local(aligned, aligned, None, None, aligned, aligned, aligned, None, None, wp, 4096, 2, 4, 4, 5, 0,
                                       None), "bn_sync_bwd_local")
    refused(lib.ssdk_bn_sync_bwd_apply(aligned, aligned, aligned, 0, aligned, None, None, aligned, aligned, aligned, 2, 4, 4, 0, 0,
                                       None), "bn_sync_bwd_apply")
    refused(lib.ssdk_bn_sync_bwd_apply(aligned, aligned, aligned, 2, None, None, None, aligned, aligned, aligned, 2, 4, 4, 0, 0,
                                       None), "bn_sync_bwd_apply")


def test_sync_entry_points_are_declared_and_exported():
    from ssds import _native as N

    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ssdk.h")).read()
    for name in ("ssdk_bn_sync_local_stats", "ssdk_bn_sync_fwd_finalize", "ssdk_bn_act_apply", "ssdk_bn_sync_bwd_local",
                 "ssdk_bn_sync_bwd_apply"):
        assert name in N.EXPORTS and name + "(" in hdr and hasattr(N.lib, name)
    assert N.lib.ssdk_version() == 245
