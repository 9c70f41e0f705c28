"""core/optimizer.SsdkAdam / SsdkRMSprop on the HIP device (csrc/ssdk_sgd.hip: ssdk_adam_step, ssdk_rmsprop_step): the
kernels against torch's Adam / RMSprop, the device-side NaN/Inf skip, a live learning rate inside a captured graph, the
training step and GraphedTrainStep on them, and a torch state dict loaded onto the device (reference: core/optimizer.py:73-134
builds torch.optim.Adam / RMSprop; experiments/cfgs/tests/test.yml trains with `adam`)."""
from collections import OrderedDict
import copy

import pytest

pytestmark = pytest.mark.gpu

# ~45 tensors (two launches per call): tails around the 4096-element block, one- to four-element tensors, a >= 1M tensor
SIZES = [1, 3, 4, 4095, 4096, 4097, 65537, 1 << 20, 5, 12289] + [37 * (i + 1) + 3 * i * i for i in range(34)]


def _tensors(seed):
    """The parameters: SIZES, plus a view at element offset 1 (the scalar path: not 16-byte aligned)."""
    import torch

    g = torch.Generator(device="cuda").manual_seed(seed)
    base = torch.randn(1001, device="cuda", generator=g)
    mine = [torch.randn(n, device="cuda", generator=g).requires_grad_(True) for n in SIZES] + [base[1:1000].detach().requires_grad_(True)]
    return mine, g


def _clone(ts):
    return [t.detach().clone().requires_grad_(True) for t in ts]


def _grads(params_lists, g, zero=False):
    import torch

    for i, p in enumerate(params_lists[0]):
        gr = torch.zeros_like(p) if zero else torch.randn(p.shape, device="cuda", generator=g)
        for ps in params_lists:
            ps[i].grad = gr.clone()


def _compare(o1, p1, o2, p2, rtol=1e-5, atol=1e-7):
    """Parameters and every state tensor to rtol, and to atol in units of the tensor's largest magnitude (at least 1): an
    element that is the difference of two large terms -- RMSprop's momentum buffer, up to ~100, where it crosses zero -- keeps
    the rounding of those terms; step counters exactly.  Returns the largest |x - y| / (rtol |y| + atol scale) seen (<= 1) and
    the largest |x - y|."""
    import torch

    worst = diff = 0.0
    for a, b in zip(p1, p2):
        pairs = [(a.detach(), b.detach())] + [(o1.state[a][k], o2.state[b][k]) for k in o1.state[a] if k != "step"]
        assert float(o1.state[a]["step"]) == float(o2.state[b]["step"])
        for x, y in pairs:
            scale = max(1.0, float(y.abs().max()))
            torch.testing.assert_close(x, y, rtol=rtol, atol=atol * scale)
            worst = max(worst, float(((x - y).abs() / (rtol * y.abs() + atol * scale)).max()))
            diff = max(diff, float((x - y).abs().max()))
    return worst, diff


def _ours(kind, kw, params):
    from ssds.core.optimizer import SsdkAdam, SsdkRMSprop

    return (SsdkAdam if kind == "adam" else SsdkRMSprop)(params, **kw)


def _ours_and_torch(kind, kw, params, ref, **torch_kw):
    import torch

    return _ours(kind, kw, params), (torch.optim.Adam if kind == "adam" else torch.optim.RMSprop)(ref, **kw, **torch_kw)


CASES = [("adam", dict(lr=1e-3, betas=(0.9, 0.99), weight_decay=1e-4, amsgrad=False)),
         ("adam", dict(lr=1e-3, betas=(0.9, 0.99), weight_decay=0.0, amsgrad=True)),
         ("rmsprop", dict(lr=1e-3, alpha=0.99, eps=1e-8, weight_decay=1e-4, momentum=0.0)),
         ("rmsprop", dict(lr=1e-3, alpha=0.99, eps=1e-8, weight_decay=0.0, momentum=0.9))]


@pytest.mark.parametrize("kind,kw", CASES)
def test_kernels_match_torch(kind, kw):
    """20 steps against torch's foreach implementation (and, for Adam, its fused one where this build has it on the device),
    one of them with zero gradients: parameters and every state tensor to rtol 1e-5 / atol 1e-7, step counters exactly."""
    import torch

    mine, g = _tensors(11)
    ref = _clone(mine)
    o_mine, o_ref = _ours_and_torch(kind, kw, mine, ref, foreach=True)
    others = [(o_ref, ref)]
    if kind == "adam":
        fused = _clone(mine)
        try:
            others.append((torch.optim.Adam(fused, fused=True, **kw), fused))
        except (RuntimeError, ValueError):
            pass
    for s in range(20):
        _grads([mine] + [ps for _, ps in others], g, zero=(s == 7))
        o_mine.step()
        for o, _ in others:
            o.step()
    for o, ps in others:
        worst, diff = _compare(o_mine, mine, o, ps)
        print("{} {} vs {}{}: largest deviation {:.3g} of the tolerance, largest |difference| {:.3g}".format(
            kind, kw, type(o).__name__, " (fused)" if o.param_groups[0].get("fused") else "", worst, diff))
        assert all(float(o_mine.state[p]["step"]) == 20.0 and o_mine.state[p]["step"].is_cuda for p in mine)


@pytest.mark.parametrize("kind,kw", CASES)
def test_the_device_skip_touches_nothing(kind, kw):
    """found_inf = 1: parameters, every state tensor and every step counter keep their bits; a skipped FIRST step followed by
    a real one equals torch's first step."""
    import torch

    mine, g = _tensors(12)
    ref = _clone(mine)
    o_mine, o_ref = _ours_and_torch(kind, kw, mine, ref, foreach=True)
    _grads([mine, ref], g)
    o_mine.found_inf = torch.ones(1, device="cuda")
    o_mine.step()  # the first step, skipped: state is created as zeros, nothing else happens
    for p in mine:
        st = o_mine.state[p]
        assert float(st["step"]) == 0.0 and all(float(v.abs().max()) == 0.0 for v in st.values())
    del o_mine.found_inf
    o_mine.step()
    o_ref.step()
    _compare(o_mine, mine, o_ref, ref)
    for _ in range(2):
        _grads([mine, ref], g)
        o_mine.step()
    before = [(p.detach().clone(), {k: v.clone() for k, v in o_mine.state[p].items()}) for p in mine]
    _grads([mine], g)
    o_mine.found_inf = torch.ones(1, device="cuda")
    o_mine.step()
    del o_mine.found_inf
    for p, (pb, sb) in zip(mine, before):
        assert torch.equal(p, pb)
        assert all(torch.equal(o_mine.state[p][k], v) for k, v in sb.items())


@pytest.mark.parametrize("kind,kw", [CASES[1], CASES[3]])
def test_a_captured_step_reads_the_learning_rate_live(kind, kw):
    """opt.step() alone captured in a graph: three replays with the lr tensor changed in place in between equal three eager
    steps with the same rates (the counters advance inside the graph too)."""
    import torch

    mine, g = _tensors(13)
    twin = _clone(mine)
    lr, lr_twin = torch.full((), 1e-3, device="cuda"), torch.full((), 1e-3, device="cuda")
    o_mine, o_twin = _ours(kind, dict(kw, lr=lr), mine), _ours(kind, dict(kw, lr=lr_twin), twin)
    _grads([mine, twin], g)
    o_mine.init_state(every=True)  # no allocation inside the capture
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        o_mine.step()
    for rate in (1e-3, 5e-4, 3e-3):
        lr.fill_(rate)
        lr_twin.fill_(rate)
        graph.replay()
        o_twin.step()
    torch.cuda.synchronize()
    for a, b in zip(mine, twin):
        assert torch.equal(a, b)
        for k, v in o_twin.state[b].items():
            assert torch.equal(o_mine.state[a][k], v), k
    assert all(float(o_mine.state[p]["step"]) == 3.0 for p in mine)


def _tiny_step_setup(seed=0):
    """The tiny SSD-MobileNetV2 training step of tests/test_gpu_train.py."""
    import torch
    from ssds.core import criterion
    from ssds.dataset.synthetic import SyntheticDetectionLoader
    from ssds.modeling import nets, ssds
    from ssds.modeling.layers import box
    from ssds.pipeline.pipeline_anchor_ddp import ModelWithLossBasic

    torch.manual_seed(seed)
    o, e, h = ssds.SSD.add_extras([[5, 7, "Conv:S"], [96, 320, 64]], [2, 2, 2], 5)
    model = ssds.SSD(nets.MobileNetV2(outputs=o), e, h, 5)
    mwl = ModelWithLossBasic(model, criterion.FocalLoss(), criterion.SmoothL1Loss(), 5, [0.5, 0.4], 0).cuda()
    anchors = OrderedDict((s, box.generate_anchors(s, [1], [2.0, 2.828])) for s in (16, 32, 64))
    loader = SyntheticDetectionLoader(4, (128, 128), 5, steps=1, device=torch.device("cuda"), max_gt=6)
    images, targets = loader.batch()
    targets[..., 2:4] = targets[..., 2:4].clamp(min=24)
    targets[targets[..., 4] < 0] = -1
    return mwl.train(), images, targets, anchors


def _configured(name, params, lr=1e-3):
    from ssds.core import optimizer
    from ssds.core.config import cfg

    c = copy.deepcopy(cfg.TRAIN.OPTIMIZER)
    c.OPTIMIZER, c.LEARNING_RATE = name, lr
    return optimizer.configure_optimizer([list(params)], c)


def _state_snapshot(opt, params):
    return [{k: v.clone() for k, v in opt.state[p].items()} for p in params if p in opt.state]


@pytest.mark.parametrize("name", ["adam", "rmsprop"])
def test_train_step_runs_the_native_optimizer_with_the_device_skip(name):
    import torch
    from ssds.core.optimizer import SsdkAdam, SsdkRMSprop
    from ssds.pipeline.pipeline_anchor_ddp import _device_skip, train_step

    mwl, images, targets, anchors = _tiny_step_setup(1)
    opt = _configured(name, mwl.parameters())
    assert type(opt) is (SsdkAdam if name == "adam" else SsdkRMSprop) and _device_skip(opt)
    flat = lambda m: torch.cat([p.detach().flatten() for p in m.parameters()])  # noqa: E731
    p0 = flat(mwl).clone()
    for _ in range(2):
        c, l, skipped = train_step(mwl, images, targets, anchors, opt)
        assert isinstance(skipped, torch.Tensor) and float(skipped) == 0.0
    assert torch.isfinite(flat(mwl)).all() and not torch.equal(p0, flat(mwl))
    params = list(mwl.parameters())
    assert all(float(opt.state[p]["step"]) == 2.0 for p in params if p.grad is not None)
    before, st_before = flat(mwl).clone(), _state_snapshot(opt, params)
    bad_images = images.clone()
    bad_images[0, 0, 0, 0] = float("nan")
    c, l, skipped = train_step(mwl, bad_images, targets, anchors, opt)
    assert isinstance(skipped, torch.Tensor) and float(skipped) == 1.0
    assert torch.equal(before, flat(mwl)), "a skipped step must not touch the parameters"
    for a, b in zip(st_before, _state_snapshot(opt, params)):
        assert all(torch.equal(a[k], b[k]) for k in a), "... nor the optimizer state"


def test_graphed_train_step_with_adam_equals_the_eager_step():
    """GraphedTrainStep on SsdkAdam: the warm-up leaves no trace (moments zero, steps 0), and each replay is checked against
    the eager step of a twin taken right before it, to the bar of the SGD test in tests/test_gpu_train.py.  fp32 (no autocast):
    Adam's first steps are about lr * sign(grad), so bf16 noise in tiny gradients would weigh more than it does for SGD."""
    import torch
    from ssds.core.optimizer import SsdkAdam
    from ssds.pipeline.pipeline_anchor_ddp import GraphedTrainStep, train_step

    mwl, images, targets, anchors = _tiny_step_setup(3)
    opt = SsdkAdam(mwl.parameters(), lr=1e-3, weight_decay=1e-4)
    graphed = GraphedTrainStep(mwl, images, targets, anchors, opt, autocast_dtype=None, warmup=2)
    params = list(mwl.parameters())
    assert all(p in opt.state for p in params if p.requires_grad)
    for p in params:
        st = opt.state[p]
        assert float(st["step"]) == 0.0 and st["step"].is_cuda
        assert float(st["exp_avg"].abs().max()) == 0.0 and float(st["exp_avg_sq"].abs().max()) == 0.0
    flat = lambda m: torch.cat([p.detach().flatten() for p in m.parameters()])  # noqa: E731
    for i in range(3):
        twin = copy.deepcopy(mwl)
        opt_twin = SsdkAdam(twin.parameters(), lr=1e-3, weight_decay=1e-4)
        opt_twin.load_state_dict(copy.deepcopy(opt.state_dict()))
        before = flat(mwl).clone()
        c, l, bad = graphed(images, targets)
        c2, l2, bad2 = train_step(twin, images, targets, anchors, opt_twin, autocast_dtype=None)
        assert float(bad) == 0 and float(bad2) == 0
        torch.testing.assert_close(c.float(), c2.float(), rtol=2e-2, atol=1e-5)
        step, step2 = flat(mwl) - before, flat(twin) - before
        assert float(step.abs().mean()) > 0
        assert float((step - step2).abs().mean()) <= 0.2 * float(step2.abs().mean()) + 1e-8
        assert all(float(opt.state[p]["step"]) == i + 1 for p in params if p.grad is not None)
    before = flat(mwl).clone()
    bad_images = images.clone()
    bad_images[0, 0, 0, 0] = float("nan")
    c, l, bad = graphed(bad_images, targets)
    assert float(bad) == 1.0 and torch.equal(before, flat(mwl))
    assert all(float(opt.state[p]["step"]) == 3.0 for p in params if p.grad is not None)


def test_a_loaded_torch_adam_state_runs_on_the_device():
    """torch.optim.Adam keeps `step` on the CPU; loaded into SsdkAdam the counters move to the device as fp32, the groups stay
    fused, and the next steps match torch continuing from the same state dict."""
    import torch
    from ssds.core.optimizer import SsdkAdam
    from ssds.pipeline.pipeline_anchor_ddp import _device_skip

    ref, g = _tensors(14)
    kw = dict(lr=2e-3, betas=(0.9, 0.99), weight_decay=1e-4)
    o_ref = torch.optim.Adam(ref, **kw)
    for _ in range(3):
        _grads([ref], g)
        o_ref.step()
    sd = copy.deepcopy(o_ref.state_dict())
    assert not sd["state"][0]["step"].is_cuda
    mine = _clone(ref)
    o_mine = SsdkAdam(mine, **kw)
    o_mine.load_state_dict(sd)
    assert _device_skip(o_mine)
    assert all(o_mine.state[p]["step"].is_cuda and o_mine.state[p]["step"].dtype == torch.float32 for p in mine)
    for _ in range(5):
        _grads([mine, ref], g)
        o_mine.step()
        o_ref.step()
    _compare(o_mine, mine, o_ref, ref)
