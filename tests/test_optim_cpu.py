"""core/optimizer.SsdkAdam / SsdkRMSprop without a GPU: the Python update their parameters take off the HIP device is torch's
single-tensor rule bit for bit, their state dicts are interchangeable with the torch classes in both directions, the C-ABI
entry points of csrc/ssdk_sgd.hip refuse bad arguments before they launch anything, and configure_optimizer keeps the torch
classes for CPU parameters (reference: core/optimizer.py:73-134)."""
import copy
import ctypes

import pytest
import torch

ADAM_CASES = [dict(amsgrad=False, weight_decay=0.0), dict(amsgrad=True, weight_decay=1e-4),
              dict(amsgrad=False, weight_decay=1e-4), dict(amsgrad=True, weight_decay=0.0)]
RMSPROP_CASES = [dict(momentum=m, weight_decay=wd) for m in (0.0, 0.9) for wd in (0.0, 1e-4)]


def _pair(kind, kw, seed=0):
    """(ours, torch's) on two identical copies of four CPU tensors in two parameter groups with different learning rates."""
    from ssds.core.optimizer import SsdkAdam, SsdkRMSprop

    g = torch.Generator().manual_seed(seed)
    shapes = [(5, 3), (7,), (2, 3, 3, 3), (1,)]
    mine = [torch.randn(s, generator=g).requires_grad_(True) for s in shapes]
    ref = [t.detach().clone().requires_grad_(True) for t in mine]
    groups = lambda ps: [{"params": ps[:2], "lr": 1e-2}, {"params": ps[2:], "lr": 3e-3}]  # noqa: E731
    if kind == "adam":
        return (SsdkAdam(groups(mine), betas=(0.9, 0.99), **kw), torch.optim.Adam(groups(ref), betas=(0.9, 0.99), foreach=False, **kw),
                mine, ref)
    return (SsdkRMSprop(groups(mine), alpha=0.99, eps=1e-8, **kw),
            torch.optim.RMSprop(groups(ref), alpha=0.99, eps=1e-8, foreach=False, **kw), mine, ref)


def _steps(opt_pairs, gen, steps, zero_at=-1):
    for s in range(steps):
        grads = None
        for opt, params in opt_pairs:
            if grads is None:
                grads = [torch.zeros_like(p) if s == zero_at else torch.randn(p.shape, generator=gen) for p in params]
            for p, gr in zip(params, grads):
                p.grad = gr.clone()
            opt.step()


def _assert_identical(o1, p1, o2, p2):
    for a, b in zip(p1, p2):
        assert torch.equal(a, b), float((a - b).abs().max())
        s1, s2 = o1.state[a], o2.state[b]
        assert set(s1) == set(s2), (set(s1), set(s2))
        for k in s1:
            assert s1[k].dtype == s2[k].dtype and torch.equal(s1[k], s2[k]), k


@pytest.mark.parametrize("kind,kw", [("adam", kw) for kw in ADAM_CASES] + [("rmsprop", kw) for kw in RMSPROP_CASES])
def test_python_update_is_torchs_single_tensor_rule_bit_for_bit(kind, kw):
    mine_opt, ref_opt, mine, ref = _pair(kind, kw)
    _steps([(mine_opt, mine), (ref_opt, ref)], torch.Generator().manual_seed(1), 10, zero_at=4)
    _assert_identical(mine_opt, mine, ref_opt, ref)
    assert all(g["fused"] is True for g in mine_opt.param_groups)
    assert all(float(mine_opt.state[p]["step"]) == 10.0 for p in mine)


@pytest.mark.parametrize("kind,kw", [("adam", ADAM_CASES[1]), ("rmsprop", RMSPROP_CASES[3])])
def test_state_dicts_interchange_with_torch_both_ways(kind, kw):
    gen = torch.Generator().manual_seed(2)
    mine_opt, ref_opt, mine, ref = _pair(kind, kw)
    _steps([(mine_opt, mine), (ref_opt, ref)], gen, 3)
    # torch -> ours -> continue == torch continuing
    mine_opt2, _, mine2, _ = _pair(kind, kw)
    with torch.no_grad():
        for a, b in zip(mine2, ref):
            a.copy_(b)
    mine_opt2.load_state_dict(copy.deepcopy(ref_opt.state_dict()))
    assert all(g["fused"] is True for g in mine_opt2.param_groups), "a torch state dict turned the device-side skip off"
    assert all(mine_opt2.state[p]["step"].dtype == torch.float32 and mine_opt2.state[p]["step"].dim() == 0 for p in mine2)
    # ours -> torch -> continue == ours continuing
    _, ref_opt3, _, ref3 = _pair(kind, kw)
    with torch.no_grad():
        for a, b in zip(ref3, mine):
            a.copy_(b)
    ref_opt3.load_state_dict(copy.deepcopy(mine_opt.state_dict()))
    for g in ref_opt3.param_groups:  # ``fused`` is the marker of ours; torch's Adam would take its fused CPU kernel with it
        g["fused"] = None
    gen_state = gen.get_state()
    _steps([(mine_opt2, mine2), (ref_opt, ref)], gen, 4)
    _assert_identical(mine_opt2, mine2, ref_opt, ref)
    gen.set_state(gen_state)
    _steps([(ref_opt3, ref3), (mine_opt, mine)], gen, 4)
    _assert_identical(mine_opt, mine, ref_opt3, ref3)


@pytest.mark.parametrize("kind,key", [("rmsprop", "centered"), ("rmsprop", "maximize"), ("adam", "maximize"),
                                      ("adam", "decoupled_weight_decay")])
def test_options_the_kernels_do_not_implement_are_refused(kind, key):
    mine_opt, ref_opt, mine, ref = _pair(kind, {})
    ref_opt.param_groups[1][key] = True
    _steps([(ref_opt, ref)], torch.Generator().manual_seed(3), 1)
    before = copy.deepcopy(mine_opt.state_dict())
    with pytest.raises(ValueError, match=key):
        mine_opt.load_state_dict(ref_opt.state_dict())
    assert mine_opt.state_dict() == before, "a refused state dict was loaded in part"


def test_a_skipped_step_creates_zero_state_and_changes_nothing():
    """found_inf on the Python path: state is created as zeros before the step is skipped, parameters and counters stay."""
    mine_opt, _, mine, _ = _pair("adam", dict(amsgrad=True))
    before = [p.detach().clone() for p in mine]
    for p in mine:
        p.grad = torch.ones_like(p)
    mine_opt.found_inf = torch.ones(1)
    mine_opt.step()
    for p, b in zip(mine, before):
        st = mine_opt.state[p]
        assert torch.equal(p, b) and float(st["step"]) == 0.0
        assert all(float(st[k].abs().max()) == 0.0 for k in ("exp_avg", "exp_avg_sq", "max_exp_avg_sq"))


def _lib():
    from ssds import _native as N

    return N


def _err(N):
    return N.lib.ssdk_last_error().decode()


def test_c_entry_points_are_exported_and_refuse_bad_arguments():
    N = _lib()
    assert "ssdk_adam_step" in N.EXPORTS and "ssdk_rmsprop_step" in N.EXPORTS
    L = N.lib
    arr = ctypes.c_void_p * 1
    fake = lambda: arr(0x1000)  # noqa: E731 -- never dereferenced: every call below fails validation first
    ne = (ctypes.c_int64 * 1)(4)
    big = (ctypes.c_int64 * 1)(1 << 32)
    nul = arr(0)
    adam = lambda n, p, g, m, v, vmax, st, numel, ams: L.ssdk_adam_step(  # noqa: E731
        n, p, g, m, v, vmax, st, numel, None, 1e-3, 0.9, 0.999, 1e-8, 0.0, ams, None, None)
    rms = lambda n, p, g, sq, buf, st, numel, mom: L.ssdk_rmsprop_step(  # noqa: E731
        n, p, g, sq, buf, st, numel, None, 1e-2, 0.99, 1e-8, 0.0, mom, None, None)
    assert adam(0, None, None, None, None, None, None, None, 1) == 0
    assert rms(0, None, None, None, None, None, None, 0.9) == 0
    bad_adam = [
        (-1, fake(), fake(), fake(), fake(), None, fake(), ne, 0),      # n < 0
        (1, None, fake(), fake(), fake(), None, fake(), ne, 0),         # NULL params
        (1, fake(), None, fake(), fake(), None, fake(), ne, 0),         # NULL grads
        (1, fake(), fake(), None, fake(), None, fake(), ne, 0),         # NULL exp_avg
        (1, fake(), fake(), fake(), None, None, fake(), ne, 0),         # NULL exp_avg_sq
        (1, fake(), fake(), fake(), fake(), None, fake(), ne, 1),       # AMSGrad without max_exp_avg_sq
        (1, fake(), fake(), fake(), fake(), None, None, ne, 0),         # NULL steps
        (1, fake(), fake(), fake(), fake(), None, fake(), None, 0),     # NULL numel
        (1, fake(), fake(), nul, fake(), None, fake(), ne, 0),          # a NULL tensor pointer
        (1, fake(), fake(), fake(), fake(), None, nul, ne, 0),          # a NULL step counter
        (1, fake(), fake(), fake(), fake(), None, fake(), big, 0),      # >= 2^32 elements
    ]
    for args in bad_adam:
        assert adam(*args) == -1, args  # SSDK_E_BADARG
        assert "ssdk_adam_step" in _err(N), args
    bad_rms = [
        (-1, fake(), fake(), fake(), None, fake(), ne, 0.0),
        (1, None, fake(), fake(), None, fake(), ne, 0.0),
        (1, fake(), fake(), None, None, fake(), ne, 0.0),
        (1, fake(), fake(), fake(), None, fake(), ne, 0.9),             # momentum without momentum buffers
        (1, fake(), fake(), fake(), None, None, ne, 0.0),
        (1, fake(), fake(), fake(), None, fake(), big, 0.0),
    ]
    for args in bad_rms:
        assert rms(*args) == -1, args
        assert "ssdk_rmsprop_step" in _err(N), args


def _cfg(name, **kw):
    from ssds.core.config import cfg

    c = copy.deepcopy(cfg.TRAIN.OPTIMIZER)
    c.OPTIMIZER = name
    for k, v in kw.items():
        setattr(c, k, v)
    return c


@pytest.mark.parametrize("name", ["adam", "amsgrad", "rmsprop", "sgd"])
def test_configure_optimizer_keeps_the_torch_classes_on_cpu(name):
    from ssds.core import optimizer as O

    params = [[torch.nn.Parameter(torch.randn(3)), torch.nn.Parameter(torch.randn(2, 2))]]
    c = _cfg(name, LEARNING_RATE=0.005, MOMENTUM=0.8, MOMENTUM_2=0.95, EPS=1e-6, WEIGHT_DECAY=2e-4)
    opt = O.configure_optimizer(params, c)
    assert not isinstance(opt, O.SsdkOptimizer)
    g = opt.param_groups[0]
    if name in ("adam", "amsgrad"):
        assert type(opt) is torch.optim.Adam
        assert g["betas"] == (0.8, 0.95) and g["eps"] == 1e-8 and g["amsgrad"] == (name == "amsgrad")
    elif name == "rmsprop":
        assert type(opt) is torch.optim.RMSprop
        assert g["alpha"] == 0.95 and g["eps"] == 1e-6 and g["momentum"] == 0.8
    else:
        assert type(opt) is torch.optim.SGD and g["momentum"] == 0.8
    assert g["lr"] == 0.005 and g["weight_decay"] == 2e-4
