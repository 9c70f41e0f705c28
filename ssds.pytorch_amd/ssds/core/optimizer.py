"""Optimizer plumbing of the training entry points (reference ``ssds/core/optimizer.py``):
``trainable_param`` (:28-70) turns cfg.TRAIN.TRAINABLE_SCOPE ("a,b;c.d": ',' joins modules of one
parameter group, ';' separates groups with differential learning rates) into parameter lists and sets
``requires_grad``; ``configure_optimizer`` (:73-134) and ``configure_lr_scheduler`` (:137-166) map the cfg
names to torch.optim objects -- on a HIP device to SsdkSGD / SsdkAdam / SsdkRMSprop, the same optimizers on the kernels of
csrc/ssdk_sgd.hip."""
import ctypes
import os

import torch
import torch.optim as optim
from torch.optim import lr_scheduler


def _native_ok(p):
    return (p.is_cuda and p.dtype == torch.float32 and p.grad.dtype == torch.float32 and p.is_contiguous()
            and p.grad.is_contiguous() and not p.grad.is_sparse)


class SsdkOptimizer(optim.Optimizer):
    """What SsdkSGD, SsdkAdam and SsdkRMSprop share: their ``step()`` hands every fp32 parameter tensor of a group to one C entry
    point of csrc/ssdk_sgd.hip (a handful of multi-tensor launches, no host synchronisation), with the same ``param_groups``
    keys and ``state`` entries as the torch class plus ``fused=True`` (pipeline_anchor_ddp._device_skip), so ``state_dict()``
    / ``load_state_dict()`` and the lr schedulers are interchangeable with it (reference: core/optimizer.py:73-134 builds the
    torch classes).

    The NaN/Inf skip of the reference's loop (pipeline_anchor_apex.py:110-111, 126-127) is taken on the device: when the
    attribute ``found_inf`` (a 1-element float tensor, non-zero = skip -- the hook torch's GradScaler uses on fused optimizers)
    is set, the kernels read it and leave every tensor untouched.  A learning rate that is a device TENSOR is read by the kernel
    (``lr_dev``): a captured hipGraph keeps a live learning rate (pipeline_anchor_ddp.GraphedTrainStep).  Missing state is
    created as zeros here, before the launch, whether the step is then skipped or not.

    Parameters that are not contiguous fp32 HIP tensors take torch's own single-tensor update rule in Python (tests on the CPU).

    A subclass names its C entry point and the state it passes (``_native_args``), creates the state of one parameter
    (``_init_param_state``), writes the Python update (``_python_step``) and lists the group options the kernels do not
    implement (``_refused``: a loaded state dict that sets one is refused)."""

    _refused = ()

    def _init_param_state(self, group, p):
        raise NotImplementedError

    def _native_args(self, group):
        """(entry point, state keys in the order of its pointer arrays -- None for an array passed as NULL, "step" for the
        step counters -- hyperparameters between ``lr`` and ``found_inf``)"""
        raise NotImplementedError

    def _python_step(self, group, params):
        raise NotImplementedError

    def init_state(self, every=True):
        """Create the missing state of every trainable parameter (``every``) or of every parameter that has a gradient.
        GraphedTrainStep calls it before it snapshots the optimizer: state that first appeared during its warm-up would not be
        restored."""
        for group in self.param_groups:
            for p in group["params"]:
                if p.requires_grad if every else p.grad is not None:
                    self._init_param_state(group, p)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        found_inf = getattr(self, "found_inf", None)
        for group in self.param_groups:
            native, other = [], []
            for p in group["params"]:
                if p.grad is None:
                    continue
                self._init_param_state(group, p)
                (native if _native_ok(p) else other).append(p)
            if native:
                self._launch(group, native, found_inf)
            if other:
                if found_inf is not None and bool(found_inf.item() > 0):
                    continue
                self._python_step(group, other)
        return loss

    def _launch(self, group, params, found_inf):
        from ssds import _native as N

        name, keys, hyper = self._native_args(group)
        dev = params[0].device
        n = len(params)
        arr = ctypes.c_void_p * n
        arrays = [arr(*[p.data_ptr() for p in params]), arr(*[p.grad.data_ptr() for p in params])]
        for key in keys:
            if key is None:
                arrays.append(None)
                continue
            ts = [self.state[p][key] for p in params]
            for p, t in zip(params, ts):  # never a host pointer (a loaded CPU step), a wrong dtype or size for the kernel
                if not (isinstance(t, torch.Tensor) and t.device == p.device and t.dtype == torch.float32 and t.is_contiguous()
                        and t.numel() == (1 if key == "step" else p.numel())):
                    raise RuntimeError("{}: state[{!r}] of a parameter {} on {} is not a contiguous fp32 tensor of {} elements on "
                                       "that device".format(type(self).__name__, key, tuple(p.shape), p.device,
                                                            1 if key == "step" else p.numel()))
            arrays.append(arr(*[t.data_ptr() for t in ts]))
        ne = (ctypes.c_int64 * n)(*[p.numel() for p in params])
        lr = group["lr"]
        lr_dev = None
        if isinstance(lr, torch.Tensor) and lr.is_cuda:
            if lr.dtype != torch.float32 or lr.numel() != 1:
                raise ValueError("{}: a device learning rate is one fp32 element, got {} {}".format(
                    type(self).__name__, lr.dtype, tuple(lr.shape)))
            lr_dev = lr.data_ptr()
        fi = None
        if found_inf is not None:
            fi = found_inf if (found_inf.is_cuda and found_inf.dtype == torch.float32) else found_inf.to(dev, torch.float32)
            self._found_inf_keepalive = fi
        with torch.cuda.device(dev):
            N.check(getattr(N.lib, name)(n, *arrays, ne, lr_dev, 0.0 if lr_dev is not None else float(lr), *hyper,
                                         None if fi is None else fi.data_ptr(), N.stream_ptr(dev)), name)

    def load_state_dict(self, state_dict):
        """torch's loader copies the SAVED group keys over ours and keeps ``step`` where the saved groups say: a state dict of
        the torch class brings ``fused=None`` (which would turn the device-side skip off) and CPU ``step`` tensors.  Here every
        group is fused again, every ``step`` an fp32 scalar on its parameter's device, and a group with an option the kernels
        do not implement is refused before anything is loaded."""
        for g in state_dict["param_groups"]:
            for key in self._refused:
                if g.get(key):
                    raise ValueError("{} does not implement {}={!r}".format(type(self).__name__, key, g[key]))
        super(SsdkOptimizer, self).load_state_dict(state_dict)
        for group in self.param_groups:
            for k, v in self.defaults.items():
                group.setdefault(k, v)
            group["fused"] = True
            for p in group["params"]:
                st = self.state.get(p)
                if st and "step" in st:
                    s = st["step"]
                    s = s if isinstance(s, torch.Tensor) else torch.tensor(float(s))
                    st["step"] = s.to(device=p.device, dtype=torch.float32).reshape(())


class SsdkSGD(SsdkOptimizer):
    """``torch.optim.SGD`` (momentum, weight decay, Nesterov; dampening 0) on csrc/ssdk_sgd.hip (``ssdk_sgd_step``); state:
    ``momentum_buffer``.  See SsdkOptimizer."""

    _refused = ("dampening", "maximize")

    def __init__(self, params, lr=1e-3, momentum=0.0, weight_decay=0.0, nesterov=False):
        if nesterov and momentum <= 0:
            raise ValueError("Nesterov momentum requires a momentum")
        defaults = dict(lr=lr, momentum=momentum, dampening=0, weight_decay=weight_decay, nesterov=nesterov,
                        maximize=False, foreach=None, differentiable=False, fused=True)
        super(SsdkSGD, self).__init__(params, defaults)

    def _init_param_state(self, group, p):
        st = self.state[p]
        if group["momentum"] != 0 and "momentum_buffer" not in st:
            st["momentum_buffer"] = torch.zeros_like(p, memory_format=torch.preserve_format)

    def _native_args(self, group):
        mom = float(group["momentum"])
        return ("ssdk_sgd_step", ["momentum_buffer" if mom != 0 else None],
                [mom, float(group["weight_decay"]), 1 if group["nesterov"] else 0])

    def _python_step(self, group, params):
        lr, mom, wd, nest = group["lr"], float(group["momentum"]), float(group["weight_decay"]), bool(group["nesterov"])
        for p in params:
            g = p.grad if wd == 0 else p.grad.add(p, alpha=wd)
            if mom != 0:
                buf = self.state[p]["momentum_buffer"]
                buf.mul_(mom).add_(g)
                g = g.add(buf, alpha=mom) if nest else buf
            p.add_(g.to(p.dtype), alpha=-float(lr))


def _step_counter(p):
    return torch.zeros((), dtype=torch.float32, device=p.device)


class SsdkAdam(SsdkOptimizer):
    """``torch.optim.Adam`` (L2 weight decay, AMSGrad; no decoupled weight decay, no maximize) on csrc/ssdk_sgd.hip
    (``ssdk_adam_step``: bias corrections in fp64 from each tensor's ``step`` on the device); state: ``step`` (fp32 scalar on
    the parameter's device), ``exp_avg``, ``exp_avg_sq``, ``max_exp_avg_sq`` (AMSGrad).  See SsdkOptimizer."""

    _refused = ("maximize", "decoupled_weight_decay")

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, amsgrad=False):
        if not (0.0 <= lr and 0.0 <= eps and 0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0 and 0.0 <= weight_decay):
            raise ValueError("invalid Adam hyperparameters: lr={} betas={} eps={} weight_decay={}".format(lr, betas, eps,
                                                                                                       weight_decay))
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=False,
                        foreach=None, capturable=False, differentiable=False, fused=True, decoupled_weight_decay=False)
        super(SsdkAdam, self).__init__(params, defaults)

    def _init_param_state(self, group, p):
        st = self.state[p]
        if "step" not in st:
            st["step"] = _step_counter(p)
        for key in ("exp_avg", "exp_avg_sq") + (("max_exp_avg_sq",) if group["amsgrad"] else ()):
            if key not in st:
                st[key] = torch.zeros_like(p, memory_format=torch.preserve_format)

    def _native_args(self, group):
        ams = bool(group["amsgrad"])
        beta1, beta2 = group["betas"]
        return ("ssdk_adam_step", ["exp_avg", "exp_avg_sq", "max_exp_avg_sq" if ams else None, "step"],
                [float(beta1), float(beta2), float(group["eps"]), float(group["weight_decay"]), 1 if ams else 0])

    def _python_step(self, group, params):  # torch.optim.adam._single_tensor_adam
        lr, (beta1, beta2), eps, wd = float(group["lr"]), group["betas"], group["eps"], group["weight_decay"]
        for p in params:
            st = self.state[p]
            st["step"] += 1
            g = p.grad if wd == 0 else p.grad.add(p, alpha=wd)
            st["exp_avg"].lerp_(g, 1 - beta1)
            st["exp_avg_sq"].mul_(beta2).addcmul_(g, g, value=1 - beta2)
            step = st["step"].item()
            step_size = lr / (1 - beta1 ** step)
            bc2_sqrt = (1 - beta2 ** step) ** 0.5
            v = st["exp_avg_sq"]
            if group["amsgrad"]:
                v = torch.maximum(st["max_exp_avg_sq"], v, out=st["max_exp_avg_sq"])
            p.addcdiv_(st["exp_avg"], (v.sqrt() / bc2_sqrt).add_(eps), value=-step_size)


class SsdkRMSprop(SsdkOptimizer):
    """``torch.optim.RMSprop`` (non-centered; momentum, weight decay; no maximize) on csrc/ssdk_sgd.hip
    (``ssdk_rmsprop_step``); state: ``step`` (fp32 scalar on the parameter's device), ``square_avg``, ``momentum_buffer``
    (momentum > 0).  See SsdkOptimizer."""

    _refused = ("centered", "maximize")

    def __init__(self, params, lr=1e-2, alpha=0.99, eps=1e-8, weight_decay=0.0, momentum=0.0):
        if not (0.0 <= lr and 0.0 <= eps and 0.0 <= alpha and 0.0 <= weight_decay and 0.0 <= momentum):
            raise ValueError("invalid RMSprop hyperparameters: lr={} alpha={} eps={} weight_decay={} momentum={}".format(
                lr, alpha, eps, weight_decay, momentum))
        defaults = dict(lr=lr, momentum=momentum, alpha=alpha, eps=eps, centered=False, weight_decay=weight_decay,
                        capturable=False, foreach=None, maximize=False, differentiable=False, fused=True)
        super(SsdkRMSprop, self).__init__(params, defaults)

    def _init_param_state(self, group, p):
        st = self.state[p]
        if "step" not in st:
            st["step"] = _step_counter(p)
        for key in ("square_avg",) + (("momentum_buffer",) if group["momentum"] > 0 else ()):
            if key not in st:
                st[key] = torch.zeros_like(p, memory_format=torch.preserve_format)

    def _native_args(self, group):
        mom = float(group["momentum"])
        return ("ssdk_rmsprop_step", ["square_avg", "momentum_buffer" if mom > 0 else None, "step"],
                [float(group["alpha"]), float(group["eps"]), float(group["weight_decay"]), mom])

    def _python_step(self, group, params):  # torch.optim.rmsprop._single_tensor_rmsprop (centered=False)
        lr, alpha, eps, wd, mom = float(group["lr"]), group["alpha"], group["eps"], group["weight_decay"], group["momentum"]
        for p in params:
            st = self.state[p]
            st["step"] += 1
            g = p.grad if wd == 0 else p.grad.add(p, alpha=wd)
            st["square_avg"].mul_(alpha).addcmul_(g, g, value=1 - alpha)
            avg = st["square_avg"].sqrt().add_(eps)
            if mom > 0:
                buf = st["momentum_buffer"]
                buf.mul_(mom).addcdiv_(g, avg)
                p.add_(buf, alpha=-lr)
            else:
                p.addcdiv_(g, avg, value=-lr)


def _resolve(model, dotted):
    m = model
    for part in dotted.split("."):
        if not hasattr(m, part):
            raise ValueError(dotted + " is not in the model")
        m = getattr(m, part)
    return m


def trainable_param(model, trainable_scope):
    if trainable_scope == "":
        for p in model.parameters():
            p.requires_grad = True
        return [list(model.parameters())]
    for p in model.parameters():
        p.requires_grad = False
    groups = []
    for scope in trainable_scope.split(";"):
        params = []
        for name in scope.split(","):
            sub = _resolve(model, name)
            for p in sub.parameters():
                p.requires_grad = True
            params.extend(sub.parameters())
        groups.append(params)
    return groups


def configure_optimizer(trainable_param, cfg):
    if len(cfg.DIFFERENTIAL_LEARNING_RATE) == 0 or len(trainable_param) == 1:
        params = trainable_param[0]
    else:
        assert len(cfg.DIFFERENTIAL_LEARNING_RATE) == len(trainable_param)
        params = [{"params": p, "lr": lr} for p, lr in zip(trainable_param, cfg.DIFFERENTIAL_LEARNING_RATE)]
    name = cfg.OPTIMIZER
    # On a HIP device the update runs as a few multi-tensor launches (csrc/ssdk_sgd.hip: SsdkSGD, SsdkAdam, SsdkRMSprop), and
    # the kernels take a device-side ``found_inf`` flag: pipeline_anchor_ddp.train_step skips a step on NaN/Inf without reading
    # the flag back (the reference syncs 4-6 times per step, pipeline_anchor_apex.py:114-126).
    flat = [q for g in params for q in g["params"]] if params and isinstance(params[0], dict) else params
    fused = len(flat) > 0 and all(q.is_cuda and q.is_floating_point() for q in flat)
    if name == "sgd":
        if fused and os.environ.get("SSDK_SGD_NATIVE", "1") != "0":  # round 6: the update on csrc/ssdk_sgd.hip
            return SsdkSGD(params, lr=cfg.LEARNING_RATE, momentum=cfg.MOMENTUM, weight_decay=cfg.WEIGHT_DECAY)
        return optim.SGD(params, lr=cfg.LEARNING_RATE, momentum=cfg.MOMENTUM, weight_decay=cfg.WEIGHT_DECAY,
                         **({"fused": True} if fused else {}))
    if name == "rmsprop":
        return (SsdkRMSprop if fused else optim.RMSprop)(params, lr=cfg.LEARNING_RATE, momentum=cfg.MOMENTUM,
                                                         alpha=cfg.MOMENTUM_2, eps=cfg.EPS, weight_decay=cfg.WEIGHT_DECAY)
    if name in ("adam", "amsgrad"):
        return (SsdkAdam if fused else optim.Adam)(params, lr=cfg.LEARNING_RATE, betas=(cfg.MOMENTUM, cfg.MOMENTUM_2),
                                                   weight_decay=cfg.WEIGHT_DECAY, amsgrad=(name == "amsgrad"))
    raise AssertionError("optimizer can not be recognized")


def configure_lr_scheduler(optimizer, cfg):
    name = cfg.SCHEDULER
    if name == "step":
        return lr_scheduler.StepLR(optimizer, step_size=cfg.STEPS[0], gamma=cfg.GAMMA)
    if name == "multi_step":
        return lr_scheduler.MultiStepLR(optimizer, milestones=cfg.STEPS, gamma=cfg.GAMMA)
    if name == "exponential":
        return lr_scheduler.ExponentialLR(optimizer, gamma=cfg.GAMMA)
    if name == "sgdr":
        return lr_scheduler.CosineAnnealingWarmRestarts(optimizer, T_0=2, T_mult=2, eta_min=cfg.LR_MIN)
    raise AssertionError("scheduler can not be recognized.")
