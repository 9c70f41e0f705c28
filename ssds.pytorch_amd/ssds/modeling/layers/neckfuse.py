"""The memory-bound neck operations of the FPN / BiFPN training step on the NCHW tensors themselves (csrc/ssdk_necktrain.hip),
forward and backward:

    neck_fuse            y = w0 a + w1 R_b(b) [+ w2 R_c(c)]     R = SAME | UP2 (nearest x2) | POOL2 (max_pool2d(kernel 2))
                         BiFPNModule's weighted fusions; without weights the FPN top-down step  lateral + upsample(x)
    TrainMaxPool3x3s2    nn.MaxPool2d(3, 2, 1), the ResNet stem's

PyTorch-ROCm runs a fusion as four to six ATen launches with a full-size temporary each, and its backward ends in whole-tensor
reductions for the scalar weight gradients; its max-pool keeps an int64 index per output element.  Here a fusion is one launch
forward and one (+ a one-workgroup launch for the weight gradient) backward, the fusion weights are read from device memory (a
column of the fast-normalised fp32 [K, L] tensor BiFPNModule.forward computes: no ``.item()``), and the pooling backward
recomputes the arg-max from the saved input (first maximum in row-major window order, torch's rule).

``use_native_neck(model)`` enables the path per model; a model it was never called on runs the earlier expressions."""
import torch
import torch.nn as nn

from ssds import _native as N

SAME, UP2, POOL2 = 0, 1, 2  # include/ssdk.h SSDK_FUSE_*
# The longest chain of dependent fp32 additions a term of a weight gradient passes through in csrc/ssdk_necktrain.hip, at the largest
# supported tensor (2^31 elements): 16 products of a work item + 64 items of a thread's inner accumulator + 33 flushes into its outer
# one + 6 (wave tree) + 4 (waves of the workgroup) + 16 partials per thread of the final launch + 6 + 4 (its trees).
WSUM_DEPTH = 16 + 64 + 33 + 6 + 4 + 16 + 6 + 4
STATS = {"bifpn_modules": 0, "fpn_models": 0, "maxpools": 0, "fuse_forward": 0, "fuse_backward": 0, "pool_forward": 0, "pool_backward": 0}
_HALF = (torch.bfloat16, torch.float16)


def _geometry(a, src, mode):
    """The source dims the kernels expect of ``src`` under ``mode`` for the output dims of ``a``, or None."""
    n, c, h, w = (int(v) for v in a.shape)
    sn, sc, sh, sw = (int(v) for v in src.shape)
    if (sn, sc) != (n, c):
        return None
    if mode == SAME:
        ok = (sh, sw) == (h, w)
    elif mode == UP2:
        ok = h % 2 == 0 and w % 2 == 0 and (sh, sw) == (h // 2, w // 2)
    elif mode == POOL2:
        ok = (sh // 2, sw // 2) == (h, w)
    else:
        ok = False
    return (sh, sw) if ok else None


def _check(a, b, c, weights, col, mode_b, mode_c):
    srcs = [a, b] + ([] if c is None else [c])
    for t in srcs:
        if not (torch.is_tensor(t) and t.is_cuda and t.dim() == 4 and t.dtype in _HALF and t.is_contiguous()):
            raise ValueError("neck_fuse: 16-bit contiguous NCHW tensors on a HIP device, got {} {} on {}".format(
                tuple(t.shape) if torch.is_tensor(t) else type(t), getattr(t, "dtype", None), getattr(t, "device", None)))
        if t.dtype != a.dtype or t.device != a.device:
            raise ValueError("neck_fuse: the sources differ in dtype or device")
    if _geometry(a, b, mode_b) is None or (c is not None and _geometry(a, c, mode_c) is None):
        raise ValueError("neck_fuse: source shapes {} do not fit the output {} under modes {} / {}".format(
            [tuple(t.shape) for t in srcs[1:]], tuple(a.shape), mode_b, mode_c))
    if weights is not None:
        if not (weights.is_cuda and weights.device == a.device and weights.dtype == torch.float32 and weights.dim() == 2
                and int(weights.shape[0]) == len(srcs) and 0 <= col < int(weights.shape[1])):
            raise ValueError("neck_fuse: weights must be an fp32 [{}, L] tensor on the sources' device with 0 <= col < L".format(len(srcs)))


class _NeckFuse(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b, c, weights, col, mode_b, mode_c):
        _check(a, b, c, weights, col, mode_b, mode_c)
        n, ch, h, w = (int(v) for v in a.shape)
        dev = a.device
        a, b = a.detach(), b.detach()
        c = None if c is None else c.detach()
        wt = None if weights is None else weights.detach().contiguous()
        cols = 0 if wt is None else int(wt.shape[1])
        hb, wb = int(b.shape[2]), int(b.shape[3])
        hc, wc = (0, 0) if c is None else (int(c.shape[2]), int(c.shape[3]))
        y = torch.empty_like(a)
        with torch.cuda.device(dev):
            N.check(N.lib.ssdk_neck_fuse_fwd(a.data_ptr(), b.data_ptr(), None if c is None else c.data_ptr(),
                                             None if wt is None else wt.data_ptr() + 4 * col, cols, y.data_ptr(), n, ch, h, w,
                                             mode_b, hb, wb, mode_c, hc, wc, N.dtype_code(a), N.stream_ptr(dev)), "neck_fuse_fwd")
        STATS["fuse_forward"] += 1
        need_w = wt is not None and ctx.needs_input_grad[3]
        # a source is read again for the weight gradient and for the arg-max of a pooled gradient
        ctx.save_for_backward(a if need_w else None,
                              b if need_w or (mode_b == POOL2 and ctx.needs_input_grad[1]) else None,
                              c if c is not None and (need_w or (mode_c == POOL2 and ctx.needs_input_grad[2])) else None, wt)
        ctx.meta = (tuple(a.shape), tuple(b.shape), None if c is None else tuple(c.shape), col, mode_b, mode_c, a.dtype, need_w)
        return y

    @staticmethod
    def backward(ctx, gy):
        a, b, c, wt = ctx.saved_tensors
        sa, sb, sc, col, mode_b, mode_c, dt, need_w = ctx.meta
        n, ch, h, w = sa
        dev = gy.device
        gy = gy.contiguous()
        if gy.dtype != dt:
            gy = gy.to(dt)
        need_a, need_b, need_c = ctx.needs_input_grad[0], ctx.needs_input_grad[1], sc is not None and ctx.needs_input_grad[2]
        ga = gb = gc = gw = ws = None
        if need_a:
            ga = gy if wt is None else torch.empty(sa, device=dev, dtype=dt)
        if need_b:
            gb = torch.empty(sb, device=dev, dtype=dt)
        if need_c:
            gc = torch.empty(sc, device=dev, dtype=dt)
        nbytes = 0
        if need_w:
            gw = torch.empty(tuple(wt.shape), device=dev, dtype=torch.float32)
            nbytes = int(N.lib.ssdk_neck_fuse_bwd_workspace_bytes(n, ch, h, w))
            ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        with torch.cuda.device(dev):
            N.check(N.lib.ssdk_neck_fuse_bwd(gy.data_ptr(), ptr(a), ptr(b), ptr(c), 2 if sc is None else 3,
                                             None if wt is None else wt.data_ptr() + 4 * col, 0 if wt is None else int(wt.shape[1]),
                                             None if wt is None else ptr(ga), ptr(gb), ptr(gc), ptr(gw), 0 if gw is None else int(gw.shape[1]),
                                             col, ptr(ws), nbytes, n, ch, h, w, mode_b, sb[2], sb[3], mode_c,
                                             0 if sc is None else sc[2], 0 if sc is None else sc[3], N.dtype_code(gy), N.stream_ptr(dev)),
                    "neck_fuse_bwd")
        STATS["fuse_backward"] += 1
        return ga, gb, gc, gw, None, None, None


def neck_fuse(a, b, c=None, weights=None, col=0, mode_b=SAME, mode_c=SAME):
    """y = w0 a + w1 R_b(b) [+ w2 R_c(c)] with (w0, w1[, w2]) = weights[:, col], or all 1 when ``weights`` is None, on
    csrc/ssdk_necktrain.hip; differentiable in a, b, c and weights (whose gradient is one [K, L] tensor).  Explicit: 16-bit contiguous
    NCHW tensors on a HIP device and an fp32 [K, L] weight tensor on the same device, anything else raises."""
    return _NeckFuse.apply(a, b, c, weights, int(col), int(mode_b), int(mode_c))


def _kernel_inputs(*tensors):
    """The tensors as the kernels take them -- under autocast cast to its dtype, the contract of DenseConv3x3.forward -- or None
    when one of them is not a 16-bit contiguous NCHW tensor on a HIP device."""
    autocast = torch.is_autocast_enabled()
    out = []
    for t in tensors:
        if not (torch.is_tensor(t) and t.is_cuda and t.dim() == 4):
            return None
        if autocast:
            t = t.to(torch.get_autocast_dtype("cuda"))
        if t.dtype not in _HALF or not t.is_contiguous() or t.dtype != (out[0].dtype if out else t.dtype):
            return None
        out.append(t)
    return out


def try_fuse(a, b, c=None, weights=None, col=0, mode_b=SAME, mode_c=SAME):
    """``neck_fuse`` when the operands meet its contract (16-bit, contiguous, HIP device; under autocast after the cast to its dtype;
    weights fp32 or in the tensors' dtype; shapes that fit the modes), else None: the caller runs its eager expression."""
    srcs = _kernel_inputs(*([a, b] if c is None else [a, b, c]))
    if srcs is None:
        return None
    a, b = srcs[0], srcs[1]
    c = srcs[2] if c is not None else None
    if _geometry(a, b, mode_b) is None or (c is not None and _geometry(a, c, mode_c) is None):
        return None
    if weights is not None:
        if not weights.is_cuda or weights.dim() != 2 or weights.dtype not in (torch.float32, a.dtype):
            return None
        with torch.autocast("cuda", enabled=False):
            return _NeckFuse.apply(a, b, c, weights.float(), int(col), int(mode_b), int(mode_c))
    with torch.autocast("cuda", enabled=False):
        return _NeckFuse.apply(a, b, c, None, 0, int(mode_b), int(mode_c))


class _MaxPool3x3s2(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        n, c, h, w = (int(v) for v in x.shape)
        dev = x.device
        x = x.detach()
        y = torch.empty((n, c, (h - 1) // 2 + 1, (w - 1) // 2 + 1), device=dev, dtype=x.dtype)
        with torch.cuda.device(dev):
            N.check(N.lib.ssdk_maxpool3x3s2_train_fwd(x.data_ptr(), y.data_ptr(), n, c, h, w, N.dtype_code(x), N.stream_ptr(dev)),
                    "maxpool3x3s2_train_fwd")
        STATS["pool_forward"] += 1
        ctx.save_for_backward(x)
        return y

    @staticmethod
    def backward(ctx, gy):
        (x,) = ctx.saved_tensors
        n, c, h, w = (int(v) for v in x.shape)
        dev = x.device
        gy = gy.contiguous()
        if gy.dtype != x.dtype:
            gy = gy.to(x.dtype)
        gx = torch.empty_like(x)
        with torch.cuda.device(dev):
            N.check(N.lib.ssdk_maxpool3x3s2_train_bwd(x.data_ptr(), gy.data_ptr(), gx.data_ptr(), n, c, h, w, N.dtype_code(x),
                                                      N.stream_ptr(dev)), "maxpool3x3s2_train_bwd")
        STATS["pool_backward"] += 1
        return gx


def maxpool3x3s2(x):
    """max_pool2d(x, 3, stride 2, pad 1) on csrc/ssdk_necktrain.hip, differentiable.  Explicit: a 16-bit contiguous NCHW tensor on a
    HIP device, anything else raises."""
    if not (torch.is_tensor(x) and x.is_cuda and x.dim() == 4 and x.dtype in _HALF and x.is_contiguous()):
        raise ValueError("maxpool3x3s2: a 16-bit contiguous NCHW tensor on a HIP device, got {} {} on {}".format(
            tuple(x.shape) if torch.is_tensor(x) else type(x), getattr(x, "dtype", None), getattr(x, "device", None)))
    return _MaxPool3x3s2.apply(x)


def _pair(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


def pool_supported(m):
    """``m`` is a max-pool 3x3 / stride 2 / pad 1 / dilation 1 in floor mode that returns no indices."""
    return (isinstance(m, nn.MaxPool2d) and _pair(m.kernel_size) == (3, 3) and _pair(m.stride) == (2, 2) and _pair(m.padding) == (1, 1)
            and _pair(m.dilation) == (1, 1) and not m.ceil_mode and not m.return_indices)


class TrainMaxPool3x3s2(nn.MaxPool2d):
    """``nn.MaxPool2d(3, 2, 1)`` whose 16-bit contiguous HIP-device forward / backward run on csrc/ssdk_necktrain.hip (no index
    tensor is kept); everything else is ``nn.MaxPool2d.forward``."""

    def forward(self, x):
        if not (x.is_cuda and x.dim() == 4 and x.dtype in _HALF and x.is_contiguous() and pool_supported(self)):
            return super(TrainMaxPool3x3s2, self).forward(x)
        return _MaxPool3x3s2.apply(x)


# what an unset SSDK_NECK_TRAIN means (train_routing.PASSES; docs/SWITCHES.md): every probed case and both step A/Bs
# favour the kernels.  1 routes the fusions, the top-down adds and the stem max-pool of the SSDFPN / SSDBiFPN training step to
# csrc/ssdk_necktrain.hip, 0 leaves them on the eager expressions
DEFAULT = "1"


def use_native_neck(model):
    """Enable the kernels on ``model`` in place (no new parameters, same ``state_dict``): every ``BiFPNModule`` and an ``SSDFPN`` get
    the flag their forward reads, a ``ResNet.maxpool`` that is a plain ``nn.MaxPool2d(3, 2, 1)`` becomes ``TrainMaxPool3x3s2``.
    -> model; STATS counts what was switched."""
    from ssds.modeling.nets.resnet import ResNet
    from ssds.modeling.ssds.bifpn import BiFPNModule
    from ssds.modeling.ssds.fpn import SSDFPN

    for m in model.modules():
        if isinstance(m, BiFPNModule) and not m.native_neck:
            m.native_neck = True
            STATS["bifpn_modules"] += 1
        elif isinstance(m, SSDFPN) and not m.native_neck:
            m.native_neck = True
            STATS["fpn_models"] += 1
        elif isinstance(m, ResNet) and type(m.maxpool) is nn.MaxPool2d and pool_supported(m.maxpool):
            m.maxpool.__class__ = TrainMaxPool3x3s2
            STATS["maxpools"] += 1
    return model
