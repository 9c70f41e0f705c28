"""The ShuffleNetV2 unit of the training step on the NCHW tensors themselves (csrc/ssdk_shuffletrain.hip, include/ssdk_shuffletrain.h):

    conv_slice(x, Cb, w)    y = W x[:, Cb:]        the first 1x1 of a stride-1 unit reads the second half of x where it lies
    join(left, right)       y[2i] = left[i], y[2i + 1] = right[i]        = channel_shuffle(cat((left, right), 1), 2)

PyTorch-ROCm runs a stride-1 unit as ``chunk`` (a view), ``nn.Conv2d`` on the non-contiguous half, ``cat`` and ``channel_shuffle``
(three passes over the unit's output) and splits and re-assembles the gradient the same way.  Here the slice is an image stride in
the 1x1 kernel, the join is one launch forward and one backward, and the gradient of ``x`` is written exactly once: the join's
backward writes ``gy[:, 0::2]`` into the first Cb channels of a fresh buffer, the slice convolution's backward writes its input
gradient into the last Cb channels of the same buffer and returns it -- no zero fill, no add of two full-size gradients.  The two
backward passes share one per-call object made in the unit's forward; the join takes ``x`` detached, so autograd sees one edge
into ``x``, and the join's backward always runs first (the convolution's incoming gradient depends on it).

``use_native_shuffle(model)`` enables the path per model; a model it was never called on runs the earlier expressions."""
import os

import torch
import torch.nn as nn

from ssds import _native as N
from ssds.modeling.layers import kernel_conv as K

STATS = {"units": 0, "depthwise": 0, "pointwise": 0, "slice_forward": 0, "slice_backward": 0, "join_forward": 0, "join_backward": 0}

# The longest chain of dependent fp32 additions a product of ssdk_pws_wgrad (= ssdk_pw_wgrad) passes through, the bar of
# tests/test_gpu_shuffle_train.py: |dW - truth| <= D 2^-24 sum |dy| |x|.  Both kernels (pw_wgrad_kernel, pw_wgrad_tiled_kernel):
#   a v_mfma_f32_16x16x32 adds 32 products and the accumulator -- counted as a chain of                         32
#   a pixel range is `cps` chunks of 128 pixels = 4 MFMAs each, chained through the accumulator                  4 cps
#   pw_wgrad_reduce_kernel: 16 partials in a chain (15) and the four quarters in order (3), one pass per factor
#   64 of the <= 4096 pixel ranges, so at most two passes                                                       2 (15 + 3)
# The products themselves are exact (two 16-bit values in fp32).  `cps` grows with the batch: wgrad_plan() below restates the
# library's plan (tests/test_shuffle_train_cpu.py holds it against ssdk_pws_wgrad_workspace_bytes).
def wgrad_sum_depth(cps):
    return 32 + 4 * int(cps) + 2 * (15 + 3)


# ... and a product of y = a x (ssdk_pws_forward = the kernels of ssdk_pw_forward): ceil(K / 32) MFMAs chained through the
# accumulator, which starts from the bias:                                                                      32 + ceil(K / 32)
def gemm_sum_depth(k):
    return 32 + (int(k) + 31) // 32


# ... and a term of the statistics sums (sum y, sum y^2 of the fp32 accumulators).  A wave visits `iters` pixel groups -- 1 whenever
# the groups of 128 pixels give the chip fewer workgroups than it has room for, as at every shape of the tests (<= 6 groups).
#   pw_gemm_short_kernel: the lane's 8 pixels (8), the xor tree over 16 lanes (4), the wave's own word once per group (iters)
#   pw_gemm_long_kernel: the lane's 8 pixels per group in one chain (8 iters), then the tree (4)
#   pw_wgrad_reduce_kernel, at most two passes: 2 (15 + 3); + 1 for the square, which is rounded before it is added
def stats_sum_depth(iters=1):
    return 8 * int(iters) + 4 + int(iters) + 2 * (15 + 3) + 1


def wgrad_plan(b, cout, cin, hw):
    """-> (tiled, splits, chunks per split) of ssdk_pws_wgrad, as csrc/ssdk_pwtrain_kernels.h pw_wgrad_plan decides them."""
    mf, nf = (cout + 15) // 16, (cin + 15) // 16
    chunks = b * ((hw + 127) // 128)
    tiled = mf >= 4 and nf >= 4
    if tiled:
        tiles, target = ((cout + 127) // 128) * ((cin + 127) // 128), 512
    else:
        mfw, nfw = min(mf, 3), (2 if nf >= 2 else 1)
        tiles, target = ((mf + mfw - 1) // mfw) * ((nf + nfw - 1) // nfw), 4096
    splits = min(max(target // tiles, 1), chunks)
    cps = (chunks + splits - 1) // splits
    return tiled, (chunks + cps - 1) // cps, cps


def slice_geometry(shape, cb):
    """(element offset, image stride) of ``x[:, cb:]`` in a contiguous NCHW tensor of ``shape`` -- what the kernels take as the
    pointer offset and the image stride of a slice."""
    _, c, h, w = (int(v) for v in shape)
    return int(cb) * h * w, c * h * w


def _pad8(v):
    return (int(v) + 7) // 8 * 8


def _kernel_tensor(t):
    return torch.is_tensor(t) and t.is_cuda and t.dim() == 4 and t.dtype in K.HALF and t.is_contiguous()


def _describe(t):
    return "{} {} on {}".format(tuple(t.shape) if torch.is_tensor(t) else type(t), getattr(t, "dtype", None), getattr(t, "device", None))


class _Shared(object):
    """What the two backward passes of one stride-1 unit call share: the gradient buffer of the unit's input."""
    __slots__ = ("buf",)

    def __init__(self):
        self.buf = None


def prepare_weights(w, dt):
    """weight [Cout, Cin, 1, 1] (fp32 master or 16 bit) -> w16 [Cout, Kp], wt16 [Cin, Mp] in ``dt``, zero-padded (ssdk_pws_prepare)."""
    cout, cin = int(w.shape[0]), int(w.shape[1])
    dev = w.device
    w16 = torch.empty((cout, _pad8(cin)), device=dev, dtype=dt)
    wt16 = torch.empty((cin, _pad8(cout)), device=dev, dtype=dt)
    w32 = w.detach().reshape(cout, cin).float().contiguous()  # (a no-op for the fp32 master parameter)
    N.check(N.lib.ssdk_pws_prepare(w32.data_ptr(), w16.data_ptr(), wt16.data_ptr(), cout, cin, N.BF16 if dt == torch.bfloat16 else N.F16,
                                   N.stream_ptr(dev)), "pws_prepare")
    return w16, wt16


def pws_forward(x_ptr, x_stride, a, bias, y_ptr, y_stride, b, k, m, hw, code, dev, want_sums=False):
    """One ssdk_pws_forward call on raw pointers (a: the padded matrix tensor [M, lda]); -> sums [M, 2] or None."""
    sums = ws = wp = None
    need = 0
    if want_sums:
        need = int(N.lib.ssdk_pws_stats_workspace_bytes(b, k, m, hw))
        ws, wp = K.workspace(dev, need)
        sums = torch.empty((m, 2), device=dev, dtype=torch.float32)
    N.check(N.lib.ssdk_pws_forward(x_ptr, x_stride, a.data_ptr(), int(a.shape[1]), None if bias is None else bias.data_ptr(), y_ptr, y_stride,
                                   None if sums is None else sums.data_ptr(), wp, need,
                                   b, k, m, hw, code, N.stream_ptr(dev)), "pws_forward")
    return sums


def pws_wgrad(gy, x_ptr, x_stride, b, cout, cin, hw, code, dev):
    """-> dW [Cout, Cin, 1, 1] fp32 of a 1x1 convolution whose input lies at ``x_ptr`` with images ``x_stride`` elements apart."""
    need = int(N.lib.ssdk_pws_wgrad_workspace_bytes(b, cout, cin, hw))
    ws, wp = K.workspace(dev, need)
    gw32 = torch.empty((cout, cin, 1, 1), device=dev, dtype=torch.float32)
    N.check(N.lib.ssdk_pws_wgrad(gy.data_ptr(), x_ptr, x_stride, gw32.data_ptr(), wp, need, b, cout, cin, hw, code,
                                 N.stream_ptr(dev)), "pws_wgrad")
    return gw32


class _ConvSlice(torch.autograd.Function):
    """y = W x[:, Cb:] of a contiguous 16-bit x [N, C, H, W] (C - Cb >= 8 input channels), W [M, C - Cb, 1, 1] fp32 or 16 bit.
    The gradient of x is a full-size buffer: the one ``share`` carries (its first Cb channels written by the join's backward), else
    a fresh one whose first Cb channels are zero-filled."""

    @staticmethod
    def forward(ctx, x, w, cb, share, want_sums):
        n, c, h, wd = (int(v) for v in x.shape)
        m, k, hw, dev, dt = int(w.shape[0]), c - cb, h * wd, x.device, x.dtype
        code = N.dtype_code(x)
        x = x.detach()
        off, stride = slice_geometry(x.shape, cb)
        with torch.cuda.device(dev):
            w16, wt16 = prepare_weights(w, dt)
            y = torch.empty((n, m, h, wd), device=dev, dtype=dt)
            sums = pws_forward(x.data_ptr() + 2 * off, stride, w16, None, y.data_ptr(), m * hw, n, k, m, hw, code, dev, want_sums)
        STATS["slice_forward"] += 1
        ctx.save_for_backward(x, wt16)
        ctx.meta = (cb, m, w.dtype, share)
        if want_sums:
            ctx.mark_non_differentiable(sums)
            ctx.set_materialize_grads(False)
            return y, sums
        return y

    @staticmethod
    def backward(ctx, gy, _gsums=None):
        x, wt16 = ctx.saved_tensors
        cb, m, wdt, share = ctx.meta
        if gy is None:
            return None, None, None, None, None
        n, c, h, wd = (int(v) for v in x.shape)
        k, hw, dev = c - cb, h * wd, x.device
        gy = gy.contiguous()
        if gy.dtype != x.dtype:
            gy = gy.to(x.dtype)
        code = N.dtype_code(x)
        off, stride = slice_geometry(x.shape, cb)
        gx = gw = None
        with torch.cuda.device(dev):
            if ctx.needs_input_grad[0]:
                gx = share.buf if share is not None else None
                if gx is None:  # (no join behind this call wrote the left half)
                    gx = torch.empty_like(x)
                    gx[:, :cb].zero_()
                else:
                    share.buf = None
                pws_forward(gy.data_ptr(), m * hw, wt16, None, gx.data_ptr() + 2 * off, stride, n, m, k, hw, code, dev)
            if ctx.needs_input_grad[1]:
                gw = pws_wgrad(gy, x.data_ptr() + 2 * off, stride, n, m, k, hw, code, dev)
                gw = gw if wdt == torch.float32 else gw.to(wdt)
        STATS["slice_backward"] += 1
        return gx, gw, None, None, None


class _Join(torch.autograd.Function):
    """y[2i] = left[i], y[2i + 1] = right[i].  ``half``: ``left`` is the unit's whole input x (detached by the caller), of which the
    first Cb channels are read; its gradient goes into ``share.buf`` (a fresh full-size buffer), not through autograd."""

    @staticmethod
    def forward(ctx, left, right, half, share):
        n, cb, h, wd = (int(v) for v in right.shape)
        dev, hw = right.device, h * wd
        left, right = left.detach(), right.detach()
        y = torch.empty((n, 2 * cb, h, wd), device=dev, dtype=right.dtype)
        with torch.cuda.device(dev):
            N.check(N.lib.ssdk_shuffle_join_fwd(left.data_ptr(), (2 if half else 1) * cb * hw, right.data_ptr(), y.data_ptr(), n, cb, hw,
                                                N.dtype_code(right), N.stream_ptr(dev)), "shuffle_join_fwd")
        STATS["join_forward"] += 1
        ctx.meta = ((n, cb, h, wd), right.dtype, half, share)
        return y

    @staticmethod
    def backward(ctx, gy):
        (n, cb, h, wd), dt, half, share = ctx.meta
        dev, hw = gy.device, h * wd
        gy = gy.contiguous()
        if gy.dtype != dt:
            gy = gy.to(dt)
        gright = torch.empty((n, cb, h, wd), device=dev, dtype=dt)
        gleft = ret = None
        stride = cb * hw
        if half:
            if share is not None:
                gleft = share.buf = torch.empty((n, 2 * cb, h, wd), device=dev, dtype=dt)
                stride = 2 * cb * hw
        elif ctx.needs_input_grad[0]:
            gleft = ret = torch.empty((n, cb, h, wd), device=dev, dtype=dt)
        with torch.cuda.device(dev):
            N.check(N.lib.ssdk_shuffle_join_bwd(gy.data_ptr(), None if gleft is None else gleft.data_ptr(), stride, gright.data_ptr(), n, cb, hw,
                                                N.dtype_code(gy), N.stream_ptr(dev)), "shuffle_join_bwd")
        STATS["join_backward"] += 1
        return ret, gright, None, None


def conv_slice(x, cb, weight, share=None, want_sums=False):
    """conv2d(x[:, cb:], weight) on csrc/ssdk_shuffletrain.hip without the chunk copy, differentiable in x and weight.  Explicit: a
    16-bit contiguous NCHW tensor on a HIP device, a dense 1x1 weight [M >= 8, C - cb >= 8, 1, 1] (fp32 master or x's dtype) on the
    same device; anything else raises.  ``want_sums``: -> (y, sums [M, 2])."""
    if not _kernel_tensor(x):
        raise ValueError("conv_slice: a 16-bit contiguous NCHW tensor on a HIP device, got " + _describe(x))
    cb = int(cb)
    k = int(x.shape[1]) - cb
    if not (torch.is_tensor(weight) and weight.dim() == 4 and tuple(weight.shape[2:]) == (1, 1) and weight.device == x.device
            and weight.dtype in (torch.float32, x.dtype)):
        raise ValueError("conv_slice: a 1x1 weight in fp32 or the tensor's dtype on its device, got " + _describe(weight))
    if cb < 0 or k < 8 or int(weight.shape[1]) != k or int(weight.shape[0]) < 8:
        raise ValueError("conv_slice: weight {} does not fit channels [{}:] of {} (at least 8 channels either side)".format(
            tuple(weight.shape), cb, tuple(x.shape)))
    if x.numel() == 0:
        raise ValueError("conv_slice: empty tensor")
    return _ConvSlice.apply(x, weight, cb, share, bool(want_sums))


def join(left, right, half=False, share=None):
    """channel_shuffle(cat((left, right), 1), 2) in one launch, differentiable.  ``half``: ``left`` is a tensor of 2 Cb channels whose
    FIRST Cb are the operand (the unit's input; no gradient flows to it through autograd -- see ``_Join``).  Explicit: 16-bit
    contiguous NCHW tensors of one dtype on one HIP device whose shapes fit, anything else raises."""
    for t in (left, right):
        if not _kernel_tensor(t):
            raise ValueError("join: 16-bit contiguous NCHW tensors on a HIP device, got " + _describe(t))
    if left.dtype != right.dtype or left.device != right.device:
        raise ValueError("join: the operands differ in dtype or device")
    n, cb, h, w = (int(v) for v in right.shape)
    if tuple(left.shape) != (n, 2 * cb if half else cb, h, w) or right.numel() == 0:
        raise ValueError("join: left {} does not fit right {} (half={})".format(tuple(left.shape), tuple(right.shape), half))
    return _Join.apply(left.detach() if half else left, right, bool(half), share)


def _kernel_inputs(*tensors):
    """The tensors as the kernels take them -- under autocast cast to its dtype, the contract of neckfuse.try_fuse -- or None when
    one of them is not a 16-bit contiguous NCHW tensor on a HIP device, or they differ in dtype or device."""
    autocast = torch.is_autocast_enabled()
    out = []
    for t in tensors:
        if not (torch.is_tensor(t) and t.is_cuda and t.dim() == 4):
            return None
        if autocast:
            t = t.to(torch.get_autocast_dtype("cuda"))
        if t.dtype not in K.HALF or not t.is_contiguous() or t.numel() == 0 or (out and (t.dtype != out[0].dtype or t.device != out[0].device)):
            return None
        out.append(t)
    return out


def try_join(left, right):
    """``join`` of two whole tensors when they meet its contract (under autocast after the cast to its dtype), else None: the caller
    runs its eager expression."""
    srcs = _kernel_inputs(left, right)
    if srcs is None or srcs[0].shape != srcs[1].shape:
        return None
    with torch.autocast("cuda", enabled=False):
        return _Join.apply(srcs[0], srcs[1], False, None)


def _slice_conv(conv, cb):
    """``conv`` is a 1x1 layer the slice kernel computes: a marked PointwiseConv2d, dense, stride 1, no bias, >= 8 channels either side."""
    from ssds.modeling.layers.pointwise import PointwiseConv2d

    return (type(conv) is PointwiseConv2d and conv._ssdk_any_width and conv.kernel_size == (1, 1) and conv.stride == (1, 1)
            and conv.padding == (0, 0) and conv.dilation == (1, 1) and conv.groups == 1 and conv.bias is None
            and conv.in_channels == cb >= 8 and conv.out_channels >= 8 and os.environ.get("SSDK_PW_NATIVE", "1") != "0")


def try_unit(unit, x):
    """The forward of a flagged ``shufflenet.InvertedResidual`` on the kernels, or None when ``x`` is outside their contract (CPU,
    fp32 without autocast, channels_last, an odd number of channels, a first 1x1 that is not a marked PointwiseConv2d): the unit
    then runs its eager expressions."""
    srcs = _kernel_inputs(x)
    if srcs is None:
        return None
    xk = srcs[0]
    if unit.stride != 1:
        left, right = unit.branch1(x), unit.branch2(x)
        out = try_join(left, right)
        if out is None:  # (the branches ran: they are not run again)
            from ssds.modeling.nets.shufflenet import channel_shuffle

            out = channel_shuffle(torch.cat((left, right), dim=1), 2)
        return out
    c = int(xk.shape[1])
    cb = c // 2
    mods = list(unit.branch2.children())
    if c % 2 or not mods or not _slice_conv(mods[0], cb):
        return None
    conv = mods[0]
    w = conv.weight
    if w.dtype not in (torch.float32, xk.dtype) or w.device != xk.device:
        return None
    from ssds.modeling.layers.pointwise import BN_STATS_MIN_BYTES

    share = _Shared() if (torch.is_grad_enabled() and xk.requires_grad) else None
    want = (conv._ssdk_bn_follows and conv.training
            and xk.shape[0] * conv.out_channels * xk.shape[2] * xk.shape[3] * 2 >= BN_STATS_MIN_BYTES)
    with torch.autocast("cuda", enabled=False):
        if want:
            r, sums = _ConvSlice.apply(xk, w, cb, share, True)
            r._ssdk_bn_sums = sums
        else:
            r = _ConvSlice.apply(xk, w, cb, share, False)
    for m in mods[1:]:
        r = m(r)
    rk = _kernel_inputs(r)
    if rk is None or rk[0].dtype != xk.dtype or tuple(rk[0].shape) != (int(xk.shape[0]), cb, int(xk.shape[2]), int(xk.shape[3])):
        # (a branch that left the contract: the eager join; the slice convolution then finds no buffer and zero-fills the left half)
        from ssds.modeling.nets.shufflenet import channel_shuffle

        return channel_shuffle(torch.cat((xk[:, :cb], r), dim=1), 2)
    with torch.autocast("cuda", enabled=False):
        return _Join.apply(xk.detach(), rk[0], True, share)


# what an unset SSDK_SHUFFLE_TRAIN means (train_routing.PASSES; docs/SWITCHES.md): 1 routes the ShuffleNetV2 units of the
# training step to csrc/ssdk_shuffletrain.hip and the project's depthwise kernels, 0 leaves them on chunk / cat / channel_shuffle and nn.Conv2d
DEFAULT = "1"


def _dense_1x1(m):
    return (isinstance(m, nn.Conv2d) and m.kernel_size == (1, 1) and m.stride == (1, 1) and m.padding == (0, 0) and m.groups == 1
            and m.dilation == (1, 1))


def use_native_shuffle(model):
    """Enable the kernels on ``model`` in place (no new parameters, same ``state_dict``), wherever it has a ShuffleNetV2 backbone:
      * every ``shufflenet.InvertedResidual`` gets the flag its forward reads;
      * every ``nn.Conv2d(C, C, 3, s, 1, groups=C, bias=False)`` of the backbone becomes a ``dwconv.DepthwiseConv2d`` (class swap);
      * every dense 1x1 of the backbone, and every other dense 1x1 of the model whose input width is no multiple of 8 (the FPN
        laterals on the 116-channel map), is marked: as a ``PointwiseConv2d`` it may take the any-width kernels.
    -> model; STATS counts what was switched.  A model without such a backbone is not touched."""
    from ssds.modeling.layers.dwconv import DepthwiseConv2d
    from ssds.modeling.nets.shufflenet import InvertedResidual, ShuffleNetV2

    # (a ShuffleNetV2, or units that stand alone; a unit inside a backbone is met twice, the second time already switched)
    backbones = [m for m in model.modules() if isinstance(m, (ShuffleNetV2, InvertedResidual))]
    if not backbones:
        return model
    for bb in backbones:
        STATS["depthwise"] += K.swap_layers(bb, DepthwiseConv2d, also=lambda m: m.groups > 1)
        for m in bb.modules():
            if isinstance(m, InvertedResidual) and not m.__dict__.get("native_shuffle", False):
                m.native_shuffle = True
                STATS["units"] += 1
            elif _dense_1x1(m) and not m.__dict__.get("_ssdk_any_width", False):
                m._ssdk_any_width = True
                STATS["pointwise"] += 1
    for m in model.modules():
        if _dense_1x1(m) and m.in_channels % 8 != 0 and m.in_channels >= 8 and not m.__dict__.get("_ssdk_any_width", False):
            m._ssdk_any_width = True
            STATS["pointwise"] += 1
    return model
