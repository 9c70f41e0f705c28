"""The DenseNet dense block of the training step on ONE feature buffer (csrc/ssdk_densetrain.hip, include/ssdk_densetrain.h).

``_DenseLayer.forward`` in train mode re-concatenates everything before the layer, runs a full BatchNorm over those Cin_j channels
(statistics pass, apply pass, a stored output), keeps both Cin_j-wide tensors for backward, and autograd splits the gradient of the
concatenation into j + 1 slices that it adds one by one: memory and traffic quadratic in the depth of a block.  ``TrainDenseBlock``
runs the whole block as ONE ``torch.autograd.Function`` on a feature buffer F [N, Ctot, H, W] and a gradient buffer G of that shape:

    forward   place(x -> F[:, :C0], + the channels' (sum, sum of squares))
              per layer j, K = C0 + 32 j:
                norm1      ssdk_bn_act_train_stats on the PREFIX [0, K) of the block's sums: a finalize, no pass over the data --
                           channel c holds the same data for every later layer, its statistics are computed once, when it is written
                conv1      ssdk_dense_train_pw_forward: m = W1 op(F[:, :K]), op = relu(norm1(.)) applied on load, + the sums of m
                norm2+relu ssdk_bn_act_train_fwd_sums (act = 2)
                conv2      ssdk_conv3x3_train_forward -> a 32-channel temporary
                place      the temporary -> F[:, K : K + 32], + its sums
              returns F itself
    backward  G = clone of the incoming gradient; layers in reverse:
                conv2      ssdk_conv3x3_train_dgrad / _wgrad on a contiguous copy of G[:, K : K + 32]
                norm2+relu ssdk_bn_act_train_bwd
                conv1      ssdk_dense_train_pw_wgrad (op on load again), ssdk_pws_forward: s = W1^T dm into a shared scratch
                norm1      ssdk_dense_train_bn1_reduce, ssdk_dense_train_bn1_apply: G[:, :K] += dx (fp32 add, one rounding -- the
                           rounding autograd's own accumulation of 16-bit gradients makes)
              returns G[:, :C0] and fp32 gradients of every parameter

Saved for backward: F, each layer's m (128 channels) and relu2 output (128 channels; SAVED rather than rebuilt with
ssdk_bn_act_apply), the small fp32 vectors and the 16-bit weight images.  No ``cat``, no stored relu(norm1(x)).

The swap is at block level (``use_native_dense_block`` sets ``block.__class__``): same modules, parameters, buffers and
``state_dict`` keys.  Eval mode, CPU tensors, fp32 without autocast, ``drop_rate > 0`` and synchronised BatchNorm layers run
``_DenseBlock.forward`` (counted in STATS["fallback"], reasons in FALLBACK_REASONS).  DESIGN.md 4.5o."""
import collections

import torch
import torch.nn as nn

from ssds import _native as N
from ssds.modeling.layers import denseconv
from ssds.modeling.layers import kernel_conv as K
from ssds.modeling.layers import shuffletrain as ST
from ssds.modeling.layers.batchnorm import _ws as _bn_ws
from ssds.modeling.nets.densenet import _DenseBlock, _DenseLayer

GROWTH, CMID = 32, 128  # the widths the path is built and tested for (DenseNet121 / 169 / 201): conv2 is 128 -> 32
STATS = {"swapped": 0, "native_forward": 0, "forward_layers": 0, "backward_layers": 0, "fallback": 0}
FALLBACK_REASONS = collections.Counter()  # reason -> count of the forwards that took _DenseBlock.forward


# ---- summation depths: the longest chain of dependent fp32 additions a term passes through (the bars of tests/test_gpu_dense_train.py)
# dense_reduce_kernel (ssdk_dense_train_place, ssdk_dense_train_bn1_reduce), workgroup (channel, s) of S = reduce_split(n, c):
#   its images are s, s + S, ...: at most ceil(n / S); an item is (image, run of 8 pixels), a thread takes items tid, tid + 256, ...
#   and adds each item's 8 elements one after the other                                       8 ceil(ceil(n / S) ceil(hw / 8) / 256)
#   the xor butterfly over the 64 lanes (6), the four waves in order (3)                      6 + 3
#   dense_finalize_kernel: the S partials of the channel in index order                       S - 1
#   + 1: the square (place) / the product g xhat (bn1_reduce) is rounded before it is added   1
def reduce_split(n, c):
    """The number of image ranges a channel's reduction is split into (csrc/ssdk_densetrain.hip dense_split)."""
    return max(1, min((2048 + int(c) - 1) // int(c), int(n), 64))


def reduce_sum_depth(n, c, hw):
    s = reduce_split(n, c)
    items = ((int(n) + s - 1) // s) * ((int(hw) + 7) // 8)
    return 8 * ((items + 255) // 256) + 6 + 3 + (s - 1) + 1


place_sum_depth = bn1_sum_depth = reduce_sum_depth


# ssdk_dense_train_pw_forward / _pw_wgrad are the kernels of ssdk_pws_forward / ssdk_pws_wgrad with the operand transform: op(x) is
# formed per element BEFORE the MFMAs and adds nothing to a chain, so their depths are those of shuffletrain (same plan, same order).
def pw_gemm_sum_depth(k):
    return ST.gemm_sum_depth(k)


def pw_stats_sum_depth(iters=1):
    return ST.stats_sum_depth(iters)


def pw_wgrad_sum_depth(b, m, k, hw):
    return ST.wgrad_sum_depth(ST.wgrad_plan(b, m, k, hw)[2])


# ---- the five entry points on raw pointers (the block function and the tests share them) ---------------------------------------
def place(t, y_ptr, y_stride, sums_ptr, n, c, hw, code, dev):
    """ssdk_dense_train_place: contiguous t [n, c, hw] -> the slice at ``y_ptr``; (sum, sum of squares) -> ``sums_ptr`` [c, 2]."""
    need = int(N.lib.ssdk_dense_train_place_workspace_bytes(n, c, hw))
    ws, wp = K.workspace(dev, need)
    N.check(N.lib.ssdk_dense_train_place(t.data_ptr(), y_ptr, y_stride, sums_ptr, wp, need, n, c, hw, code, N.stream_ptr(dev)),
            "dense_train_place")


def pw_forward(x_ptr, x_stride, coef, a, m, b, k, cm, hw, code, dev, want_sums=True):
    """ssdk_dense_train_pw_forward: m [b, cm, hw] = a op(x); -> sums [cm, 2] or None."""
    sums = ws = wp = None
    need = 0
    if want_sums:
        need = int(N.lib.ssdk_pws_stats_workspace_bytes(b, k, cm, hw))
        ws, wp = K.workspace(dev, need)
        sums = torch.empty((cm, 2), device=dev, dtype=torch.float32)
    N.check(N.lib.ssdk_dense_train_pw_forward(x_ptr, x_stride, coef.data_ptr(), a.data_ptr(), int(a.shape[1]), m.data_ptr(),
                                              None if sums is None else sums.data_ptr(), wp, need,
                                              b, k, cm, hw, code, N.stream_ptr(dev)), "dense_train_pw_forward")
    return sums


def pw_wgrad(dm, x_ptr, x_stride, coef, b, cm, k, hw, code, dev):
    """ssdk_dense_train_pw_wgrad -> dW [cm, k, 1, 1] fp32."""
    need = int(N.lib.ssdk_pws_wgrad_workspace_bytes(b, cm, k, hw))
    ws, wp = K.workspace(dev, need)
    gw = torch.empty((cm, k, 1, 1), device=dev, dtype=torch.float32)
    N.check(N.lib.ssdk_dense_train_pw_wgrad(dm.data_ptr(), x_ptr, x_stride, coef.data_ptr(), gw.data_ptr(), wp, need, b, cm, k,
                                            hw, code, N.stream_ptr(dev)), "dense_train_pw_wgrad")
    return gw


def bn1_reduce(s_ptr, x_ptr, x_stride, coef, mean, invstd, n, k, hw, code, dev):
    """ssdk_dense_train_bn1_reduce -> red [k, 2] fp32 = (d bias, d weight) of norm1."""
    need = int(N.lib.ssdk_dense_train_bn1_workspace_bytes(n, k, hw))
    ws, wp = K.workspace(dev, need)
    red = torch.empty((k, 2), device=dev, dtype=torch.float32)
    N.check(N.lib.ssdk_dense_train_bn1_reduce(s_ptr, x_ptr, x_stride, coef.data_ptr(), mean.data_ptr(), invstd.data_ptr(), red.data_ptr(),
                                              wp, need, n, k, hw, code, N.stream_ptr(dev)), "dense_train_bn1_reduce")
    return red


def bn1_apply(s_ptr, x_ptr, x_stride, coef, mean, invstd, weight, red, g_ptr, g_stride, n, k, hw, code, dev):
    """ssdk_dense_train_bn1_apply: the prefix [0, k) of the gradient buffer at ``g_ptr`` += norm1's input gradient."""
    N.check(N.lib.ssdk_dense_train_bn1_apply(s_ptr, x_ptr, x_stride, coef.data_ptr(), mean.data_ptr(), invstd.data_ptr(), weight.data_ptr(),
                                             red.data_ptr(), g_ptr, g_stride, n, k, hw, code, N.stream_ptr(dev)), "dense_train_bn1_apply")


# ---- the block ---------------------------------------------------------------------------------------------------------------------
def _momentum(bn):
    """nn.BatchNorm2d's bookkeeping for one training forward (as FastBatchNorm2d.forward does it) -> the momentum of this step."""
    if not getattr(bn, "_ssdk_counter_external", False):
        bn.num_batches_tracked.add_(1)
    return bn.momentum if bn.momentum is not None else 1.0 / float(bn.num_batches_tracked)


def layer_forward(F, bsums, k, layer, params, momenta=None):
    """Layer ``layer`` of a block on the buffer F [N, Ctot, H, W]: reads the channels [0, k) and the prefix [0, k) of the block's sums
    ``bsums`` [Ctot, 2], writes the channels [k, k + 32) and their sums.  ``params``: norm1.weight, norm1.bias, conv1.weight,
    norm2.weight, norm2.bias, conv2.weight.  ``momenta``: (norm1's, norm2's) for this step; None: the modules' bookkeeping runs.
    -> what the backward needs: m, relu2 output, mean1, invstd1, coef1, mean2, invstd2, wt16, the input-gradient image of conv2."""
    n, ctot, h, w = (int(v) for v in F.shape)
    hw, dev, dt = h * w, F.device, F.dtype
    code, sp, fs = N.dtype_code(F), N.stream_ptr(dev), ctot * hw
    g1, b1, w1, g2, b2, w2 = params
    bn1, bn2 = layer.norm1, layer.norm2
    mom1, mom2 = momenta if momenta is not None else (_momentum(bn1), _momentum(bn2))
    mean1 = torch.empty(k, device=dev, dtype=torch.float32)
    invstd1 = torch.empty(k, device=dev, dtype=torch.float32)
    coef1 = torch.empty((k, 4), device=dev, dtype=torch.float32)
    wp, need = _bn_ws(dev, n, k)
    N.check(N.lib.ssdk_bn_act_train_stats(F.data_ptr(), bsums.data_ptr(), g1.data_ptr(), b1.data_ptr(), bn1.running_mean.data_ptr(),
                                          bn1.running_var.data_ptr(), mean1.data_ptr(), invstd1.data_ptr(), coef1.data_ptr(), wp, need, n, k,
                                          hw, float(mom1), float(bn1.eps), code, sp), "bn_train_stats")
    w16, wt16 = ST.prepare_weights(w1, dt)
    m = torch.empty((n, CMID, h, w), device=dev, dtype=dt)
    sums2 = pw_forward(F.data_ptr(), fs, coef1, w16, m, n, k, CMID, hw, code, dev)
    r2 = torch.empty_like(m)
    mean2 = torch.empty(CMID, device=dev, dtype=torch.float32)
    invstd2 = torch.empty(CMID, device=dev, dtype=torch.float32)
    wp, need = _bn_ws(dev, n, CMID)
    N.check(N.lib.ssdk_bn_act_train_fwd_sums(m.data_ptr(), sums2.data_ptr(), g2.data_ptr(), b2.data_ptr(), bn2.running_mean.data_ptr(),
                                             bn2.running_var.data_ptr(), r2.data_ptr(), mean2.data_ptr(), invstd2.data_ptr(), wp, need, n,
                                             CMID, hw, float(mom2), float(bn2.eps), 2, code, sp), "bn_train_fwd_sums")
    img, dimg = denseconv.prepare_images(w2, dt, want_dgrad=True)
    t = torch.empty((n, GROWTH, h, w), device=dev, dtype=dt)
    N.check(N.lib.ssdk_conv3x3_train_forward(r2.data_ptr(), img.data_ptr(), None, t.data_ptr(), n, CMID, GROWTH, h, w, 1, code, sp),
            "conv3x3_train_forward")
    place(t, F.data_ptr() + 2 * k * hw, fs, bsums.data_ptr() + 8 * k, n, GROWTH, hw, code, dev)
    return [m, r2, mean1, invstd1, coef1, mean2, invstd2, wt16, dimg]


def layer_backward(F, G, scratch, k, saved, params, need, flows):
    """The backward of that layer on the gradient buffer G (shape of F): reads G[:, k : k + 32], adds norm1's input gradient to
    G[:, :k] when ``flows`` (somebody reads it afterwards).  ``scratch``: >= N k HW elements of F's dtype.  ``need``: which of the six
    parameter gradients are wanted.  -> the six gradients (fp32 or None), in the order of ``params``."""
    n, ctot, h, w = (int(v) for v in F.shape)
    hw, dev = h * w, F.device
    code, sp, fs = N.dtype_code(F), N.stream_ptr(dev), ctot * hw
    m, r2, mean1, invstd1, coef1, mean2, invstd2, wt16, dimg = saved
    g1, b1, w1, g2, b2, w2 = params
    grads = [None] * 6
    gnew = G[:, k:k + GROWTH].contiguous()
    dr2 = torch.empty_like(r2)
    N.check(N.lib.ssdk_conv3x3_train_dgrad(gnew.data_ptr(), dimg.data_ptr(), dr2.data_ptr(), n, CMID, GROWTH, h, w, 1, code, sp),
            "conv3x3_train_dgrad")
    if need[5]:
        nb = int(N.lib.ssdk_conv3x3_train_wgrad_workspace_bytes(n, CMID, GROWTH, h, w, 1))
        ws, wp = K.workspace(dev, nb)
        grads[5] = torch.empty((GROWTH, CMID, 3, 3), device=dev, dtype=torch.float32)
        N.check(N.lib.ssdk_conv3x3_train_wgrad(r2.data_ptr(), gnew.data_ptr(), grads[5].data_ptr(), wp, nb, n, CMID, GROWTH, h, w, 1,
                                               code, sp), "conv3x3_train_wgrad")
    dm = torch.empty_like(m)
    gg2 = torch.empty(CMID, device=dev, dtype=torch.float32)
    gb2 = torch.empty(CMID, device=dev, dtype=torch.float32)
    wp, nb = _bn_ws(dev, n, CMID)
    N.check(N.lib.ssdk_bn_act_train_bwd(m.data_ptr(), dr2.data_ptr(), g2.data_ptr(), b2.data_ptr(), mean2.data_ptr(), invstd2.data_ptr(),
                                        dm.data_ptr(), gg2.data_ptr(), gb2.data_ptr(), wp, nb, n, CMID, hw, 2, code, sp), "bn_train_bwd")
    grads[3], grads[4] = (gg2 if need[3] else None), (gb2 if need[4] else None)
    if need[2]:
        grads[2] = pw_wgrad(dm, F.data_ptr(), fs, coef1, n, CMID, k, hw, code, dev)
    if not (flows or need[0] or need[1]):
        return grads
    ST.pws_forward(dm.data_ptr(), CMID * hw, wt16, None, scratch.data_ptr(), k * hw, n, CMID, k, hw, code, dev)
    red = bn1_reduce(scratch.data_ptr(), F.data_ptr(), fs, coef1, mean1, invstd1, n, k, hw, code, dev)
    grads[0], grads[1] = (red[:, 1].contiguous() if need[0] else None), (red[:, 0].contiguous() if need[1] else None)
    if flows:
        bn1_apply(scratch.data_ptr(), F.data_ptr(), fs, coef1, mean1, invstd1, g1, red, G.data_ptr(), fs, n, k, hw, code, dev)
    return grads


class _DenseBlockTrain(torch.autograd.Function):
    """x [N, C0, H, W] 16 bit, contiguous; ``params``: per layer norm1.weight, norm1.bias, conv1.weight, norm2.weight, norm2.bias,
    conv2.weight (fp32 masters).  -> F [N, C0 + 32 L, H, W]."""

    @staticmethod
    def forward(ctx, x, block, *params):
        layers = list(block.values())
        n, c0, h, w = (int(v) for v in x.shape)
        hw, dev, dt = h * w, x.device, x.dtype
        ctot = c0 + GROWTH * len(layers)
        x = x.detach()
        saved = []
        with torch.cuda.device(dev):
            F = torch.empty((n, ctot, h, w), device=dev, dtype=dt)
            bsums = torch.empty((ctot, 2), device=dev, dtype=torch.float32)  # the block's (sum, sum of squares) per channel
            place(x, F.data_ptr(), ctot * hw, bsums.data_ptr(), n, c0, hw, N.dtype_code(x), dev)
            for j, layer in enumerate(layers):
                saved += layer_forward(F, bsums, c0 + GROWTH * j, layer, params[6 * j:6 * j + 6])
        STATS["forward_layers"] += len(layers)
        ctx.save_for_backward(F, *(saved + list(params)))
        ctx.meta = (len(layers), c0)
        return F

    @staticmethod
    def backward(ctx, gF):
        nl, c0 = ctx.meta
        F = ctx.saved_tensors[0]
        saved, params = ctx.saved_tensors[1:1 + 9 * nl], ctx.saved_tensors[1 + 9 * nl:]
        n, _, h, w = (int(v) for v in F.shape)
        dev, dt = F.device, F.dtype
        need_grad = ctx.needs_input_grad
        grads = [None] * (6 * nl)
        with torch.cuda.device(dev):
            G = gF.to(dt).clone(memory_format=torch.contiguous_format)  # the ONE gradient buffer of the block
            scratch = torch.empty((n, c0 + GROWTH * (nl - 1), h * w), device=dev, dtype=dt)  # s = W1^T dm, shared by the layers
            for j in reversed(range(nl)):
                grads[6 * j:6 * j + 6] = layer_backward(F, G, scratch, c0 + GROWTH * j, saved[9 * j:9 * j + 9], params[6 * j:6 * j + 6],
                                                        need_grad[2 + 6 * j:2 + 6 * j + 6], j > 0 or need_grad[0])
        STATS["backward_layers"] += nl
        for i, p in enumerate(params):  # (parameters are fp32 masters; anything else gets its own dtype back)
            if grads[i] is not None and grads[i].dtype != p.dtype:
                grads[i] = grads[i].to(p.dtype)
        return (G[:, :c0] if need_grad[0] else None, None) + tuple(grads)


def _is_sync(bn):
    return isinstance(bn, nn.SyncBatchNorm) or bool(getattr(bn, "_ssdk_sync", False))


def unsupported_reason(block):
    """None when ``block`` is a ``_DenseBlock`` the kernels take, else the reason by name."""
    if not isinstance(block, _DenseBlock):
        return "not a _DenseBlock"
    layers = list(block.values())
    if not layers or not all(isinstance(l, _DenseLayer) for l in layers):
        return "not a block of _DenseLayer modules"
    c0 = layers[0].conv1.in_channels
    for j, l in enumerate(layers):
        if l.drop_rate > 0:
            return "drop_rate > 0"
        c1, c2 = l.conv1, l.conv2
        if c2.out_channels != GROWTH:
            return "growth {} (the kernels are built for {})".format(c2.out_channels, GROWTH)
        if c1.out_channels != CMID or c2.in_channels != CMID:
            return "bottleneck width {} (the kernels are built for {})".format(c1.out_channels, CMID)
        if c1.in_channels != c0 + GROWTH * j or c0 < 8:
            return "input widths do not follow C0 + {} j with C0 >= 8".format(GROWTH)
        if (c1.kernel_size, c1.stride, c1.padding, c1.groups, c1.bias) != ((1, 1), (1, 1), (0, 0), 1, None) or not denseconv.supported(c2) \
                or c2.stride != (1, 1) or c2.bias is not None:
            return "convolutions outside the 1x1 / 3x3 contracts"
        for bn in (l.norm1, l.norm2):
            if not (isinstance(bn, nn.modules.batchnorm._BatchNorm) and bn.affine and bn.track_running_stats):
                return "BatchNorm without affine parameters or running statistics"
    return None


def supported(block):
    return unsupported_reason(block) is None


class TrainDenseBlock(_DenseBlock):
    """``_DenseBlock`` whose training forward on a 16-bit HIP tensor (or under autocast to one: the contract of ``DenseConv3x3``)
    is one ``_DenseBlockTrain``; everything else is ``_DenseBlock.forward``."""

    def _decline(self, x):
        if not self.training:
            return "eval mode"
        if not (torch.is_tensor(x) and x.is_cuda and x.dim() == 4 and x.numel() > 0):
            return "not a 4-d tensor on a HIP device"
        dt = torch.get_autocast_dtype("cuda") if torch.is_autocast_enabled() else x.dtype
        if dt not in K.HALF:
            return "fp32 without autocast"
        for l in self.values():
            if l.drop_rate > 0:
                return "drop_rate > 0"
            if _is_sync(l.norm1) or _is_sync(l.norm2):
                return "synchronised BatchNorm"
            if any(p.dtype != torch.float32 or p.device != x.device for p in l.parameters()):
                return "parameters that are not fp32 masters on the tensor's device"
        return None

    def forward(self, init_features):
        why = self._decline(init_features)
        if why is not None:
            STATS["fallback"] += 1
            FALLBACK_REASONS[why] += 1
            return super(TrainDenseBlock, self).forward(init_features)
        x = init_features
        if torch.is_autocast_enabled():
            x = x.to(torch.get_autocast_dtype("cuda"))
        x = x.contiguous()
        params = []
        for l in self.values():
            params += [l.norm1.weight, l.norm1.bias, l.conv1.weight, l.norm2.weight, l.norm2.bias, l.conv2.weight]
        STATS["native_forward"] += 1
        with torch.autocast("cuda", enabled=False):
            return _DenseBlockTrain.apply(x, self, *params)


def use_native_dense_block(model):
    """Switch every supported ``_DenseBlock`` of ``model`` to ``TrainDenseBlock`` (in place: same modules, parameters, buffers and
    ``state_dict`` keys).  -> blocks switched."""
    n = 0
    for m in model.modules():
        if type(m) is _DenseBlock and supported(m):
            m.__class__ = TrainDenseBlock
            n += 1
    STATS["swapped"] += n
    return n


# what an unset SSDK_DENSE_TRAIN means (train_routing.PASSES; docs/SWITCHES.md): 1 routes the dense blocks of a DenseNet
# backbone's training step to csrc/ssdk_densetrain.hip, 0 leaves them on ``_DenseBlock.forward`` (torch.cat and a full BatchNorm per layer)
DEFAULT = "0"
