"""The EfficientNet MBConv block inside the training step (nets/efficientnet.py ``MBConvBlock``) on csrc/ssdk_mbconvtrain.hip: the
5x5 depthwise convolution (forward, input gradient, weight gradient) and SiLU + squeeze-excite behind the depthwise BatchNorm as ONE
function of that BatchNorm's output ``u`` -- ``z = silu(u) * g``, ``g = sigmoid(W2 silu(W1 mean_hw(silu(u)) + b1) + b2)`` -- whose
``silu(u)`` is never stored.  The swap is at BLOCK level (``use_native_mbconv`` sets ``blk.__class__``): the convolution modules keep
their classes, parameters and ``state_dict`` keys.  DESIGN.md 4.6b."""
import torch

from ssds import _native as N
from ssds.modeling.layers import kernel_conv as K
from ssds.modeling.nets.efficientnet import MBConvBlock

STATS = {"swapped": 0, "native_forward": 0, "fallback": 0}
MAX_C, MAX_R = 4096, 1024  # csrc/ssdk_mbconvtrain.hip kSeMaxC / kSeMaxR (LDS of the gate kernels)


# ---- summation depths: the longest chain of dependent fp32 additions a term passes through (the bars of tests/mbconvjudge.py) ----
def dw5_parts(n, c, h, w, stride):
    """workgroup partials per (channel, tap) of the weight gradient -- from the library's own workspace size"""
    return int(N.lib.ssdk_dwconv5_bwd_weight_workspace_bytes(n, c, h, w, stride)) // (25 * 4 * c)


def DW5_SUM_DEPTH(n, c, h, w, stride):
    """dw5_wgrad_kernel: a thread adds the 8 products of its unit into acc[tap] by fused multiply-adds (8), the xor tree of the wave
    (6), the four waves in order (3); dw5_wgrad_reduce_kernel: lane l adds the partials l, l + 64, ... (P = ceil(parts / 64)), then
    the xor tree (6).  The product of two 16-bit values is exact in fp32 and the fused multiply-add rounds once, so nothing is added
    for the products."""
    return 8 + 6 + 3 + (dw5_parts(n, c, h, w, stride) + 63) // 64 + 6


def _chunk(hw):
    """se_sum_kernel: elements per wave -- the plane (a wave per plane below 1024 pixels) or a quarter of it rounded up to octets"""
    return hw if hw < 1024 else ((hw + 3) // 4 + 7) // 8 * 8


def SE_RED_DEPTH(hw):
    """se_sum_kernel: lane l owns the octets l, l + 64, ... of its wave's range, element e of every octet in accumulator e
    (ceil(chunk / 512) additions), the eight accumulators as a tree (3), the xor tree (6), and above 1023 pixels the four waves in
    order (3)."""
    return (_chunk(hw) + 511) // 512 + 3 + 6 + (3 if hw >= 1024 else 0)


def SE_POOL_DEPTH(hw):
    """... and the mean: 1 / HW is rounded (1) and multiplied on (1)."""
    return SE_RED_DEPTH(hw) + 2


def SE_FC1_DEPTH(c):
    """se_gate_kernel FC1 (and se_gate_bwd_kernel's W2^T dv2): a lane adds channels l, l + 64, ... (ceil(C / 64) fused multiply-adds),
    the xor tree (6), the bias (1)."""
    return (int(c) + 63) // 64 + 6 + 1


def SE_FC2_DEPTH(r):
    """se_gate_kernel FC2: Cr fused multiply-adds in index order, the bias (1)."""
    return int(r) + 1


def SE_GATE_BWD_DEPTHS(n, c, cr):
    """ssdk_se_gate_bwd, per output D with |err| <= D u mass (masses in tests/mbconvjudge.py).  With A = |dgate_raw| g (1 - g):
      dv2 = (dgate_raw g)(1 - g): three roundings                                            |d dv2| <= 3 u A
      s = silu(hp): fast exp + reciprocal (4 u each) and the product                          |d s|   <= 9 u |hp|
      ds = W2^T dv2: ceil(C / 64) + 6 additions on terms that are 3 u off                     |d ds|  <= (ceil(C / 64) + 9) u Ms, Ms = |W2|^T A
      silu'(hp) = s (1 + hp (1 - s)): sigmoid 9 u, 1 - s (1), hp (1 - s) (1), 1 + . (1), the product (1) propagate to
                                                                                              |d silu'| <= 21 u (1 + |hp|), |silu'| <= 1.1
      dh = ds silu'(hp)                       |d dh| <= (1.1 (ceil(C / 64) + 9) + 21 + 1.1) u Ms (1 + |hp|) =: Dh u Mh
      db1 = sum_n dh: N additions             Dh + N            on sum_n Mh
      dW1 = sum_n dh pooled: N fused adds     Dh + N + 1        on sum_n Mh |pooled|
      dpool = W1^T dh: Cr fused adds          Dh + Cr + 1       on |W1|^T Mh
      db2 = sum_n dv2                         3 + N             on sum_n A
      dW2 = sum_n dv2 s                       3 + 9 + N         on sum_n A |hp|."""
    dh = int(1.1 * ((int(c) + 63) // 64 + 9) + 21 + 1.1) + 1
    return {"dh": dh, "db1": dh + n, "dw1": dh + n + 1, "dpool": dh + cr + 1, "db2": 3 + n, "dw2": 12 + n}


# ---- the depthwise 5x5 -----------------------------------------------------------------------------------------------------------
class _DwConv5x5(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, stride):
        x = x.contiguous()
        ctx.wdt = w.dtype
        # an fp32 master weight next to a 16-bit tensor: cast here, outside autograd, as dwconv._DwConv3x3 does -- the fp32 weight
        # gradient then reaches the parameter as it is
        w = w.detach().to(x.dtype).contiguous()
        n, c, h, wd = (int(v) for v in x.shape)
        ho, wo = (h - 1) // stride + 1, (wd - 1) // stride + 1
        y = torch.empty((n, c, ho, wo), device=x.device, dtype=x.dtype)
        with torch.cuda.device(x.device):
            N.check(N.lib.ssdk_dwconv5_fwd(x.data_ptr(), w.data_ptr(), y.data_ptr(), n, c, h, wd, stride, N.dtype_code(x),
                                           N.stream_ptr(x.device)), "dwconv5_fwd")
        ctx.save_for_backward(x, w)
        ctx.stride = stride
        return y

    @staticmethod
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        stride, dev = ctx.stride, x.device
        gy = K.grad_in(gy, x.dtype)
        n, c, h, wd = (int(v) for v in x.shape)
        gx = gw = None
        with torch.cuda.device(dev):
            if ctx.needs_input_grad[0]:
                gx = torch.empty_like(x)
                N.check(N.lib.ssdk_dwconv5_bwd_data(gy.data_ptr(), w.data_ptr(), gx.data_ptr(), n, c, h, wd, stride, N.dtype_code(x),
                                                    N.stream_ptr(dev)), "dwconv5_bwd_data")
            if ctx.needs_input_grad[1]:
                need = int(N.lib.ssdk_dwconv5_bwd_weight_workspace_bytes(n, c, h, wd, stride))
                ws, wp = K.workspace(dev, need)
                gw32 = torch.empty((c, 1, 5, 5), device=dev, dtype=torch.float32)
                N.check(N.lib.ssdk_dwconv5_bwd_weight(x.data_ptr(), gy.data_ptr(), gw32.data_ptr(), wp, need, n, c, h, wd,
                                                      stride, N.dtype_code(x), N.stream_ptr(dev)), "dwconv5_bwd_weight")
                gw = K.weight_grad_out(gw32, ctx.wdt)
        return gx, gw, None


def dwconv5x5(x, weight, stride):
    """Depthwise 5x5, pad 2, stride 1 | 2, no bias: x [N, C, H, W] bf16 / fp16 on a HIP device, weight [C, 1, 5, 5] (fp32 master or
    the tensor dtype), differentiable in both (the weight gradient is accumulated in fp32 and returned in the weight's dtype)."""
    N.require_device(x, "dwconv5x5")
    N.require_device(weight, "dwconv5x5")
    if x.dim() != 4 or tuple(weight.shape) != (int(x.shape[1]), 1, 5, 5) or stride not in (1, 2):
        raise N.SsdkError("dwconv5x5: x [N, C, H, W], weight [C, 1, 5, 5], stride 1 | 2 expected, got {}, {}, {}".format(
            tuple(x.shape), tuple(weight.shape), stride))
    if x.dtype not in K.HALF or weight.dtype not in (torch.float32, x.dtype):
        raise N.SsdkError("dwconv5x5: a 16-bit x and an fp32 / same-dtype weight expected, got {} and {}".format(x.dtype, weight.dtype))
    with torch.autocast("cuda", enabled=False):
        return _DwConv5x5.apply(x, weight, int(stride))


# ---- SiLU + squeeze-excite -------------------------------------------------------------------------------------------------------
class _SiluSqueezeExcite(torch.autograd.Function):
    """u [N, C, H, W] 16 bit; w1 [Cr, C, 1, 1], b1 [Cr], w2 [C, Cr, 1, 1], b2 [C] fp32 -> z = silu(u) g.  Saved for backward: u, gate,
    pooled, hidden_pre (and the two weights)."""

    @staticmethod
    def forward(ctx, u, w1, b1, w2, b2):
        u = u.contiguous()
        n, c, h, w = (int(v) for v in u.shape)
        cr, dev = int(w1.shape[0]), u.device
        w1c, b1c, w2c, b2c = (t.detach().contiguous() for t in (w1, b1, w2, b2))
        pooled = torch.empty((n, c), device=dev, dtype=torch.float32)
        hidden = torch.empty((n, cr), device=dev, dtype=torch.float32)
        gate = torch.empty((n, c), device=dev, dtype=torch.float32)
        z = torch.empty_like(u)
        code, sp = N.dtype_code(u), N.stream_ptr(dev)
        with torch.cuda.device(dev):
            N.check(N.lib.ssdk_se_pool_fwd(u.data_ptr(), pooled.data_ptr(), n, c, h, w, code, sp), "se_pool_fwd")
            N.check(N.lib.ssdk_se_gate_fwd(pooled.data_ptr(), w1c.data_ptr(), b1c.data_ptr(), w2c.data_ptr(), b2c.data_ptr(),
                                           hidden.data_ptr(), gate.data_ptr(), n, c, cr, sp), "se_gate_fwd")
            N.check(N.lib.ssdk_se_scale_fwd(u.data_ptr(), gate.data_ptr(), z.data_ptr(), n, c, h, w, code, sp), "se_scale_fwd")
        ctx.save_for_backward(u, gate, pooled, hidden, w1c, w2c)
        ctx.shapes = (tuple(w1.shape), tuple(w2.shape))
        return z

    @staticmethod
    def backward(ctx, gz):
        u, gate, pooled, hidden, w1, w2 = ctx.saved_tensors
        n, c, h, w = (int(v) for v in u.shape)
        cr, dev = int(w1.shape[0]), u.device
        gz = gz.contiguous()
        if gz.dtype != u.dtype:
            gz = gz.to(u.dtype)
        f32 = dict(device=dev, dtype=torch.float32)
        draw, dpool = torch.empty((n, c), **f32), torch.empty((n, c), **f32)
        dw1, db1, dw2, db2 = torch.empty((cr, c), **f32), torch.empty((cr,), **f32), torch.empty((c, cr), **f32), torch.empty((c,), **f32)
        du = torch.empty_like(u)
        need = int(N.lib.ssdk_se_gate_bwd_workspace_bytes(n, c, cr))
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        code, sp = N.dtype_code(u), N.stream_ptr(dev)
        with torch.cuda.device(dev):
            N.check(N.lib.ssdk_se_bwd_reduce(u.data_ptr(), gz.data_ptr(), draw.data_ptr(), n, c, h, w, code, sp), "se_bwd_reduce")
            N.check(N.lib.ssdk_se_gate_bwd(draw.data_ptr(), gate.data_ptr(), pooled.data_ptr(), hidden.data_ptr(), w1.data_ptr(),
                                           w2.data_ptr(), dpool.data_ptr(), dw1.data_ptr(), db1.data_ptr(), dw2.data_ptr(),
                                           db2.data_ptr(), ws.data_ptr(), need, n, c, cr, sp), "se_gate_bwd")
            N.check(N.lib.ssdk_se_bwd_apply(u.data_ptr(), gz.data_ptr(), gate.data_ptr(), dpool.data_ptr(), du.data_ptr(), n, c, h, w,
                                            code, sp), "se_bwd_apply")
        s1, s2 = ctx.shapes
        return du, dw1.view(s1), db1, dw2.view(s2), db2


def silu_squeeze_excite(u, w1, b1, w2, b2):
    """z = silu(u) * sigmoid(W2 silu(W1 mean_hw(silu(u)) + b1) + b2): u [N, C, H, W] bf16 / fp16 on a HIP device, the parameters of
    the two squeeze-excite convolutions in fp32 ([Cr, C, 1, 1] / [Cr] / [C, Cr, 1, 1] / [C]; [Cr, C] / [C, Cr] are taken too).
    Differentiable in all five; the parameter gradients are fp32 in the parameters' shapes."""
    for t in (u, w1, b1, w2, b2):
        N.require_device(t, "silu_squeeze_excite")
    c = int(u.shape[1]) if u.dim() == 4 else -1
    cr = int(w1.shape[0])
    if (u.dim() != 4 or w1.numel() != cr * c or w2.numel() != cr * c or int(w2.shape[0]) != c or tuple(b1.shape) != (cr,)
            or tuple(b2.shape) != (c,) or c > MAX_C or cr > MAX_R):
        raise N.SsdkError("silu_squeeze_excite: u [N, C, H, W], w1 [Cr, C(, 1, 1)], b1 [Cr], w2 [C, Cr(, 1, 1)], b2 [C] with C <= {}, "
                          "Cr <= {} expected, got {}, {}, {}, {}, {}".format(MAX_C, MAX_R, tuple(u.shape), tuple(w1.shape),
                                                                             tuple(b1.shape), tuple(w2.shape), tuple(b2.shape)))
    if u.dtype not in K.HALF or any(t.dtype != torch.float32 for t in (w1, b1, w2, b2)):
        raise N.SsdkError("silu_squeeze_excite: a 16-bit u and fp32 parameters expected")
    with torch.autocast("cuda", enabled=False):
        return _SiluSqueezeExcite.apply(u, w1, b1, w2, b2)


# ---- the block -------------------------------------------------------------------------------------------------------------------
def supported(block):
    """An ``MBConvBlock`` whose depthwise convolution is k x k in {3, 5}, stride 1 | 2, bias-free, and whose squeeze-excite widths fit
    the gate kernels' LDS (every block of EfficientNet-B0 ... B5: hidden width <= 3072, Cr <= 128)."""
    if not isinstance(block, MBConvBlock):
        return False
    _, dw, se, proj, _ = block.parts()
    conv = dw[0]
    fc1, fc2 = se.se[1], se.se[3]
    c = conv.in_channels
    return (conv.kernel_size in ((3, 3), (5, 5)) and conv.stride in ((1, 1), (2, 2)) and conv.groups == c == conv.out_channels
            and conv.padding == (conv.kernel_size[0] // 2,) * 2 and conv.dilation == (1, 1) and conv.bias is None
            and conv.padding_mode == "zeros" and fc1.in_channels == c == fc2.out_channels and fc1.kernel_size == (1, 1)
            and fc2.kernel_size == (1, 1) and fc1.bias is not None and fc2.bias is not None and c <= MAX_C
            and fc1.out_channels <= MAX_R and proj.in_channels == c)


class TrainMBConvBlock(MBConvBlock):
    """``MBConvBlock`` whose training forward on 16-bit HIP tensors (or under autocast to them) runs the 5x5 depthwise convolution
    and SiLU + squeeze-excite on csrc/ssdk_mbconvtrain.hip; everything else (eval, CPU, fp32) is ``MBConvBlock.forward``."""

    def _dtype(self, x):
        if not (self.training and torch.is_tensor(x) and x.is_cuda and x.dim() == 4):
            return None
        dt = torch.get_autocast_dtype("cuda") if torch.is_autocast_enabled() else x.dtype
        if dt not in K.HALF:
            return None
        _, dw, se, _, _ = self.parts()
        if any(p.dtype != torch.float32 for p in (se.se[1].weight, se.se[1].bias, se.se[3].weight, se.se[3].bias)):
            return None
        return dt

    def forward(self, x):
        dt = self._dtype(x)
        if dt is None:
            STATS["fallback"] += 1
            return super(TrainMBConvBlock, self).forward(x)
        STATS["native_forward"] += 1
        expand, dw, se, proj, bn = self.parts()
        h = x if expand is None else expand(x)
        conv, dw_bn = dw[0], dw[1]
        if conv.kernel_size == (5, 5):
            if h.dtype != dt:
                h = h.to(dt)
            y = dwconv5x5(h, conv.weight, conv.stride[0])
        else:
            y = conv(h)  # the DepthwiseConv2d module as it is: its BatchNorm-statistics hand-off survives
        u = dw_bn(y)
        if u.dtype != dt:
            u = u.to(dt)
        z = silu_squeeze_excite(u, se.se[1].weight, se.se[1].bias, se.se[3].weight, se.se[3].bias)
        out = bn(proj(z))
        if self.use_residual:
            return x + self._drop_connect(out)
        return out


def use_native_mbconv(model):
    """Switch every supported ``MBConvBlock`` of ``model`` to ``TrainMBConvBlock`` (in place: same modules, parameters and
    ``state_dict`` keys).  -> blocks switched."""
    n = 0
    for m in model.modules():
        if type(m) is MBConvBlock and supported(m):
            m.__class__ = TrainMBConvBlock
            n += 1
    STATS["swapped"] += n
    return n


# what an unset SSDK_MBCONV_TRAIN means (train_routing.PASSES; docs/SWITCHES.md): "0" leaves the MBConv blocks on
# ``MBConvBlock.forward`` (the library's 5x5 depthwise kernels and the eager SiLU / pool / 1x1 / multiply passes)
DEFAULT = "1"
