"""The ResNet / ResNeXt stem convolution inside the training step: ``nn.Conv2d(Cin <= 3, Cout <= 64, 7, 2, 3, bias=False)``
(nets/resnet.py conv1) on csrc/ssdk_stem7train.hip -- forward and weight gradient on the 16-bit NCHW tensors autograd hands over,
with the fp32 master weight rounded inside the kernel (no per-step cast of the parameter, no layout transposes).  The image has
no gradient; if somebody asks for one it comes from the framework's convolution backward.  DESIGN.md 4.5e."""
import torch
import torch.nn as nn

from ssds import _native as N

STATS = {"swapped": 0, "native_forward": 0, "native_wgrad": 0, "fallback": 0}


class _StemConv7x7s2(torch.autograd.Function):
    """x [N, Cin <= 3, H, W] 16 bit (contiguous), w [Cout <= 64, Cin, 7, 7] fp32 master parameter -> y [N, Cout, Ho, Wo] 16 bit.
    Backward: the weight gradient (fp32, matrix cores over pixels, fixed-order partial sums)."""

    @staticmethod
    def forward(ctx, x, w):
        n, cin, h, wd = (int(v) for v in x.shape)
        cout, dev = int(w.shape[0]), x.device
        ho, wo = (h - 1) // 2 + 1, (wd - 1) // 2 + 1
        x = x.detach()
        y = torch.empty((n, cout, ho, wo), device=dev, dtype=x.dtype)
        with torch.cuda.device(dev):
            N.check(N.lib.ssdk_stem7x7s2_fwd(x.data_ptr(), w.detach().contiguous().data_ptr(), y.data_ptr(), n, cin, h, wd, cout,
                                             N.dtype_code(x), N.stream_ptr(dev)), "stem7x7s2_fwd")
        STATS["native_forward"] += 1
        ctx.save_for_backward(x, w)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        n, cin, h, wd = (int(v) for v in x.shape)
        cout, dev = int(w.shape[0]), x.device
        gy = gy.contiguous()
        if gy.dtype != x.dtype:
            gy = gy.to(x.dtype)
        gx = gw = None
        if ctx.needs_input_grad[1]:
            need = int(N.lib.ssdk_stem7x7s2_wgrad_workspace_bytes(n, h, wd, cout))
            ws = torch.empty(need + 16, dtype=torch.uint8, device=dev)
            wp = (ws.data_ptr() + 15) & ~15
            gw = torch.empty((cout, cin, 7, 7), device=dev, dtype=torch.float32)
            with torch.cuda.device(dev):
                N.check(N.lib.ssdk_stem7x7s2_wgrad(x.data_ptr(), gy.data_ptr(), gw.data_ptr(), wp, need, n, cin, h, wd, cout,
                                                   N.dtype_code(x), N.stream_ptr(dev)), "stem7x7s2_wgrad")
            STATS["native_wgrad"] += 1
        if ctx.needs_input_grad[0]:
            gx = torch.ops.aten.convolution_backward(gy, x, w.to(x.dtype), None, [2, 2], [3, 3], [1, 1], False, [0, 0], 1,
                                                     [True, False, False])[0]
        return gx, gw


def stem_conv7x7s2(x, w):
    """y = conv2d(x, round_to_dtype(w), stride 2, pad 3) on the HIP kernels: x [N, Cin <= 3, H, W] bf16 / fp16 on a HIP device,
    w [Cout <= 64, Cin, 7, 7] fp32.  Differentiable in w (fp32 gradient) and, through the framework, in x."""
    N.require_device(x, "stem_conv7x7s2")
    N.require_device(w, "stem_conv7x7s2")
    if x.dim() != 4 or w.dim() != 4 or tuple(w.shape[2:]) != (7, 7) or int(w.shape[1]) != int(x.shape[1]):
        raise N.SsdkError("stem_conv7x7s2: x [N, Cin, H, W] and w [Cout, Cin, 7, 7] expected, got {} and {}".format(
            tuple(x.shape), tuple(w.shape)))
    if x.dtype not in (torch.bfloat16, torch.float16) or w.dtype != torch.float32:
        raise N.SsdkError("stem_conv7x7s2: a 16-bit x and an fp32 w expected, got {} and {}".format(x.dtype, w.dtype))
    return _StemConv7x7s2.apply(x.contiguous(), w)


class StemConv7x7s2(nn.Conv2d):
    """``nn.Conv2d(Cin <= 3, Cout <= 64, k = 7, stride 2, pad 3, bias = False)`` -- the first layer of the ResNet / ResNeXt
    backbones -- whose 16-bit HIP-device forward / weight gradient run on ``csrc/ssdk_stem7train.hip`` (same parameter,
    ``state_dict`` key and initialisation); everything else is ``nn.Conv2d.forward``."""

    def _native(self, x):
        return (x.is_cuda and x.dim() == 4 and self.kernel_size == (7, 7) and self.padding == (3, 3) and self.dilation == (1, 1)
                and self.stride == (2, 2) and self.groups == 1 and self.padding_mode == "zeros" and self.bias is None
                and self.in_channels <= 3 and self.out_channels <= 64 and int(x.shape[1]) == self.in_channels)

    def forward(self, x):
        if not self._native(x):
            STATS["fallback"] += 1
            return super(StemConv7x7s2, self).forward(x)
        w = self.weight
        if torch.is_autocast_enabled():
            x = x.to(torch.get_autocast_dtype("cuda"))
        if x.dtype not in (torch.bfloat16, torch.float16) or w.dtype != torch.float32:
            STATS["fallback"] += 1
            return super(StemConv7x7s2, self).forward(x)
        with torch.autocast("cuda", enabled=False):
            return _StemConv7x7s2.apply(x.contiguous(), w)


def _matches(m):
    return (type(m) is nn.Conv2d and m.kernel_size == (7, 7) and m.padding == (3, 3) and m.stride == (2, 2) and m.groups == 1
            and m.dilation == (1, 1) and m.padding_mode == "zeros" and m.bias is None and m.in_channels <= 3
            and m.out_channels <= 64)


def use_native_stem7(model):
    """Switch the image-side 7x7 / stride-2 convolutions of ``model`` (<= 3 input channels, <= 64 filters, pad 3, no bias) to the
    kernel-backed subclass (in place).  -> layers switched."""
    n = 0
    for m in model.modules():
        if _matches(m):
            m.__class__ = StemConv7x7s2
            n += 1
    STATS["swapped"] += n
    return n


# what an unset SSDK_STEM7_TRAIN means (train_routing.PASSES; docs/SWITCHES.md): nothing measured yet, so the library
# routing stays the default.  "0" leaves the 7x7 stem on nn.Conv2d (the library convolution behind autocast's weight cast)
DEFAULT = "0"
