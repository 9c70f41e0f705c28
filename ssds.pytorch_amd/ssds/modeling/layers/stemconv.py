"""The image-side stem convolutions inside the training step, forward and weight gradient on the 16-bit NCHW tensors autograd hands
over, with the fp32 master weight rounded inside the kernel (no per-step cast of the parameter, no layout transposes):

    StemConv7x7s2   ``nn.Conv2d(Cin <= 3, Cout <= 64, 7, 2, 3, bias=False)``, the ResNet / ResNeXt stem (nets/resnet.py conv1) on
                    csrc/ssdk_stem7train.hip.  DESIGN.md 4.5e
    StemConv3x3s2   ``nn.Conv2d(Cin <= 3, Cout <= 32, 3, 2, 1, bias=False)``, the first layer of the MobileNet backbones, on
                    csrc/ssdk_stemtrain.hip

The image has no gradient; if somebody asks for one it comes from the framework's convolution backward."""
import collections

import torch

from ssds import _native as N
from ssds.modeling.layers import kernel_conv as K

STATS = {"swapped": 0, "native_forward": 0, "native_wgrad": 0, "fallback": 0}  # (of the 7x7 stem)

# what differs between the two stems: ``name`` (entry points ssdk_<name>_fwd / _wgrad, the ``what`` of the error strings), kernel
# size and padding, the workspace of the weight gradient from (n, h, w, cout), the STATS dict or None, and ``library_wgrad(w)``:
# image widths whose weight gradient is left to the library
_Stem = collections.namedtuple("_Stem", "name k pad fwd wgrad wgrad_workspace_bytes stats library_wgrad")
# rows that are not whole 16-byte groups (the 300 px configuration): the kernel's element-wise operand path is slower than the
# library's weight gradient (tools/run/r06_s43.sh) -- only the forward is ours there
_STEM3 = _Stem("stem3x3s2", 3, 1, N.lib.ssdk_stem3x3s2_fwd, N.lib.ssdk_stem3x3s2_wgrad,
               lambda n, h, w, cout: N.lib.ssdk_stem3x3s2_wgrad_workspace_bytes(n, h), None, lambda w: w % 16 != 0)
_STEM7 = _Stem("stem7x7s2", 7, 3, N.lib.ssdk_stem7x7s2_fwd, N.lib.ssdk_stem7x7s2_wgrad, N.lib.ssdk_stem7x7s2_wgrad_workspace_bytes,
               STATS, lambda w: False)


class _StemConv(torch.autograd.Function):
    """x [N, Cin <= 3, H, W] 16 bit (contiguous), w [Cout, Cin, k, k] fp32 master parameter -> y [N, Cout, Ho, Wo] 16 bit, stride 2.
    Backward: the weight gradient (fp32, matrix cores over pixels, fixed-order partial sums); the image's gradient, if anybody
    asks for it, comes from the framework's convolution backward."""

    @staticmethod
    def forward(ctx, x, w, stem):
        n, cin, h, wd = (int(v) for v in x.shape)
        cout, dev = int(w.shape[0]), x.device
        ho, wo = (h - 1) // 2 + 1, (wd - 1) // 2 + 1
        x = x.detach()
        y = torch.empty((n, cout, ho, wo), device=dev, dtype=x.dtype)
        with torch.cuda.device(dev):
            N.check(stem.fwd(x.data_ptr(), w.detach().contiguous().data_ptr(), y.data_ptr(), n, cin, h, wd, cout, N.dtype_code(x),
                             N.stream_ptr(dev)), stem.name + "_fwd")
        if stem.stats is not None:
            stem.stats["native_forward"] += 1
        ctx.save_for_backward(x, w)
        ctx.stem = stem
        return y

    @staticmethod
    def _library_backward(gy, x, w, stem, mask):
        return torch.ops.aten.convolution_backward(gy, x, w.to(x.dtype), None, [2, 2], [stem.pad] * 2, [1, 1], False, [0, 0], 1, mask)

    @staticmethod
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        stem = ctx.stem
        n, cin, h, wd = (int(v) for v in x.shape)
        cout, dev = int(w.shape[0]), x.device
        gy = K.grad_in(gy, x.dtype)
        gx = gw = None
        if ctx.needs_input_grad[1] and stem.library_wgrad(wd):
            gw = _StemConv._library_backward(gy, x, w, stem, [False, True, False])[1].to(w.dtype)
        elif ctx.needs_input_grad[1]:
            need = int(stem.wgrad_workspace_bytes(n, h, wd, cout))
            ws, wp = K.workspace(dev, need)
            gw32 = torch.empty((cout, cin, stem.k, stem.k), device=dev, dtype=torch.float32)
            with torch.cuda.device(dev):
                N.check(stem.wgrad(x.data_ptr(), gy.data_ptr(), gw32.data_ptr(), wp, need, n, cin, h, wd, cout, N.dtype_code(x),
                                   N.stream_ptr(dev)), stem.name + "_wgrad")
            if stem.stats is not None:
                stem.stats["native_wgrad"] += 1
            gw = K.weight_grad_out(gw32, w.dtype)
        if ctx.needs_input_grad[0]:
            gx = _StemConv._library_backward(gy, x, w, stem, [True, False, False])[0]
        return gx, gw, None


def stem_conv7x7s2(x, w):
    """y = conv2d(x, round_to_dtype(w), stride 2, pad 3) on the HIP kernels: x [N, Cin <= 3, H, W] bf16 / fp16 on a HIP device,
    w [Cout <= 64, Cin, 7, 7] fp32.  Differentiable in w (fp32 gradient) and, through the framework, in x."""
    N.require_device(x, "stem_conv7x7s2")
    N.require_device(w, "stem_conv7x7s2")
    if x.dim() != 4 or w.dim() != 4 or tuple(w.shape[2:]) != (7, 7) or int(w.shape[1]) != int(x.shape[1]):
        raise N.SsdkError("stem_conv7x7s2: x [N, Cin, H, W] and w [Cout, Cin, 7, 7] expected, got {} and {}".format(
            tuple(x.shape), tuple(w.shape)))
    if x.dtype not in K.HALF or w.dtype != torch.float32:
        raise N.SsdkError("stem_conv7x7s2: a 16-bit x and an fp32 w expected, got {} and {}".format(x.dtype, w.dtype))
    return _StemConv.apply(x.contiguous(), w, _STEM7)


def _stem_geometry(m, k, pad, max_cout):
    return (m.kernel_size == (k, k) and m.padding == (pad, pad) and m.stride == (2, 2) and m.groups == 1 and m.dilation == (1, 1)
            and m.padding_mode == "zeros" and m.bias is None and m.in_channels <= 3 and m.out_channels <= max_cout)


class StemConv7x7s2(K.KernelConv2d):
    """``nn.Conv2d(Cin <= 3, Cout <= 64, k = 7, stride 2, pad 3, bias = False)`` -- the first layer of the ResNet / ResNeXt
    backbones -- whose 16-bit HIP-device forward / weight gradient run on ``csrc/ssdk_stem7train.hip`` (same parameter,
    ``state_dict`` key and initialisation); everything else is ``nn.Conv2d.forward``."""

    copies_strided = True

    @staticmethod
    def matches(m):
        return _stem_geometry(m, 7, 3, 64)

    def fallback(self, x):
        STATS["fallback"] += 1
        return super(StemConv7x7s2, self).fallback(x)

    def _run(self, x, w):
        return _StemConv.apply(x, w, _STEM7)


class StemConv3x3s2(K.KernelConv2d):
    """``nn.Conv2d(Cin <= 3, Cout <= 32, k = 3, stride 2, pad 1, bias = False)`` -- the first layer of the MobileNet backbones --
    whose 16-bit HIP-device forward / weight gradient run on ``csrc/ssdk_stemtrain.hip`` (same parameter, ``state_dict`` key and
    initialisation); everything else is ``nn.Conv2d.forward``."""

    # the path the class was first published under, where it stays importable: pickled models and tests/golden/route_digest.json
    # name a class by its module
    __module__ = "ssds.modeling.layers.pointwise"
    copies_strided = True

    @staticmethod
    def matches(m):
        return _stem_geometry(m, 3, 1, 32)

    def _run(self, x, w):
        return _StemConv.apply(x, w, _STEM3)


def use_native_stem7(model):
    """Switch the image-side 7x7 / stride-2 convolutions of ``model`` (<= 3 input channels, <= 64 filters, pad 3, no bias) to the
    kernel-backed subclass (in place).  -> layers switched."""
    n = K.swap_layers(model, StemConv7x7s2)
    STATS["swapped"] += n
    return n


def use_native_stem(model):
    """Switch the image-side 3x3 / stride-2 convolutions of ``model`` (<= 3 input channels, <= 32 filters, no bias) to the
    kernel-backed subclass (in place).  -> layers switched."""
    return K.swap_layers(model, StemConv3x3s2)


# what an unset SSDK_STEM7_TRAIN means (train_routing.PASSES; docs/SWITCHES.md): nothing measured yet, so the library
# routing stays the default.  "0" leaves the 7x7 stem on nn.Conv2d (the library convolution behind autocast's weight cast)
DEFAULT = "0"
