"""The decoder step of the Shelf neck in the training step, on the NCHW tensors themselves (csrc/ssdk_convttrain.hip,
include/ssdk_convttrain.h): ``ConvTranspose2d(Cin, Cout, 3, stride=2, padding=1, bias)(x) + skip`` -- forward, input gradient,
weight and bias gradient.

PyTorch-ROCm runs the step as a library transposed convolution behind autocast's weight cast, an eager add over the largest maps
of the neck, and the library's two gradients plus a bias reduction.  ``ShelfConvT`` is an ``nn.ConvTranspose2d`` (same parameters,
``state_dict`` keys and initialisation) whose 16-bit HIP-device forward / backward run on the ssdk kernels:

    prepare          ssdk_convt_train_prepare   fp32 master weight -> the 16-bit forward and input-gradient images
    forward          ssdk_convt_train_forward   y  = convT(x, W) + bias + skip   (by output parity class; added in fp32, one rounding)
    input gradient   ssdk_convt_train_dgrad     gx = conv_s2(gy, W)
    weight gradient  ssdk_convt_train_wgrad     gW and gb in fp32 from one pass over gy, pixel ranges added in index order
    skip gradient    gy itself: no kernel, no copy

The layer is the adjoint of the dense 3x3 / stride 2 / pad 1 convolution Cout -> Cin on the (2H-1) x (2W-1) map whose OIHW weight
is ``weight`` as it lies in memory, so the images are that convolution's (denseconv.pack_dense_frag*), with the roles swapped.

kernel 3, stride 2, padding 1, no output padding, groups 1, Cin and Cout multiples of 16 in 16 .. 4096.  CPU tensors, fp32 tensors,
non-contiguous tensors and every other layer shape take ``nn.ConvTranspose2d.forward`` followed by the add.

The images are packed again by every call (one small launch): the native optimizers update parameters through raw pointers, so no
tensor version counter says when a cached image is stale."""
import torch
import torch.nn as nn

from ssds import _native as N
from ssds.modeling.layers import kernel_conv as K
from ssds.modeling.layers import denseconv

MIN_C, MAX_C = 16, 4096  # csrc/ssdk_convttrain.hip ct_check
STATS = {"swapped": 0, "native_forward": 0, "native_dgrad": 0, "native_wgrad": 0}


def shape_supported(cin, cout):
    """The channel counts csrc/ssdk_convttrain.hip takes."""
    return all(c % 16 == 0 and MIN_C <= c <= MAX_C for c in (cin, cout))


def supported(m):
    """``m`` is a transposed 3x3 / stride 2 / padding 1 convolution without output padding, of a supported shape."""
    return (isinstance(m, nn.ConvTranspose2d) and m.kernel_size == (3, 3) and m.stride == (2, 2) and m.padding == (1, 1)
            and m.output_padding == (0, 0) and m.dilation == (1, 1) and m.groups == 1 and m.padding_mode == "zeros"
            and shape_supported(m.in_channels, m.out_channels))


# ---- the images and the walks of the kernels over them, as torch expressions (layout and algebra: any device, any dtype) ----
def pack_forward_image(w):
    """The image the forward reads, of ``w`` [Cin, Cout, 3, 3]: [Cout / 16][KS][4][16][8], rows = output channels,
    k = tap * Cin + input channel, taps flipped -- the input-gradient image of the convolution whose OIHW weight is ``w``."""
    return denseconv.pack_dense_frag_dgrad(w)


def pack_dgrad_image(w):
    """The image the input gradient reads: [Cin / 16][KS][4][16][8], rows = input channels, k = tap * Cout + output channel --
    that convolution's forward image."""
    return denseconv.pack_dense_frag(w)


def forward_class_taps(py, px):
    """The (dy, dx, image tap) the forward kernel walks for the output pixels (2a + py, 2b + px): it reads x[a + dy][b + dx]
    against tap ``image tap`` of the forward image; (1 + py)(1 + px) of them, 9 per 2 x 2 output pixels."""
    taps = []
    for t in range((1 + py) * (1 + px)):
        tyk, txk = ((t >> 1), (t & 1)) if px else (t, 0)
        taps.append((tyk, txk, 3 * (2 * tyk if py else 1) + (2 * txk if px else 1)))
    return taps


def forward_from_image(x, image, cout):
    """convT(x, w) evaluated the way the forward kernel does, from ``image = pack_forward_image(w)``: per output parity class one
    product over the (H - py) x (W - px) pixels that have the neighbours it reads, every tap in range, nothing masked."""
    n, cin, h, w = (int(v) for v in x.shape)
    wt = denseconv.unpack_dense_frag(image, cout, cin)  # [Cout, Cin, 3, 3], taps as the image numbers them
    y = x.new_zeros((n, cout, 2 * h - 1, 2 * w - 1))
    for py in (0, 1):
        for px in (0, 1):
            hh, ww = h - py, w - px
            if hh == 0 or ww == 0:
                continue
            acc = 0
            for dy, dx, tap in forward_class_taps(py, px):
                acc = acc + torch.einsum("oc,nchw->nohw", wt[:, :, tap // 3, tap % 3], x[:, :, dy:dy + hh, dx:dx + ww])
            y[:, :, py::2, px::2] = acc
    return y


def dgrad_from_image(gy, image, cin):
    """The input gradient the way its kernel computes it, from ``image = pack_dgrad_image(w)``: the 3x3 / stride 2 / pad 1
    convolution of gy, tap (ky, kx) reading gy[2a + ky - 1][2b + kx - 1]."""
    cout = int(gy.shape[1])
    wt = denseconv.unpack_dense_frag(image, cin, cout)  # [Cin, Cout, 3, 3]
    return torch.nn.functional.conv2d(gy, wt, None, 2, 1)


def prepare_images(weight, dtype, want_dgrad=True):
    """fp32 (or 16-bit) weight [Cin, Cout, 3, 3] on a HIP device -> (forward image, input-gradient image | None) in ``dtype``, one
    launch."""
    cin, cout = int(weight.shape[0]), int(weight.shape[1])
    dev = weight.device
    w32 = weight.detach().float().contiguous()  # (a 16-bit weight survives the round trip exactly)
    rb, ks, _ = denseconv.image_shape(cout, cin)
    fwd = torch.empty((rb, ks, 4, 16, 8), device=dev, dtype=dtype)
    dg = None
    if want_dgrad:
        rb, ks, _ = denseconv.image_shape(cin, cout)
        dg = torch.empty((rb, ks, 4, 16, 8), device=dev, dtype=dtype)
    with torch.cuda.device(dev):
        N.check(N.lib.ssdk_convt_train_prepare(w32.data_ptr(), fwd.data_ptr(), None if dg is None else dg.data_ptr(), cin, cout,
                                               N.dtype_code(fwd), N.stream_ptr(dev)), "convt_train_prepare")
    return fwd, dg


class _ConvT3x3S2(torch.autograd.Function):
    """x [N, Cin, H, W] 16 bit, contiguous; weight [Cin, Cout, 3, 3] fp32 (the master parameter under autocast: the weight
    gradient comes back in fp32) or in x's dtype; bias [Cout] or None; skip [N, Cout, 2H-1, 2W-1] in x's dtype, contiguous, or None.
    The gradient of the skip is the output gradient itself."""

    @staticmethod
    def forward(ctx, x, weight, bias, skip):
        n, cin, h, wd = (int(v) for v in x.shape)
        cout = int(weight.shape[1])
        dev, dt = x.device, x.dtype
        code = N.dtype_code(x)
        x = x.detach()
        fwd, dg = prepare_images(weight, dt, want_dgrad=ctx.needs_input_grad[0])
        b32 = None if bias is None else bias.detach().float().contiguous()
        sk = None if skip is None else skip.detach()
        y = torch.empty((n, cout, 2 * h - 1, 2 * wd - 1), device=dev, dtype=dt)
        with torch.cuda.device(dev):
            N.check(N.lib.ssdk_convt_train_forward(x.data_ptr(), fwd.data_ptr(), None if b32 is None else b32.data_ptr(),
                                                   None if sk is None else sk.data_ptr(), y.data_ptr(), n, cin, cout, h, wd, code,
                                                   N.stream_ptr(dev)), "convt_train_forward")
        STATS["native_forward"] += 1
        ctx.save_for_backward(x, dg)
        ctx.meta = (weight.dtype, None if bias is None else bias.dtype, cout)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, dg = ctx.saved_tensors
        wdt, bdt, cout = ctx.meta
        n, cin, h, wd = (int(v) for v in x.shape)
        dev, dt = x.device, x.dtype
        gy = K.grad_in(gy, dt)
        code = N.dtype_code(x)
        gx = gw = gb = None
        want_gb = bdt is not None and ctx.needs_input_grad[2]
        with torch.cuda.device(dev):
            sp = N.stream_ptr(dev)
            if ctx.needs_input_grad[0]:
                gx = torch.empty_like(x)
                N.check(N.lib.ssdk_convt_train_dgrad(gy.data_ptr(), dg.data_ptr(), gx.data_ptr(), n, cin, cout, h, wd, code, sp),
                        "convt_train_dgrad")
                STATS["native_dgrad"] += 1
            if ctx.needs_input_grad[1] or want_gb:
                need = int(N.lib.ssdk_convt_train_wgrad_workspace_bytes(n, cin, cout, h, wd))
                ws, wp = K.workspace(dev, need)
                gw32 = torch.empty((cin, cout, 3, 3), device=dev, dtype=torch.float32)
                gb32 = torch.empty((cout,), device=dev, dtype=torch.float32) if want_gb else None
                N.check(N.lib.ssdk_convt_train_wgrad(x.data_ptr(), gy.data_ptr(), gw32.data_ptr(), None if gb32 is None else gb32.data_ptr(),
                                                     wp, need, n, cin, cout, h, wd, code, sp), "convt_train_wgrad")
                STATS["native_wgrad"] += 1
                if ctx.needs_input_grad[1]:
                    gw = K.weight_grad_out(gw32, wdt)
                if want_gb:
                    gb = K.weight_grad_out(gb32, bdt)
        return gx, gw, gb, (gy if ctx.needs_input_grad[3] else None)


def _describe(t):
    return "{} {} on {}".format(tuple(t.shape) if torch.is_tensor(t) else type(t), getattr(t, "dtype", None), getattr(t, "device", None))


def _kernel_tensor(t):
    return torch.is_tensor(t) and t.is_cuda and t.dim() == 4 and t.dtype in K.HALF and t.is_contiguous()


def _skip_fits(x, skip, cout):
    n, _, h, w = (int(v) for v in x.shape)
    return tuple(skip.shape) == (n, cout, 2 * h - 1, 2 * w - 1) and skip.dtype == x.dtype and skip.device == x.device


def convt3x3s2(x, weight, bias=None, skip=None):
    """The native path, called explicitly: ``F.conv_transpose2d(x, weight, bias, 2, 1) + skip`` on csrc/ssdk_convttrain.hip,
    differentiable in all four.  x (and skip) 16-bit contiguous NCHW on a HIP device, weight [Cin, Cout, 3, 3] fp32 or x's dtype;
    anything else raises."""
    for name, t in (("x", x), ("skip", skip)):
        if t is not None and not _kernel_tensor(t):
            raise ValueError("convt3x3s2: {} must be a 16-bit contiguous NCHW tensor on a HIP device, got {}".format(name, _describe(t)))
    if (not torch.is_tensor(weight) or weight.dim() != 4 or tuple(weight.shape[2:]) != (3, 3) or int(weight.shape[0]) != int(x.shape[1])
            or not shape_supported(int(weight.shape[0]), int(weight.shape[1])) or weight.device != x.device
            or weight.dtype not in (torch.float32, x.dtype)):
        raise ValueError("convt3x3s2: weight [Cin, Cout, 3, 3] with Cin, Cout multiples of 16 in 16..4096, fp32 or x's dtype, on x's "
                         "device, got " + _describe(weight))
    if bias is not None and (tuple(bias.shape) != (int(weight.shape[1]),) or bias.device != x.device):
        raise ValueError("convt3x3s2: bias must be [Cout] on x's device, got " + _describe(bias))
    if skip is not None and not _skip_fits(x, skip, int(weight.shape[1])):
        raise ValueError("convt3x3s2: skip {} does not fit x {}".format(_describe(skip), _describe(x)))
    if x.numel() == 0:
        raise ValueError("convt3x3s2: empty input")
    return _ConvT3x3S2.apply(x, weight, bias, skip)


class ShelfConvT(nn.ConvTranspose2d):
    """``nn.ConvTranspose2d(Cin, Cout, 3, stride 2, padding 1)`` whose 16-bit HIP-device forward / backward run on
    csrc/ssdk_convttrain.hip (same parameters, ``state_dict`` keys and initialisation), with the skip map of the Shelf decoder
    step added by the forward kernel; everything else is ``nn.ConvTranspose2d.forward`` followed by the add."""

    takes_skip = True  # ShelfPyramid.forward hands the level's map to the step instead of adding it

    def _module_path(self, x, output_size, skip):
        y = super(ShelfConvT, self).forward(x, output_size)
        return y if skip is None else y + skip

    def forward(self, x, output_size=None, skip=None):
        if (output_size is not None or not (torch.is_tensor(x) and x.is_cuda and x.dim() == 4 and x.is_contiguous())
                or int(x.shape[1]) != self.in_channels or x.numel() == 0 or not supported(self)):
            return self._module_path(x, output_size, skip)
        w = self.weight
        xk, sk = x, skip
        if torch.is_autocast_enabled():
            xk = x.to(torch.get_autocast_dtype("cuda"))
            if sk is not None and torch.is_tensor(sk):
                sk = sk.to(xk.dtype)
        if xk.dtype not in K.HALF or (w.dtype != torch.float32 and w.dtype != xk.dtype) or w.device != xk.device:
            return self._module_path(x, output_size, skip)
        if sk is not None and not (_kernel_tensor(sk) and _skip_fits(xk, sk, self.out_channels)):
            return self._module_path(x, output_size, skip)
        with torch.autocast("cuda", enabled=False):
            return _ConvT3x3S2.apply(xk, w, self.bias, sk)


# docs/SWITCHES.md, DESIGN.md 4.5i: the step A/B at batch 32, bf16 (profiles/r16_train_step_shelf_ab.jsonl) has the kernels SLOWER than
# the module path on shelf_resnet18_513 -- 50.34 against 47.36 ms per step with the switch off, 48.00 ms on the parent commit, spreads
# under 0.1 ms -- so the routing is off unless SSDK_CONVT_TRAIN=1.  The weight-gradient pass is what loses (about 780 us against 130 us
# per layer): its 32-pixel steps are half empty on the 17- and 33-wide maps
DEFAULT = "0"  # (train_routing.PASSES reads it; 0 leaves the layers on nn.ConvTranspose2d and the eager add)


def use_native_convt(model):
    """Switch every ``nn.ConvTranspose2d`` of ``model`` that ``supported`` accepts to the kernel-backed subclass (in place; no new
    parameters, same ``state_dict``).  -> model; STATS["swapped"] counts the layers."""
    for m in model.modules():
        if type(m) is nn.ConvTranspose2d and supported(m):
            m.__class__ = ShelfConvT
            STATS["swapped"] += 1
    return model
