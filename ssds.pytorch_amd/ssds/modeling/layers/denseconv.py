"""Dense 3x3 convolutions of the training step on the NCHW tensors themselves (csrc/ssdk_conv3train.hip): the towers, smoothing
and head convolutions of SSDFPN / SSDBiFPN, the 3x3 of the ResNet bottlenecks and the extras -- forward (+ bias), input gradient
and weight gradient.

PyTorch-ROCm sends a dense ``nn.Conv2d`` in bf16 to MIOpen's implicit GEMM, through autocast's cast of the weight and the
library's own layout transposes.  ``DenseConv3x3`` is an ``nn.Conv2d`` (same parameters, ``state_dict`` keys and
initialisation) whose 16-bit HIP-device forward / backward run on the ssdk kernels:

    prepare          ssdk_conv3x3_train_prepare   fp32 master weight -> the 16-bit forward and input-gradient images
    forward          ssdk_conv3x3_train_forward   y  = conv(x, W) + bias   (bias added in fp32, one rounding)
    input gradient   ssdk_conv3x3_train_dgrad     dx = conv^T(dy, W)   (stride 2: by input-pixel parity, no zero-dilated dy)
    weight gradient  ssdk_conv3x3_train_wgrad     dW fp32, pixel ranges added in index order: bit-reproducible

pad 1, stride 1 | 2, groups 1, Cin a multiple of 16 in 16 .. 4096, Cout a multiple of 4 in 4 .. 4096.  CPU tensors, fp32
tensors, non-contiguous tensors and every other layer shape take ``nn.Conv2d.forward``.

The images are packed again by every call (one small launch): the native optimizers update parameters through raw pointers,
so no tensor version counter says when a cached image is stale."""
import torch
import torch.nn as nn

from ssds import _native as N
from ssds.modeling.layers import kernel_conv as K

MIN_CIN, MAX_CIN, MIN_COUT, MAX_COUT = 16, 4096, 4, 4096  # csrc/ssdk_conv3train.hip c3_shape_ok
STATS = {"swapped": 0, "native_forward": 0, "native_dgrad": 0, "native_wgrad": 0}


def shape_supported(cin, cout):
    """The channel counts csrc/ssdk_conv3train.hip takes."""
    return cin % 16 == 0 and MIN_CIN <= cin <= MAX_CIN and cout % 4 == 0 and MIN_COUT <= cout <= MAX_COUT


def supported(m):
    """``m`` is a dense 3x3 / pad 1 / stride 1 | 2 convolution of a supported shape."""
    return (isinstance(m, nn.Conv2d) and m.kernel_size == (3, 3) and m.padding == (1, 1) and m.dilation == (1, 1)
            and m.stride in ((1, 1), (2, 2)) and m.padding_mode == "zeros" and m.groups == 1
            and shape_supported(m.in_channels, m.out_channels))


def image_shape(rows, channels):
    """-> (RB, KS, Cp) of the dense 3x3 image (include/ssdk.h) of a weight [rows, channels, 3, 3]."""
    cp = (channels + 15) // 16 * 16
    return (rows + 15) // 16, (9 * cp + 31) // 32, cp


def pack_dense_frag(w):
    """The dense 3x3 image of include/ssdk.h of OIHW weights ``w`` [R, C, 3, 3]: the matrix [16 ceil(R / 16)][Kpad] with
    k = tap * Cp + c (Cp = C padded to 16, zeros in the padding), in fragment-major order [RB][KS][4][16][8].  Pure layout, on the
    tensor's own device (CPU tensors too)."""
    r, c, kh, kw = (int(v) for v in w.shape)
    assert kh == 3 and kw == 3, tuple(w.shape)
    rb, ks, cp = image_shape(r, c)
    mat = w.new_zeros((rb * 16, ks * 32))
    mat[:r, :9 * cp].view(r, 9, cp)[:, :, :c] = w.permute(0, 2, 3, 1).reshape(r, 9, c)
    return mat.view(rb, 16, ks, 4, 8).permute(0, 2, 3, 1, 4).contiguous()


def pack_dense_frag_dgrad(w):
    """The image of the INPUT-GRADIENT weights W'[ci][co][ky][kx] = W[co][ci][2 - ky][2 - kx]: at stride 1 dx = conv(dy, W'),
    pad 1."""
    return pack_dense_frag(w.flip(2, 3).transpose(0, 1))


def unpack_dense_frag(img, rows, channels):
    """The layout read backwards: image [RB][KS][4][16][8] -> OIHW weights [rows, channels, 3, 3]."""
    rb, ks, cp = image_shape(rows, channels)
    assert tuple(img.shape) == (rb, ks, 4, 16, 8), tuple(img.shape)
    mat = img.permute(0, 3, 1, 2, 4).reshape(rb * 16, ks * 32)
    return mat[:rows, :9 * cp].reshape(rows, 3, 3, cp)[:, :, :, :channels].permute(0, 3, 1, 2).contiguous()


def prepare_images(weight, dtype, want_dgrad=True):
    """fp32 (or 16-bit) weight [Cout, Cin, 3, 3] on a HIP device -> (forward image, input-gradient image | None) in ``dtype``, one
    launch."""
    cout, cin = int(weight.shape[0]), int(weight.shape[1])
    dev = weight.device
    w32 = weight.detach().float().contiguous()  # (a 16-bit weight survives the round trip exactly)
    rb, ks, _ = image_shape(cout, cin)
    fwd = torch.empty((rb, ks, 4, 16, 8), device=dev, dtype=dtype)
    dg = None
    if want_dgrad:
        rb, ks, _ = image_shape(cin, cout)
        dg = torch.empty((rb, ks, 4, 16, 8), device=dev, dtype=dtype)
    with torch.cuda.device(dev):
        N.check(N.lib.ssdk_conv3x3_train_prepare(w32.data_ptr(), fwd.data_ptr(), None if dg is None else dg.data_ptr(), cin, cout,
                                                 N.dtype_code(fwd), N.stream_ptr(dev)), "conv3x3_train_prepare")
    return fwd, dg


# (bias added in fp32 by the forward kernel; its gradient is a torch sum)
FAMILY = K.ImageFamily(name="conv3x3_train", stats=STATS, kernel_bias=True,
                       prepare=lambda weight, groups, dtype, want_dgrad: prepare_images(weight, dtype, want_dgrad),
                       dims=lambda n, cin, cout, h, w, groups, stride: (n, cin, cout, h, w, stride),
                       forward=N.lib.ssdk_conv3x3_train_forward, dgrad=N.lib.ssdk_conv3x3_train_dgrad,
                       wgrad=N.lib.ssdk_conv3x3_train_wgrad, wgrad_workspace_bytes=N.lib.ssdk_conv3x3_train_wgrad_workspace_bytes)


def dense_conv3x3(x, weight, bias=None, stride=1):
    """The native path, called explicitly: x 16-bit contiguous NCHW on a HIP device; differentiable."""
    return K.ImageConv3x3.apply(x, weight, bias, stride, 1, FAMILY)


class DenseConv3x3(K.KernelConv2d):
    """``nn.Conv2d(Cin, Cout, 3, stride 1 | 2, pad 1)`` whose 16-bit HIP-device forward / backward run on
    csrc/ssdk_conv3train.hip (same parameters, ``state_dict`` keys and initialisation); everything else is ``nn.Conv2d.forward``."""

    matches = staticmethod(supported)
    half_weight = True

    def _run(self, x, w):
        return K.ImageConv3x3.apply(x, w, self.bias, self.stride[0], 1, FAMILY)


# what an unset SSDK_DENSE3_TRAIN means on SSDFPN / SSDBiFPN models (train_routing.PASSES picks between this and YOLO_DEFAULT by the
# model): 1 routes the dense 3x3 layers of the training step to csrc/ssdk_conv3train.hip, 0 leaves them on nn.Conv2d (extras: the im2col
# path).  Provisional (docs/SWITCHES.md): to be re-decided from the per-layer probe and the step A/B
DEFAULT = "1"


# YOLOV3 / YOLOV4 models (docs/SWITCHES.md): every 3x3 of both shipped configs fits the kernels, and the step A/B at
# batch 32 (profiles/r15_train_step_yolo_ab.jsonl) has them SLOWER than nn.Conv2d on these ResNet-18 models -- 14.44 vs 11.43 ms
# (yolov3_resnet18_320), 28.45 vs 22.02 ms (yolov4_resnet18_512) -- so on YOLO models the routing is off unless SSDK_DENSE3_TRAIN=1
YOLO_DEFAULT = "0"  # (SSDShelf models too: never timed there, slower on the other ResNet-18 models)


def use_native_dense3x3(model):
    """Switch every dense 3x3 ``nn.Conv2d`` of ``model`` that ``supported`` accepts to the kernel-backed subclass (in place; no
    new parameters, same ``state_dict``).  -> model; STATS["swapped"] counts the layers."""
    STATS["swapped"] += K.swap_layers(model, DenseConv3x3)
    return model
