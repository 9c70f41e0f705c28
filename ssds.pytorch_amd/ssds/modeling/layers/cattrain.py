"""The two YOLO-only operations of the YOLOv3 / YOLOv4 training step on the NCHW tensors themselves (csrc/ssdk_cattrain.hip), forward
and backward:

    cat2(a, b, mode)   y = a || R(b) along the channels         R = SAME | UP2 (nearest x2)
    spp(x)             y = x || maxpool5(x) || maxpool9(x) || maxpool13(x)   (SPPModule(3), max-pool)

PyTorch-ROCm runs the concatenation behind an upsample as ``interpolate`` (which writes the upsampled tensor) + ``cat`` and splits
the gradient in several launches; its SPP block is three ``max_pool2d`` calls that each keep an int64 index per element, then ``cat``.
Here each is one launch forward and one backward, the upsampled tensor is never written, and the SPP backward recomputes the arg-max of
every window from the saved input (first maximum in row-major window order under numeric comparison, torch's rule): ``spp`` saves
only ``x``.

``use_native_cat(model)`` enables the path per model; a model it was never called on runs the earlier expressions."""
import torch

from ssds import _native as N

SAME, UP2 = 0, 1  # include/ssdk.h SSDK_FUSE_*
MAX_SIDE = N.SPP_TRAIN_MAX_SIDE  # include/ssdk_cattrain.h: the largest H / W of an SPP plane
STATS = {"yolov3_models": 0, "pan_modules": 0, "spp_modules": 0, "cat_forward": 0, "cat_backward": 0, "spp_forward": 0, "spp_backward": 0}
_HALF = (torch.bfloat16, torch.float16)


def _kernel_tensor(t):
    return torch.is_tensor(t) and t.is_cuda and t.dim() == 4 and t.dtype in _HALF and t.is_contiguous()


def _cat_geometry(a, b, mode):
    """``b`` has the dims the kernels expect under ``mode`` next to ``a``."""
    n, _, h, w = (int(v) for v in a.shape)
    bn, _, bh, bw = (int(v) for v in b.shape)
    if bn != n:
        return False
    if mode == SAME:
        return (bh, bw) == (h, w)
    if mode == UP2:
        return h % 2 == 0 and w % 2 == 0 and (bh, bw) == (h // 2, w // 2)
    return False


def _describe(t):
    return "{} {} on {}".format(tuple(t.shape) if torch.is_tensor(t) else type(t), getattr(t, "dtype", None), getattr(t, "device", None))


class _Cat2(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b, mode):
        n, c1, h, w = (int(v) for v in a.shape)
        c2 = int(b.shape[1])
        dev = a.device
        a, b = a.detach(), b.detach()
        y = torch.empty((n, c1 + c2, h, w), device=dev, dtype=a.dtype)
        with torch.cuda.device(dev):
            N.check(N.lib.ssdk_cat_train_fwd(a.data_ptr(), b.data_ptr(), y.data_ptr(), n, c1, c2, h, w, mode, N.dtype_code(a),
                                             N.stream_ptr(dev)), "cat_train_fwd")
        STATS["cat_forward"] += 1
        ctx.meta = (tuple(a.shape), tuple(b.shape), mode, a.dtype)
        return y

    @staticmethod
    def backward(ctx, gy):
        sa, sb, mode, dt = ctx.meta
        n, c1, h, w = sa
        dev = gy.device
        gy = gy.contiguous()
        if gy.dtype != dt:
            gy = gy.to(dt)
        ga = torch.empty(sa, device=dev, dtype=dt) if ctx.needs_input_grad[0] else None
        gb = torch.empty(sb, device=dev, dtype=dt) if ctx.needs_input_grad[1] else None
        with torch.cuda.device(dev):
            N.check(N.lib.ssdk_cat_train_bwd(gy.data_ptr(), None if ga is None else ga.data_ptr(), None if gb is None else gb.data_ptr(),
                                             n, c1, sb[1], h, w, mode, N.dtype_code(gy), N.stream_ptr(dev)), "cat_train_bwd")
        STATS["cat_backward"] += 1
        return ga, gb, None


def cat2(a, b, mode=SAME):
    """torch.cat((a, R(b)), 1) with R = identity (SAME) or nearest x2 (UP2) on csrc/ssdk_cattrain.hip, differentiable in a and b.
    Explicit: 16-bit contiguous NCHW tensors of one dtype on one HIP device whose shapes fit the mode, anything else raises."""
    mode = int(mode)
    for t in (a, b):
        if not _kernel_tensor(t):
            raise ValueError("cat2: 16-bit contiguous NCHW tensors on a HIP device, got " + _describe(t))
    if a.dtype != b.dtype or a.device != b.device:
        raise ValueError("cat2: the sources differ in dtype or device")
    if not _cat_geometry(a, b, mode):
        raise ValueError("cat2: source shape {} does not fit {} under mode {}".format(tuple(b.shape), tuple(a.shape), mode))
    return _Cat2.apply(a, b, mode)


class _Spp(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        n, c, h, w = (int(v) for v in x.shape)
        dev = x.device
        x = x.detach()
        y = torch.empty((n, 4 * c, h, w), device=dev, dtype=x.dtype)
        with torch.cuda.device(dev):
            N.check(N.lib.ssdk_spp_train_fwd(x.data_ptr(), y.data_ptr(), n, c, h, w, N.dtype_code(x), N.stream_ptr(dev)), "spp_train_fwd")
        STATS["spp_forward"] += 1
        ctx.save_for_backward(x)  # nothing else: the arg-max of every window is recomputed
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
            N.check(N.lib.ssdk_spp_train_bwd(x.data_ptr(), gy.data_ptr(), gx.data_ptr(), n, c, h, w, N.dtype_code(x), N.stream_ptr(dev)),
                    "spp_train_bwd")
        STATS["spp_backward"] += 1
        return gx


def spp(x):
    """torch.cat([x] + [max_pool2d(x, k, 1, k // 2) for k in (5, 9, 13)], 1) on csrc/ssdk_cattrain.hip, differentiable.  Explicit: a
    16-bit contiguous NCHW tensor on a HIP device with H, W <= MAX_SIDE, anything else raises."""
    if not _kernel_tensor(x):
        raise ValueError("spp: a 16-bit contiguous NCHW tensor on a HIP device, got " + _describe(x))
    if int(x.shape[2]) > MAX_SIDE or int(x.shape[3]) > MAX_SIDE:
        raise ValueError("spp: a {}x{} plane is over the {} x {} the kernels stage".format(int(x.shape[2]), int(x.shape[3]), MAX_SIDE, MAX_SIDE))
    return _Spp.apply(x)


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
        if t.dtype not in _HALF or not t.is_contiguous() or (out and (t.dtype != out[0].dtype or t.device != out[0].device)):
            return None
        out.append(t)
    return out


def try_cat2(a, b, mode=SAME):
    """``cat2`` when the operands meet its contract (16-bit, contiguous, HIP device; under autocast after the cast to its dtype;
    shapes that fit the mode), else None: the caller runs its eager expression."""
    srcs = _kernel_inputs(a, b)
    if srcs is None or not _cat_geometry(srcs[0], srcs[1], int(mode)) or min(srcs[0].numel(), srcs[1].numel()) == 0:
        return None
    with torch.autocast("cuda", enabled=False):
        return _Cat2.apply(srcs[0], srcs[1], int(mode))


def try_spp(x):
    """``spp`` when ``x`` meets its contract (and its plane is within MAX_SIDE), else None."""
    srcs = _kernel_inputs(x)
    if srcs is None or int(x.shape[2]) > MAX_SIDE or int(x.shape[3]) > MAX_SIDE or srcs[0].numel() == 0:
        return None
    with torch.autocast("cuda", enabled=False):
        return _Spp.apply(srcs[0])


# what an unset SSDK_CAT_TRAIN means (train_routing.PASSES; docs/SWITCHES.md): 1 routes the channel concatenations and
# the SPP block of the YOLOV3 / YOLOV4 training step to csrc/ssdk_cattrain.hip, 0 leaves them on torch's cat / interpolate / max_pool2d
DEFAULT = "1"


def spp_supported(m):
    """``m`` is the SPP block the kernels compute: three max-pool levels (windows 5, 9, 13)."""
    from ssds.modeling.ssds.yolo import SPPModule

    return isinstance(m, SPPModule) and m.num_levels == 3 and m.pool_type == "max_pool"


def use_native_cat(model):
    """Enable the kernels on ``model`` in place (no new parameters, same ``state_dict``): every ``YOLOV3``, ``PANModule`` and
    max-pool ``SPPModule(3)`` gets the flag its forward reads.  -> model; STATS counts what was switched."""
    from ssds.modeling.ssds.yolo import YOLOV3, PANModule, SPPModule

    for m in model.modules():
        if getattr(m, "native_cat", False):
            continue
        if isinstance(m, YOLOV3):
            m.native_cat = True
            STATS["yolov3_models"] += 1
        elif isinstance(m, PANModule):
            m.native_cat = True
            STATS["pan_modules"] += 1
        elif isinstance(m, SPPModule) and spp_supported(m):
            m.native_cat = True
            STATS["spp_modules"] += 1
    return model
