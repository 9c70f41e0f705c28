"""What the kernel-backed ``nn.Conv2d`` layers of the training step share: the one ``forward`` that decides between the HIP kernels
and ``nn.Conv2d.forward`` (``KernelConv2d``), the one class swap (``swap_layers``), the small steps every backward pass of the
ssdk kernels repeats (``workspace``, ``grad_in``, ``weight_grad_out``, ``bias_grad``) and the autograd function of the 3x3
families that read prepared weight images (``ImageConv3x3``: groupedconv.py, denseconv.py).

A new kernel-backed ``nn.Conv2d`` declares, on its class: ``matches(m)``, what it does with a strided input (``copies_strided``),
which weight dtypes its kernels take (``half_weight``) and ``_run(x, w)``; its ``use_*`` function is ``swap_layers(model, cls)``.
DESIGN.md section 6 has the table of what the existing classes declare."""
import collections

import torch
import torch.nn as nn

from ssds import _native as N

HALF = (torch.bfloat16, torch.float16)


def workspace(device, nbytes):
    """-> (the tensor to keep alive until the launch is queued, a 16-byte-aligned pointer to ``nbytes`` bytes of it)."""
    ws = torch.empty(nbytes + 16, dtype=torch.uint8, device=device)
    return ws, (ws.data_ptr() + 15) & ~15


def grad_in(gy, dtype):
    """The output gradient as the kernels read it: contiguous, in the dtype of the saved activation."""
    gy = gy.contiguous()
    return gy if gy.dtype == dtype else gy.to(dtype)


def weight_grad_out(gw32, wdt):
    """The kernels' fp32 weight gradient in the parameter's dtype (the fp32 master weight under autocast: as it is)."""
    return gw32 if wdt == torch.float32 else gw32.to(wdt)


def bias_grad(gy, bdt):
    """The bias gradient where torch computes it: the sum of ``gy`` over batch and pixels in fp32, in the bias's dtype."""
    return gy.sum((0, 2, 3), dtype=torch.float32).to(bdt)


class KernelConv2d(nn.Conv2d):
    """An ``nn.Conv2d`` (same parameters, ``state_dict`` keys and initialisation) whose 16-bit HIP-device forward / backward run
    on ssdk kernels; everything else is ``nn.Conv2d.forward``.  The kernels get a 4-D HIP tensor in bf16 / fp16 -- under autocast
    the input cast to the autocast dtype -- and the parameter itself, with autocast switched off around them."""

    copies_strided = False  # a non-contiguous x: True -- the kernels get a contiguous copy; False -- nn.Conv2d.forward
    half_weight = False  # the weight: False -- fp32 only (the master parameter); True -- fp32, or 16 bit in x's dtype
    checks_width = True  # x.shape[1] must be in_channels (False: the kernels' own shape errors speak)

    @staticmethod
    def matches(m):
        """The layer predicate: the ``nn.Conv2d`` configurations the kernels take.  The gate of ``forward`` and the swap
        (``swap_layers``) both ask it, and nothing else about the module."""
        raise NotImplementedError

    def runs(self):
        """A second, narrower condition asked at run time only (a switch read per call); the swap does not look at it."""
        return True

    def fallback(self, x):
        return super(KernelConv2d, self).forward(x)

    def _run(self, x, w):
        raise NotImplementedError

    def forward(self, x):
        if not (x.is_cuda and x.dim() == 4 and (self.copies_strided or x.is_contiguous())
                and (not self.checks_width or int(x.shape[1]) == self.in_channels) and self.matches(self) and self.runs()):
            return self.fallback(x)
        w = self.weight
        if torch.is_autocast_enabled():
            x = x.to(torch.get_autocast_dtype("cuda"))
        if x.dtype not in HALF or (w.dtype != torch.float32 and not (self.half_weight and w.dtype == x.dtype)):
            return self.fallback(x)
        with torch.autocast("cuda", enabled=False):
            return self._run(x.contiguous() if self.copies_strided else x, w)


def swap_layers(model, cls, also=None):
    """Switch every plain ``nn.Conv2d`` of ``model`` (no subclass: those belong to somebody) that ``cls.matches`` -- and ``also``,
    if given -- accepts to ``cls``, in place: no new parameters, same ``state_dict``.  -> layers switched."""
    n = 0
    for m in model.modules():
        if type(m) is nn.Conv2d and cls.matches(m) and (also is None or also(m)):
            m.__class__ = cls
            n += 1
    return n


# ---- 3x3 / pad 1 / stride 1 | 2 on NCHW tensors with prepared weight images ------------------------------------------------------
# What differs between the families: ``name`` (the ``what`` of the error strings), the STATS dict, the entry points,
# ``prepare(weight, groups, dtype, want_dgrad) -> (forward image, input-gradient image | None)``, ``dims(n, cin, cout, h, w, groups,
# stride)`` -> the shape arguments as the entry points take them, and whether the forward kernel adds the bias (else torch does)
ImageFamily = collections.namedtuple("ImageFamily", "name stats prepare forward dgrad wgrad wgrad_workspace_bytes dims kernel_bias")


class ImageConv3x3(torch.autograd.Function):
    """x [N, Cin, H, W] 16 bit, contiguous; weight [Cout, Cin / groups, 3, 3] fp32 (the master parameter under autocast: the weight
    gradient comes back in fp32) or in x's dtype; bias or None (its gradient is a torch sum)."""

    @staticmethod
    def forward(ctx, x, weight, bias, stride, groups, fam):
        n, cin, h, wd = (int(v) for v in x.shape)
        cout = int(weight.shape[0])
        dev, dt = x.device, x.dtype
        ho, wo = (h - 1) // stride + 1, (wd - 1) // stride + 1
        code = N.dtype_code(x)
        x = x.detach()
        dims = fam.dims(n, cin, cout, h, wd, groups, stride)
        fwd, dg = fam.prepare(weight, groups, dt, ctx.needs_input_grad[0])
        y = torch.empty((n, cout, ho, wo), device=dev, dtype=dt)
        ptrs = (x.data_ptr(), fwd.data_ptr())
        if fam.kernel_bias:
            b32 = None if bias is None else bias.detach().float().contiguous()
            ptrs += (None if b32 is None else b32.data_ptr(),)
        with torch.cuda.device(dev):
            N.check(fam.forward(*(ptrs + (y.data_ptr(),) + dims + (code, N.stream_ptr(dev)))), fam.name + "_forward")
        fam.stats["native_forward"] += 1
        if bias is not None and not fam.kernel_bias:
            y += bias.detach().to(dt).view(1, cout, 1, 1)
        ctx.save_for_backward(x, dg)
        ctx.meta = (fam, dims, tuple(weight.shape), weight.dtype, None if bias is None else bias.dtype)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, dg = ctx.saved_tensors
        fam, dims, wshape, wdt, bdt = ctx.meta
        dev = x.device
        gy = grad_in(gy, x.dtype)
        tail = dims + (N.dtype_code(x),)
        gx = gw = gb = None
        with torch.cuda.device(dev):
            sp = N.stream_ptr(dev)
            if ctx.needs_input_grad[0]:
                gx = torch.empty_like(x)
                N.check(fam.dgrad(gy.data_ptr(), dg.data_ptr(), gx.data_ptr(), *tail, sp), fam.name + "_dgrad")
                fam.stats["native_dgrad"] += 1
            if ctx.needs_input_grad[1]:
                need = int(fam.wgrad_workspace_bytes(*dims))
                ws, wp = workspace(dev, need)
                gw32 = torch.empty(wshape, device=dev, dtype=torch.float32)
                N.check(fam.wgrad(x.data_ptr(), gy.data_ptr(), gw32.data_ptr(), wp, need, *tail, sp), fam.name + "_wgrad")
                fam.stats["native_wgrad"] += 1
                gw = weight_grad_out(gw32, wdt)
        if bdt is not None and ctx.needs_input_grad[2]:
            gb = bias_grad(gy, bdt)
        return gx, gw, gb, None, None, None
