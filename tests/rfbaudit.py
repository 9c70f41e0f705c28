"""Per-op audit of a recorded plan that holds RFB blocks (tests/test_gpu_rfb.py): tests/planaudit.py's ``PlanAudit`` with

* ``_ref_conv`` for a 'dilated' pack -- ``F.conv2d(..., padding = dilation = pack.dilation)`` in fp32 on the op's actual input, then
  scale, bias and the activation; every other convolution is the base class's (which computes with dilation 1);
* references for the op kinds the detectors around the blocks bring with them: ``cat`` (the concatenation is data movement: the
  comparison is exact) and ``convt`` (the Shelf decoder's transposed convolution, its weight read back out of the parity images).
"""
import torch
import torch.nn.functional as F

import planaudit
from ssds import _native as N
from ssds.modeling.layers import fused_conv as FC


def dilated_reference(x, pk, act=None, dilation=None, transpose=False):
    """fp32 on the 16-bit input ``x`` [n, c, h, w] and the pack's 16-bit weights: conv2d with padding = dilation, * scale + bias,
    activation.  ``dilation`` / ``transpose``: the WRONG layer of the negative controls (another dilation; ky and kx swapped)."""
    d = pk.dilation if dilation is None else dilation
    wt = pk.w.float().permute(0, 3, 1, 2).contiguous()  # KRSC -> [co][ci][ky][kx]
    if transpose:
        wt = wt.transpose(2, 3).contiguous()
    tf32 = torch.backends.cudnn.allow_tf32
    torch.backends.cudnn.allow_tf32 = False
    try:
        y = F.conv2d(x.float(), wt, None, 1, d, d)
    finally:
        torch.backends.cudnn.allow_tf32 = tf32
    if pk.scale is not None:
        y = y * pk.scale.view(1, -1, 1, 1)
    y = y + pk.bias.view(1, -1, 1, 1)
    return planaudit.act_fn(y, pk.act if act is None else act)


def convt_weight(pk):
    """ConvTPack -> the ConvTranspose2d weight [Cin][Cout][3][3] in fp32 (fused_conv.convt_parity_images, inverted)."""
    cin, cout = pk.cin, pk.cout
    g = (cout + 15) // 16
    w = torch.zeros(cin, cout, 3, 3, dtype=torch.float32, device=pk.w.device)
    off = 0
    for py in (0, 1):
        for px in (0, 1):
            taps = FC.convt_class_taps(py, px)
            ks = (len(taps) * cin + 31) // 32
            img = pk.w[off:off + g * ks * 512].view(g, ks, 4, 16, 8)
            off += g * ks * 512
            mat = img.permute(0, 3, 1, 2, 4).reshape(g * 16, ks * 32).float()
            for t, (_, _, ky, kx) in enumerate(taps):
                w[:, :, ky, kx] = mat[:cout, t * cin:(t + 1) * cin].t()
    assert off == pk.w.numel()
    return w


class RfbAudit(planaudit.PlanAudit):
    def _ref_conv(self, i, L):
        pk = L["pack"]
        if pk.kind != "dilated":
            return planaudit.PlanAudit._ref_conv(self, i, L)
        assert L["res"] is None and not L["nchw"] and not L.get("res_mode", 0)
        xin = self.take(L["x"], L["n"], pk.cin, L["h"], L["w"])

        def run():
            want = dilated_reference(xin, pk, act=L["act"])
            return self.view(L["y"], L["n"], pk.cout, L["h"], L["w"])[self.sel], want

        return run

    def _ref_cat(self, i, L):
        a = self.take(L["x"], L["n"], L["c1"], L["h"], L["w"])
        hb, wb = (L["h"] // 2, L["w"] // 2) if L["up2"] else (L["h"], L["w"])
        b = self.take(L["b"], L["n"], L["c2"], hb, wb)

        def run():
            want = torch.cat([a, F.interpolate(b, scale_factor=2, mode="nearest") if L["up2"] else b], 1)
            return self.view(L["y"], L["n"], L["c1"] + L["c2"], L["h"], L["w"])[self.sel], want

        return run

    def _ref_convt(self, i, L):
        pk = L["pack"]
        ho, wo = 2 * L["h"] - 1, 2 * L["w"] - 1
        xin = self.take(L["x"], L["n"], pk.cin, L["h"], L["w"])
        skip = self.take(L["res"], L["n"], pk.cout, ho, wo) if L["res"] is not None else None

        def run():
            want = F.conv_transpose2d(xin, convt_weight(pk), pk.bias, stride=2, padding=1)
            if skip is not None:
                want = want + skip
            return self.view(L["y"], L["n"], pk.cout, ho, wo)[self.sel], want

        return run

    def run(self):
        """Launches the ops one by one -> planaudit's rows (index, name, kernel, kind, median, p999, max, zeros)."""
        plan, rows = self.plan, []
        table = plan.layer_table()
        refs = {None: self._ref_conv, "xpair": self._ref_xpair, "cat": self._ref_cat, "convt": self._ref_convt,
                "stem7": self._ref_stem7, "pool": self._ref_pool}
        tf32 = torch.backends.cudnn.allow_tf32
        torch.backends.cudnn.allow_tf32 = False
        try:
            for i, L in enumerate(plan.layers):
                kind = L.get("kind")
                with torch.no_grad():
                    ref = refs[kind](i, L)  # copies the op's inputs BEFORE the launch (the arena may recycle them later)
                    plan.launch(i, i + 1)
                    torch.cuda.synchronize()
                    kern = N.last_kernel()
                    got, want = ref()
                    med, p999, mx, zeros = planaudit.stats(got, want)
                rows.append(dict(index=i, name=table[i]["name"], kernel=kern.replace("_kernel", ""),
                                 kind="fused" if kind == "xpair" else "default", median=med, p999=p999, max=mx, zeros=zeros,
                                 dilated=kind is None and L["pack"].kind == "dilated"))
        finally:
            torch.backends.cudnn.allow_tf32 = tf32
        return rows
