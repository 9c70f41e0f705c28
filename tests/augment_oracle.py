"""fp64 numpy oracle of the training input pipeline (``ssdk_augment``, ssds/dataset/augment.py): the semantics of
DESIGN.md "Data input" restated independently of the kernel, for tests/test_augment_cpu.py and tests/test_gpu_augment.py.
A helper next to tests/nethelp.py, not a test module.

Per output pixel (ox, oy) of an image described by one descriptor:
  resize   source coordinate ((2 ox + 1) CW - W) / (2 W) on the canvas (rows alike), an exact rational: integer part q and
           remainder from integer arithmetic, weight remainder / (2 W); a negative coordinate is column 0 with weight 0; the
           taps are columns min(q, CW - 1) and min(q + 1, CW - 1)  (bilinear, half-pixel centres, edge-clamped)
  paste    canvas (cx, cy) -> crop (cx - paste_x, cy - paste_y); outside [0, crop_w) x [0, crop_h) the tap is ``fill``
  flip     crop column px -> crop_w - 1 - px
  crop     source pixel (crop_x + px, crop_y + py)
  colour   clamp(color . (r, g, b, 1), 0, 255) per source pixel, not rounded
  out      (bilinear - mean[c]) / std[c]
"""
import numpy as np


def _axis(n_out, n_canvas):
    """taps i0, i1 [n_out] and the weight of i1 (fp64 of the exact rational)"""
    o = np.arange(n_out, dtype=np.int64)
    num = (2 * o + 1) * int(n_canvas) - int(n_out)
    den = 2 * int(n_out)
    q = np.where(num < 0, 0, num // den)
    f = np.where(num < 0, 0, num - q * den).astype(np.float64) / den
    return np.minimum(q, n_canvas - 1), np.minimum(q + 1, n_canvas - 1), f


def render(pixels, desc, H, W, mean, std):
    """One image: ``pixels`` the whole packed uint8 buffer, ``desc`` one record (any mapping with the descriptor's field
    names) -> [3, H, W] float64."""
    g = lambda k: int(desc[k])  # noqa: E731
    sh, sw = g("src_h"), g("src_w")
    img = np.asarray(pixels)[g("src_offset"):g("src_offset") + sh * sw * 3].reshape(sh, sw, 3).astype(np.float64)
    color = np.asarray(desc["color"], np.float64).reshape(3, 4)
    fill = np.asarray(desc["fill"], np.float64).reshape(3)
    x0, x1, fx = _axis(W, g("canvas_w"))
    y0, y1, fy = _axis(H, g("canvas_h"))

    def taps(cy, cx):  # canvas rows [H], columns [W] -> [H, W, 3]
        py, px = cy - g("paste_y"), cx - g("paste_x")
        iy, ix = (py >= 0) & (py < g("crop_h")), (px >= 0) & (px < g("crop_w"))
        sx = g("crop_x") + (g("crop_w") - 1 - px if g("flip") else px)
        sy = g("crop_y") + py
        inside = iy[:, None] & ix[None, :]
        src = img[np.clip(sy, 0, sh - 1)[:, None], np.clip(sx, 0, sw - 1)[None, :]]  # [H, W, 3]
        v = np.clip(src @ color[:, :3].T + color[:, 3], 0.0, 255.0)
        return np.where(inside[:, :, None], v, fill[None, None, :])

    t00, t01, t10, t11 = taps(y0, x0), taps(y0, x1), taps(y1, x0), taps(y1, x1)
    fx_, fy_ = fx[None, :, None], fy[:, None, None]
    top = t00 + (t01 - t00) * fx_
    bot = t10 + (t11 - t10) * fx_
    o = top + (bot - top) * fy_
    o = (o - np.asarray(mean, np.float64).reshape(3)) / np.asarray(std, np.float64).reshape(3)
    return np.ascontiguousarray(o.transpose(2, 0, 1))


def render_batch(pixels, descs, H, W, mean, std):
    return np.stack([render(pixels, d, H, W, mean, std) for d in descs])


NTSC = np.array([[0.299, 0.587, 0.114], [0.596, -0.274, -0.322], [0.211, -0.523, 0.312]], np.float64)


def color_steps(rgb, hue_deg, sat, bri, con):
    """The colour twist one step at a time in fp64, on [..., 3] pixels: RGB -> YIQ, rotate the chroma plane by ``hue_deg``
    and scale it by ``sat``, back to RGB with the inverse matrix, then ``bri * (128 + con * (v - 128))``.  Not clamped."""
    yiq = np.asarray(rgb, np.float64) @ NTSC.T
    a = np.deg2rad(hue_deg)
    i = (np.cos(a) * yiq[..., 1] - np.sin(a) * yiq[..., 2]) * sat
    q = (np.sin(a) * yiq[..., 1] + np.cos(a) * yiq[..., 2]) * sat
    v = np.stack([yiq[..., 0], i, q], -1) @ np.linalg.inv(NTSC).T
    return bri * (128.0 + con * (v - 128.0))


def targets_to_source(targets, desc, H, W):
    """Inverse geometry of the kept boxes: target rows (x, y, w, h, label) in IMAGE_SIZE pixels -> (l, t, r, b, label) in
    source pixels, through resize, paste, flip and the crop's shift (clipping by the crop is not undone)."""
    t = np.asarray(targets, np.float64)
    t = t[t[:, 4] >= 0]
    sx, sy = int(desc["canvas_w"]) / float(W), int(desc["canvas_h"]) / float(H)
    l, r = t[:, 0] * sx - int(desc["paste_x"]), (t[:, 0] + t[:, 2]) * sx - int(desc["paste_x"])
    tp, b = t[:, 1] * sy - int(desc["paste_y"]), (t[:, 1] + t[:, 3]) * sy - int(desc["paste_y"])
    if int(desc["flip"]):
        l, r = int(desc["crop_w"]) - r, int(desc["crop_w"]) - l
    return np.stack([l + int(desc["crop_x"]), tp + int(desc["crop_y"]), r + int(desc["crop_x"]), b + int(desc["crop_y"]), t[:, 4]], 1)


def iou_with_rect(box, x, y, w, h):
    l, t, r, b = (float(v) for v in box[:4])
    iw, ih = max(min(r, x + w) - max(l, x), 0.0), max(min(b, y + h) - max(t, y), 0.0)
    inter = iw * ih
    return inter / ((r - l) * (b - t) + w * h - inter)


def round_to(a, name):
    """fp64 -> the value rounded to ``name`` (float32 | bfloat16 | float16), as float64, plus one ulp of that type at it."""
    import torch

    dt = getattr(torch, name)
    r = torch.from_numpy(np.asarray(a, np.float64)).to(torch.float32).to(dt)
    bits = {"float32": 23, "bfloat16": 7, "float16": 10}[name]
    tiny = {"float32": -126, "bfloat16": -126, "float16": -14}[name]
    v = r.to(torch.float64).numpy()
    e = np.floor(np.log2(np.maximum(np.abs(v), 2.0 ** tiny)))
    return v, 2.0 ** (e - bits)
