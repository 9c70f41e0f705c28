// ssdk_augment.hip -- the training input pipeline as one pass on gfx950 (HBM-bound).
//
// Reference: the DALI graph of ssds/dataset/dali_dataiterator.py:72-103 (SSD random crop, HSV twist, brightness /
// contrast, horizontal flip, paste onto a mean-filled canvas, resize, normalise).  The host draws every random number
// (ssds/dataset/augment.py) and hands the kernel one descriptor per image; the kernel walks each OUTPUT pixel back
// through resize -> canvas -> paste -> flip -> crop to four source taps of the packed uint8 HWC RGB buffer:
//     tap inside the pasted crop : clamp(color . (r, g, b, 1), 0, 255)     (hue, saturation, brightness and contrast
//     tap outside it             : fill                                     folded into ONE 3x4 matrix on the host)
//     out = (bilinear(t00, t01, t10, t11; fx, fy) - mean[c]) / std[c]  -> dtype, NCHW
// Bilinear, half-pixel centres, edge-clamped, no antialiasing.  The source coordinate of output column x is the rational
// ((2x+1) CW - W) / (2W): integer part and remainder in INTEGER arithmetic, weight = remainder / (2W) in fp32, so the
// taps are exact and the weights good to one rounding (DESIGN.md "Data input").  fp32 operation order (no contraction:
// the Makefile's -ffp-contract=off), which tests/augment_oracle.py restates in fp64:
//     v   = ((m0*r + m1*g) + m2*b) + m3;  v = min(max(v, 0), 255)
//     top = t00 + (t01 - t00) * fx;  bot = t10 + (t11 - t10) * fx;  o = top + (bot - top) * fy;  y = (o - mean) / std
// A lane owns 8 consecutive output pixels of one row and produces all three channel planes from the same taps (the
// source is interleaved RGB); 16-byte stores per plane for the 16-bit types, as preprocess_kernel does.  blockIdx.y is
// the image, so the descriptor is wave-uniform.  Algorithmic bytes: every touched source byte of the crop once + the
// output once; the 4 taps of neighbouring pixels overlap and are served by L1 / L2.
//
// Every descriptor is checked on the HOST before anything is launched (a bad one is SSDK_E_BADARG, no launch), and the
// kernel clamps its tap coordinates to the image as well: no descriptor can make it read outside `pixels`.
#include <cmath>

#include "ssdk_conv_common.h"

namespace ssdk {

struct AugParams {
  const unsigned char* pixels;
  const ssdk_augment_desc* descs;  // device copy (workspace)
  void* y;
  int H, W, wg, dst_dtype;  // wg = ceil(W / 8)
  float mean[3], std[3];
};

__global__ __launch_bounds__(256) void augment_kernel(const AugParams p) {
  const int t = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (t >= p.H * p.wg) return;
  const int n = (int)blockIdx.y;
  const ssdk_augment_desc& d = p.descs[n];
  const int oy = t / p.wg;
  const int x0 = (t - oy * p.wg) * 8;
  const unsigned char* img = p.pixels + d.src_offset;
  const int src_w = d.src_w, src_h = d.src_h, crop_w = d.crop_w, crop_h = d.crop_h;

  // rows: canvas rows cy0 | cy1 of the two taps and the weight of the second
  int cy0, cy1;
  float fy;
  {
    const int num = (2 * oy + 1) * d.canvas_h - p.H, den = 2 * p.H;
    const int q = num < 0 ? 0 : num / den;
    fy = num < 0 ? 0.f : (float)(num - q * den) / (float)den;
    cy0 = min(q, d.canvas_h - 1);
    cy1 = min(q + 1, d.canvas_h - 1);
  }
  const int py0 = cy0 - d.paste_y, py1 = cy1 - d.paste_y;  // rows of the crop (outside [0, crop_h): fill)
  const bool in_y0 = py0 >= 0 && py0 < crop_h, in_y1 = py1 >= 0 && py1 < crop_h;
  const size_t row0 = (size_t)min(max(d.crop_y + py0, 0), src_h - 1) * (size_t)src_w;
  const size_t row1 = (size_t)min(max(d.crop_y + py1, 0), src_h - 1) * (size_t)src_w;

  float m[12], fill[3];
#pragma unroll
  for (int i = 0; i < 12; ++i) m[i] = d.color[i];
#pragma unroll
  for (int c = 0; c < 3; ++c) fill[c] = d.fill[c];

  // one tap: canvas column cx of crop row `in_y` / source row offset `row` -> 3 channels
  auto tap = [&](int cx, bool in_y, size_t row, float* v) {
    const int px = cx - d.paste_x;
    if (!in_y || px < 0 || px >= crop_w) {
      v[0] = fill[0];
      v[1] = fill[1];
      v[2] = fill[2];
      return;
    }
    const int sx = min(max(d.crop_x + (d.flip ? crop_w - 1 - px : px), 0), src_w - 1);
    const unsigned char* s = img + (row + (size_t)sx) * 3;
    const float r = (float)s[0], g = (float)s[1], b = (float)s[2];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float a = ((m[c * 4] * r + m[c * 4 + 1] * g) + m[c * 4 + 2] * b) + m[c * 4 + 3];
      v[c] = fminf(fmaxf(a, 0.f), 255.f);
    }
  };

  float out[3][8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int ox = x0 + e;
    out[0][e] = out[1][e] = out[2][e] = 0.f;
    if (ox >= p.W) continue;
    const int num = (2 * ox + 1) * d.canvas_w - p.W, den = 2 * p.W;
    const int q = num < 0 ? 0 : num / den;
    const float fx = num < 0 ? 0.f : (float)(num - q * den) / (float)den;
    const int cx0 = min(q, d.canvas_w - 1), cx1 = min(q + 1, d.canvas_w - 1);
    float t00[3], t01[3], t10[3], t11[3];
    tap(cx0, in_y0, row0, t00);
    tap(cx1, in_y0, row0, t01);
    tap(cx0, in_y1, row1, t10);
    tap(cx1, in_y1, row1, t11);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float top = t00[c] + (t01[c] - t00[c]) * fx;
      const float bot = t10[c] + (t11[c] - t10[c]) * fx;
      const float o = top + (bot - top) * fy;
      out[c][e] = (o - p.mean[c]) / p.std[c];  // ssdk_preprocess's order: subtract, divide
    }
  }

#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const size_t o = (((size_t)n * 3 + c) * p.H + oy) * p.W + x0;
    if (p.dst_dtype == SSDK_F32) {
      float* dst = (float*)p.y + o;
      for (int e = 0; e < 8 && x0 + e < p.W; ++e) dst[e] = out[c][e];
      continue;
    }
    u16* dst = (u16*)p.y + o;
    u32 h[8];
#pragma unroll
    for (int e = 0; e < 8; ++e)
      h[e] = p.dst_dtype == SSDK_BF16 ? f32_to_bits16<SSDK_BF16>(out[c][e]) : f32_to_bits16<SSDK_F16>(out[c][e]);
    if (x0 + 8 <= p.W && (((uintptr_t)dst) & 15u) == 0) {
      *reinterpret_cast<u32x4*>(dst) = u32x4{h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16)};
    } else {
      for (int e = 0; e < 8 && x0 + e < p.W; ++e) dst[e] = (u16)h[e];
    }
  }
}

constexpr int kAugMaxSide = 16384;    // H, W: (2 * 16383 + 1) * 32768 < 2^31 keeps the kernel's coordinates in int
constexpr int kAugMaxCanvas = 32768;  // canvas_w, canvas_h
constexpr int kAugMaxBatch = 65535;   // gridDim.y

}  // namespace ssdk

using namespace ssdk;

extern "C" size_t ssdk_augment_desc_bytes(void) { return sizeof(ssdk_augment_desc); }

extern "C" size_t ssdk_augment_workspace_bytes(int B) {
  if (B < 1 || B > kAugMaxBatch) return 0;
  return ((size_t)B * sizeof(ssdk_augment_desc) + 255) / 256 * 256;
}

extern "C" int ssdk_augment(const void* pixels, size_t pixels_bytes, const ssdk_augment_desc* descs_host, int B, int H,
                            int W, const float* mean, const float* std, void* y, int dst_dtype, void* workspace,
                            size_t workspace_bytes, void* stream) {
  if (!pixels || !descs_host || !mean || !std || !y || !workspace) {
    set_error("augment: null pointer (pixels %p descs_host %p mean %p std %p y %p workspace %p)", pixels,
              (const void*)descs_host, (const void*)mean, (const void*)std, y, workspace);
    return SSDK_E_BADARG;
  }
  if (B < 1 || B > kAugMaxBatch) {
    set_error("augment: B = %d outside [1, %d]", B, kAugMaxBatch);
    return SSDK_E_BADARG;
  }
  if (H < 1 || H > kAugMaxSide || W < 1 || W > kAugMaxSide) {
    set_error("augment: H = %d, W = %d outside [1, %d]", H, W, kAugMaxSide);
    return SSDK_E_BADARG;
  }
  if (dst_dtype != SSDK_F32 && dst_dtype != SSDK_BF16 && dst_dtype != SSDK_F16) {
    set_error("augment: dst_dtype %d is not SSDK_F32 | SSDK_BF16 | SSDK_F16", dst_dtype);
    return SSDK_E_BADARG;
  }
  if (workspace_bytes < ssdk_augment_workspace_bytes(B)) {
    set_error("augment: workspace_bytes %zu < ssdk_augment_workspace_bytes(%d) = %zu", workspace_bytes, B,
              ssdk_augment_workspace_bytes(B));
    return SSDK_E_BADARG;
  }
  for (int c = 0; c < 3; ++c) {
    if (!std::isfinite(mean[c]) || !std::isfinite(std[c]) || std[c] == 0.f) {
      set_error("augment: mean[%d] = %g / std[%d] = %g must be finite and std non-zero", c, mean[c], c, std[c]);
      return SSDK_E_BADARG;
    }
  }
  for (int i = 0; i < B; ++i) {
    const ssdk_augment_desc& d = descs_host[i];
    const char* bad = nullptr;
    if (d.src_h < 1 || d.src_w < 1) bad = "src_h / src_w < 1";
    else if (d.src_offset < 0 || (uint64_t)d.src_offset > pixels_bytes ||
             (uint64_t)d.src_h * (uint64_t)d.src_w * 3u > pixels_bytes - (uint64_t)d.src_offset)
      bad = "src_offset + src_h * src_w * 3 runs past pixels_bytes";
    else if (d.crop_w < 1 || d.crop_h < 1) bad = "crop_w / crop_h < 1";
    else if (d.crop_x < 0 || d.crop_y < 0 || (int64_t)d.crop_x + d.crop_w > d.src_w || (int64_t)d.crop_y + d.crop_h > d.src_h)
      bad = "crop_x / crop_y / crop_w / crop_h outside the image";
    else if (d.canvas_w < 1 || d.canvas_h < 1 || d.canvas_w > kAugMaxCanvas || d.canvas_h > kAugMaxCanvas)
      bad = "canvas_w / canvas_h outside [1, 32768]";
    else if (d.paste_x < 0 || d.paste_y < 0 || (int64_t)d.paste_x + d.crop_w > d.canvas_w || (int64_t)d.paste_y + d.crop_h > d.canvas_h)
      bad = "paste_x / paste_y: the pasted crop lies outside the canvas";
    else if (d.flip != 0 && d.flip != 1) bad = "flip is not 0 | 1";
    else {
      for (int k = 0; k < 12 && !bad; ++k)
        if (!std::isfinite(d.color[k])) bad = "color is not finite";
      for (int k = 0; k < 3 && !bad; ++k)
        if (!std::isfinite(d.fill[k])) bad = "fill is not finite";
    }
    if (bad) {
      set_error("augment: descriptor %d: %s (src_offset %lld src %dx%d crop %d,%d %dx%d canvas %dx%d paste %d,%d flip %d; "
                "pixels_bytes %zu)", i, bad, (long long)d.src_offset, d.src_w, d.src_h, d.crop_x, d.crop_y, d.crop_w, d.crop_h,
                d.canvas_w, d.canvas_h, d.paste_x, d.paste_y, d.flip, pixels_bytes);
      return SSDK_E_BADARG;
    }
  }
  hipStream_t s = (hipStream_t)stream;
  // one copy of the checked descriptors, ordered before the kernel on the caller's stream
  if (hipMemcpyAsync(workspace, descs_host, (size_t)B * sizeof(ssdk_augment_desc), hipMemcpyHostToDevice, s) != hipSuccess) {
    (void)hipGetLastError();
    set_error("augment: hipMemcpyAsync of %d descriptors to the workspace failed", B);
    return SSDK_E_LAUNCH;
  }
  AugParams p;
  p.pixels = (const unsigned char*)pixels;
  p.descs = (const ssdk_augment_desc*)workspace;
  p.y = y;
  p.H = H;
  p.W = W;
  p.wg = (W + 7) / 8;
  p.dst_dtype = dst_dtype;
  for (int c = 0; c < 3; ++c) {
    p.mean[c] = mean[c];
    p.std[c] = std[c];
  }
  const unsigned blocks = (unsigned)(((long)H * p.wg + 255) / 256);
  hipLaunchKernelGGL(augment_kernel, dim3(blocks, (unsigned)B), dim3(256), 0, s, p);
  return check_launch("augment_kernel");
}
