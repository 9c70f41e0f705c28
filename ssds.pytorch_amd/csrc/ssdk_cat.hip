// ssdk_cat.hip -- the two operations of the YOLO necks (ssds/yolo.py) that are no convolution, on gfx950: channel concatenation
// with an optional nearest x2 upsample of the second source, and the SPP block.  NHWC, bf16 | f16, HBM-bound, 16-byte vectors, one
// launch each behind ssdk_cat2 / ssdk_spp (include/ssdk_cat.h).  Every output element is a copy of an input element.
//
//   cat2_kernel  y [N][H][W][C1 + C2] = a [N][H][W][C1] || R(b): a lane owns 8 channels (16 bytes) of one output pixel and copies
//                them from a, from b at the same pixel (SSDK_FUSE_SAME) or from b's parent pixel (oy / 2, ox / 2) (SSDK_FUSE_UP2):
//                the upsampled tensor of torch.cat((a, F.interpolate(b, scale_factor=2)), 1) is never written.  Neighbouring lanes
//                own neighbouring octets: a wave reads and writes whole runs of a pixel's channels.
//
//   spp_kernel   y [N][H][W][4 C] = x || maxpool5(x) || maxpool9(x) || maxpool13(x), stride 1, padding k / 2 that never wins (the
//                maxima run over the pixels inside the map).  A workgroup owns (image, pixel tile, slice of `cs` channel octets)
//                and stages its tile + a halo of 6, clipped to the map, in LDS ONCE -- as order-preserving 16-bit keys
//                (key = bits ^ (sign ? 0xffff : 0x8000): an unsigned compare of keys is the numeric compare of the floats, with
//                -0 < +0; NaNs are made positive at staging and are then the largest keys, so a window that holds one gives one),
//                two to a dword, so a maximum of 8 channels is four packed 16-bit unsigned maxima.
//                Form: SEPARABLE -- pass 1 takes, per staged row and tile column, the row maxima over 5, 9 and 13 columns from 13
//                nested reads (r5 within r9 within r13; a column outside the map is clamped to the border column) into three LDS images; pass 2 takes per output pixel the column maxima of
//                r5 / r9 / r13 over 5 / 9 / 13 rows.  Both are exact for max on the clipped domain.  Against the cascade
//                (9 = 5 o 5, 13 = 5 o 5 o 5: three row + column rounds = six dependent LDS passes and barriers, for 30 instead
//                of 40 reads per pixel) the separable form has two passes and two barriers, and every LDS access of either is a
//                16-byte read or write at consecutive addresses over a wave (ds_read_b128 / ds_write_b128, conflict-free): 40
//                reads of 1 KiB per wave and 64 output pixels-octets, far below the time the 5 C bytes per pixel take from and to
//                HBM.  Slice 0 is copied from x itself (not from the keys), so it keeps every bit, NaN payloads included.
//                Launch (a function of the shape alone): the whole map is one tile, with cs = 4, 2 or 1 octets (the widest that
//                keeps the four images within 64 KiB: H W cs <= 1024) -- 16 x 16 and everything smaller at cs = 4, i.e. 64
//                contiguous bytes per pixel and slice; larger maps are cut into tiles of at most 16 x 16 at cs = 1.
#include "ssdk_conv_common.h"
#include "../../include/ssdk_cat.h"

namespace ssdk {

struct CatParams {
  const u16* a;
  const u16* b;
  u16* y;
  int H, W, C1, C2, up2;
  long total;  // N * H * W * (C1 + C2) / 8 lanes
};

__global__ __launch_bounds__(256) void cat2_kernel(const CatParams p) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= p.total) return;
  const int g1 = p.C1 / 8, g = g1 + p.C2 / 8;
  unsigned pix;  // fewer than 2^31 pixels
  int o;
  if (p.total <= 0x7fffffffL) {  // (uniform) 32-bit division wherever the lane index allows it
    pix = (unsigned)t / (unsigned)g;
    o = (int)((unsigned)t - pix * (unsigned)g);
  } else {
    pix = (unsigned)(t / g);
    o = (int)(t - (long)pix * g);
  }
  const u16* src;
  if (o < g1) {
    src = p.a + (size_t)pix * p.C1 + 8 * o;
  } else if (!p.up2) {
    src = p.b + (size_t)pix * p.C2 + 8 * (o - g1);
  } else {  // b is [N][H / 2][W / 2][C2]: the parent pixel
    const unsigned ox = pix % (unsigned)p.W, r = pix / (unsigned)p.W;
    const unsigned oy = r % (unsigned)p.H, n = r / (unsigned)p.H;
    src = p.b + (((size_t)n * (p.H >> 1) + (oy >> 1)) * (p.W >> 1) + (ox >> 1)) * p.C2 + 8 * (o - g1);
  }
  *reinterpret_cast<u32x4*>(p.y + (size_t)t * 8) = *reinterpret_cast<const u32x4*>(src);
}

constexpr int kSppHalo = 6;       // window 13
constexpr int kSppTile = 16;      // tile side of a map that is not one tile
constexpr int kSppWholeMap = 1024;  // H * W * cs up to which the whole map is one tile: (1 + 3) images * 16 bytes = 64 KiB

struct SppParams {
  const u16* x;
  u16* y;
  int H, W, C;
  int th, tw, tiles_y, tiles_x;  // tile size, tiles per map
  int cs, cgroups;               // channel octets per workgroup, workgroups per pixel tile
  int s_cap, r_cap;              // LDS elements (16 bytes) of the staged image and of each row-maxima image
};

typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ u32 pkmax(u32 a, u32 b) {  // v_pk_max_u16
  return __builtin_bit_cast(u32, __builtin_elementwise_max(__builtin_bit_cast(u16x2, a), __builtin_bit_cast(u16x2, b)));
}
__device__ __forceinline__ u32x4 pkmax4(const u32x4 a, const u32x4 b) {
  return u32x4{pkmax(a[0], b[0]), pkmax(a[1], b[1]), pkmax(a[2], b[2]), pkmax(a[3], b[3])};
}

template <int DT>
__device__ __forceinline__ u32 key_of_half(u32 h) {  // h: 16 bits
  constexpr u32 inf = DT == SSDK_BF16 ? 0x7f80u : 0x7c00u;
  if ((h & 0x7fffu) > inf) h &= 0x7fffu;  // NaN: positive, above +inf
  return h ^ ((h & 0x8000u) ? 0xffffu : 0x8000u);
}
template <int DT>
__device__ __forceinline__ u32x4 keys_of(const u32x4 v) {
  u32x4 k;
#pragma unroll
  for (int e = 0; e < 4; ++e) k[e] = key_of_half<DT>(v[e] & 0xffffu) | (key_of_half<DT>(v[e] >> 16) << 16);
  return k;
}
__device__ __forceinline__ u32x4 bits_of(const u32x4 k) {  // the inverse of keys_of: a key with its top bit set was positive
  u32x4 v;
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] = k[e] ^ ((((~k[e]) >> 15) & 0x00010001u) * 0xffffu | 0x80008000u);
  return v;
}

template <int DT>
__global__ __launch_bounds__(256) void spp_kernel(const SppParams p) {
  extern __shared__ u32x4 spp_lds[];  // [staged pixel][cs] | r5, r9, r13: [staged row][tile column][cs]
  u32x4* xs = spp_lds;
  u32x4* r5 = xs + p.s_cap;
  u32x4* r9 = r5 + p.r_cap;
  u32x4* r13 = r9 + p.r_cap;
  const int tid = (int)threadIdx.x, cs = p.cs;
  int b = (int)blockIdx.x;
  const int cg = b % p.cgroups;
  b /= p.cgroups;
  const int tile = b % (p.tiles_y * p.tiles_x);
  const int n = b / (p.tiles_y * p.tiles_x);
  const int ty0 = (tile / p.tiles_x) * p.th, tx0 = (tile % p.tiles_x) * p.tw;
  const int th = min(p.th, p.H - ty0), tw = min(p.tw, p.W - tx0);
  const int sy0 = max(0, ty0 - kSppHalo), sx0 = max(0, tx0 - kSppHalo);
  const int sh = min(p.H, ty0 + th + kSppHalo) - sy0, sw = min(p.W, tx0 + tw + kSppHalo) - sx0;
  const int oct0 = cg * cs, octs = p.C / 8;
  // stage: the tile and its halo, clipped to the map, as keys
  for (int i = tid; i < sh * sw * cs; i += 256) {
    const int o = i % cs, sp = i / cs;
    const int sy = sp / sw, sx = sp - sy * sw;
    u32x4 v = u32x4{0u, 0u, 0u, 0u};
    if (oct0 + o < octs)
      v = *reinterpret_cast<const u32x4*>(p.x + (((size_t)n * p.H + sy0 + sy) * p.W + sx0 + sx) * p.C + 8 * (oct0 + o));
    xs[i] = keys_of<DT>(v);
  }
  __syncthreads();
  // pass 1: maxima along the row over 5 / 9 / 13 columns, for every staged row and every column of the tile
  for (int i = tid; i < sh * tw * cs; i += 256) {
    const int o = i % cs, rp = i / cs;
    const int ry = rp / tw, tx = rp - ry * tw;
    const int ax = tx0 + tx;  // column in the map; ax + d inside the map is inside the staged columns
    const int row = (ry * sw - sx0) * cs + o;  // xs[row + column * cs]
    u32x4 m = xs[row + ax * cs];
    // a column outside the map is clamped to the border column: max is idempotent, so reading a pixel of the window twice changes
    // nothing, and without a branch around them the 12 reads are issued back to back instead of one LDS latency after the other
#pragma unroll
    for (int d = 1; d <= kSppHalo; ++d) {
      m = pkmax4(m, xs[row + max(ax - d, 0) * cs]);
      m = pkmax4(m, xs[row + min(ax + d, p.W - 1) * cs]);
      if (d == 2) r5[i] = m;
      if (d == 4) r9[i] = m;
    }
    r13[i] = m;
  }
  __syncthreads();
  // pass 2: maxima along the column of the row maxima; slice 0 is x itself
  for (int i = tid; i < th * tw * cs; i += 256) {
    const int o = i % cs, tp = i / cs;
    if (oct0 + o >= octs) continue;
    const int ty = tp / tw, tx = tp - ty * tw;
    const int ay = ty0 + ty;  // row in the map; ay + d inside the map is inside the staged rows
    const int col = tx * cs + o, ry = ay - sy0;
    u32x4 m5 = r5[ry * tw * cs + col], m9 = r9[ry * tw * cs + col], m13 = r13[ry * tw * cs + col];
#pragma unroll
    for (int d = 1; d <= kSppHalo; ++d) {  // rows outside the map are clamped to the border row, as the columns above
      const int up = (max(ay - d, 0) - sy0) * tw * cs + col, dn = (min(ay + d, p.H - 1) - sy0) * tw * cs + col;
      if (d <= 2) m5 = pkmax4(pkmax4(m5, r5[up]), r5[dn]);
      if (d <= 4) m9 = pkmax4(pkmax4(m9, r9[up]), r9[dn]);
      m13 = pkmax4(pkmax4(m13, r13[up]), r13[dn]);
    }
    const size_t pix = ((size_t)n * p.H + ay) * p.W + tx0 + tx;
    const int c0 = 8 * (oct0 + o);
    u16* yp = p.y + pix * 4 * p.C + c0;
    *reinterpret_cast<u32x4*>(yp) = *reinterpret_cast<const u32x4*>(p.x + pix * p.C + c0);
    *reinterpret_cast<u32x4*>(yp + p.C) = bits_of(m5);
    *reinterpret_cast<u32x4*>(yp + 2 * p.C) = bits_of(m9);
    *reinterpret_cast<u32x4*>(yp + 3 * p.C) = bits_of(m13);
  }
}

}  // namespace ssdk

using namespace ssdk;

extern "C" size_t ssdk_cat_desc_bytes(void) { return sizeof(ssdk_cat_desc); }
extern "C" size_t ssdk_spp_desc_bytes(void) { return sizeof(ssdk_spp_desc); }

extern "C" int ssdk_cat2(const ssdk_cat_desc* d, void* stream) {
  if (!d) {
    set_error("cat2: null descriptor");
    return SSDK_E_BADARG;
  }
  if (d->dtype != SSDK_BF16 && d->dtype != SSDK_F16) {
    set_error("cat2: dtype must be bf16 or f16");
    return SSDK_E_BADARG;
  }
  if (d->mode != SSDK_FUSE_SAME && d->mode != SSDK_FUSE_UP2) {
    set_error("cat2: mode %d (SSDK_FUSE_SAME or SSDK_FUSE_UP2)", d->mode);
    return SSDK_E_BADARG;
  }
  if (d->N < 1 || d->H < 1 || d->W < 1 || d->C1 < 8 || d->C2 < 8 || (d->C1 % 8) || (d->C2 % 8) || d->C1 > (1 << 20) || d->C2 > (1 << 20)) {
    set_error("cat2: bad geometry N=%d H=%d W=%d C1=%d C2=%d (N, H, W >= 1; C1 and C2 multiples of 8)", d->N, d->H, d->W, d->C1, d->C2);
    return SSDK_E_BADARG;
  }
  if (d->mode == SSDK_FUSE_UP2 && ((d->H | d->W) & 1)) {
    set_error("cat2: an upsampled source needs even output dims (%dx%d)", d->H, d->W);
    return SSDK_E_BADARG;
  }
  const long long M = (long long)d->N * d->H * d->W;
  const long long total = M * ((d->C1 + d->C2) / 8);
  if (M > 0x7fffffffLL || (total + 255) / 256 > 0x7fffffffLL) {
    set_error("cat2: N H W = %lld pixels (fewer than 2^31, and fewer than 2^31 workgroups of 256 octets)", M);
    return SSDK_E_BADARG;
  }
  if (!d->a || !d->b || !d->y) {
    set_error("cat2: null pointer (a, b and y are required)");
    return SSDK_E_BADARG;
  }
  if (((uintptr_t)d->a | (uintptr_t)d->b | (uintptr_t)d->y) & 15) {
    set_error("cat2: a, b and y must be 16-byte aligned");
    return SSDK_E_BADARG;
  }
  CatParams p;
  p.a = (const u16*)d->a;
  p.b = (const u16*)d->b;
  p.y = (u16*)d->y;
  p.H = d->H, p.W = d->W, p.C1 = d->C1, p.C2 = d->C2, p.up2 = d->mode == SSDK_FUSE_UP2;
  p.total = (long)total;
  hipLaunchKernelGGL(cat2_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, p);
  return check_launch("cat2_kernel");
}

extern "C" int ssdk_spp(const ssdk_spp_desc* d, void* stream) {
  if (!d) {
    set_error("spp: null descriptor");
    return SSDK_E_BADARG;
  }
  if (d->dtype != SSDK_BF16 && d->dtype != SSDK_F16) {
    set_error("spp: dtype must be bf16 or f16");
    return SSDK_E_BADARG;
  }
  if (d->N < 1 || d->H < 1 || d->W < 1 || d->C < 8 || (d->C % 8) || d->C > (1 << 20)) {
    set_error("spp: bad geometry N=%d H=%d W=%d C=%d (N, H, W >= 1; C a multiple of 8)", d->N, d->H, d->W, d->C);
    return SSDK_E_BADARG;
  }
  const long long M = (long long)d->N * d->H * d->W;
  if (M > 0x7fffffffLL) {
    set_error("spp: N H W = %lld pixels (fewer than 2^31)", M);
    return SSDK_E_BADARG;
  }
  if (!d->x || !d->y) {
    set_error("spp: null pointer (x and y are required)");
    return SSDK_E_BADARG;
  }
  if (((uintptr_t)d->x | (uintptr_t)d->y) & 15) {
    set_error("spp: x and y must be 16-byte aligned");
    return SSDK_E_BADARG;
  }
  SppParams p;
  p.x = (const u16*)d->x;
  p.y = (u16*)d->y;
  p.H = d->H, p.W = d->W, p.C = d->C;
  const int octs = d->C / 8;
  const long long hw = (long long)d->H * d->W;
  p.cs = 0;
  for (int cs = 4; cs >= 1; cs >>= 1)
    if (cs <= octs && hw * cs <= kSppWholeMap) {
      p.cs = cs;
      break;
    }
  if (p.cs) {  // the whole map is one tile
    p.tiles_y = p.tiles_x = 1;
    p.th = d->H, p.tw = d->W;
  } else {
    p.cs = 1;
    p.tiles_y = (d->H + kSppTile - 1) / kSppTile, p.tiles_x = (d->W + kSppTile - 1) / kSppTile;
    p.th = (d->H + p.tiles_y - 1) / p.tiles_y, p.tw = (d->W + p.tiles_x - 1) / p.tiles_x;
  }
  p.cgroups = (octs + p.cs - 1) / p.cs;
  const int sh_cap = d->H < p.th + 2 * kSppHalo ? d->H : p.th + 2 * kSppHalo;
  const int sw_cap = d->W < p.tw + 2 * kSppHalo ? d->W : p.tw + 2 * kSppHalo;
  p.s_cap = sh_cap * sw_cap * p.cs, p.r_cap = sh_cap * p.tw * p.cs;
  const size_t lds = (size_t)(p.s_cap + 3 * p.r_cap) * 16;  // <= 64 KiB by construction: 28 * 28 + 3 * 28 * 16 elements at most
  const long long blocks = (long long)d->N * p.tiles_y * p.tiles_x * p.cgroups;
  if (blocks > 0x7fffffffLL || lds > 65536) {
    set_error("spp: N=%d H=%d W=%d C=%d needs %lld workgroups (fewer than 2^31)", d->N, d->H, d->W, d->C, blocks);
    return SSDK_E_BADARG;
  }
  hipStream_t st = (hipStream_t)stream;
  if (d->dtype == SSDK_BF16) hipLaunchKernelGGL((spp_kernel<SSDK_BF16>), dim3((unsigned)blocks), dim3(256), lds, st, p);
  else hipLaunchKernelGGL((spp_kernel<SSDK_F16>), dim3((unsigned)blocks), dim3(256), lds, st, p);
  return check_launch("spp_kernel");
}
