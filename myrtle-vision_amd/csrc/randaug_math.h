// Per-pixel and per-table arithmetic of RandAugment (randaug.hip), written once and free of anything device specific so that the
// same text also compiles for the host (tests/test_randaug_cpu.py builds it with the host compiler and holds it to Pillow before
// any GPU is involved).  Every function restates what Pillow 12 computes for 8-bit RGB:
//   affine gather  libImaging/Geometry.c  affine_transform + bilinear_filter32RGB / bicubic_filter32RGB (fp64)
//   blend          libImaging/Blend.c     ImagingBlend (fp32, the factor a float)
//   SMOOTH         libImaging/Filter.c    ImagingFilter3x3 with (1,1,1,1,5,1,1,1,1)/13
//   tables         ImageOps.py            invert, posterize, solarize, autocontrast, equalize; timm's solarize_add
// Pillow's binary is built without contraction: a * b + c is a product and a sum here as well.
#pragma once
#include <math.h>
#include <stdint.h>

#pragma clang fp contract(off)

#ifdef __HIPCC__
#define RA_HD __host__ __device__ __forceinline__
#else
#define RA_HD static inline
#endif

// op codes of ra_op: 0 = the slot is skipped; 1..15 = timm's increasing set in the order of datasets/transforms.RANDAUG_OPS
enum {
  RA_SKIP = 0, RA_AUTOCONTRAST = 1, RA_EQUALIZE = 2, RA_INVERT = 3, RA_ROTATE = 4, RA_POSTERIZE = 5, RA_SOLARIZE = 6,
  RA_SOLARIZE_ADD = 7, RA_COLOR = 8, RA_CONTRAST = 9, RA_BRIGHTNESS = 10, RA_SHARPNESS = 11, RA_SHEAR_X = 12, RA_SHEAR_Y = 13,
  RA_TRANSLATE_X = 14, RA_TRANSLATE_Y = 15, RA_NUM_OPS = 15
};
RA_HD bool ra_is_geometric(int op) { return op == RA_ROTATE || (op >= RA_SHEAR_X && op <= RA_TRANSLATE_Y); }
RA_HD bool ra_is_enhance(int op) { return op >= RA_COLOR && op <= RA_SHARPNESS; }
RA_HD bool ra_needs_stats(int op) { return op == RA_AUTOCONTRAST || op == RA_EQUALIZE || op == RA_CONTRAST; }

RA_HD int ra_clip(int v, int n) { return v < 0 ? 0 : (v >= n ? n - 1 : v); }            // XCLIP / YCLIP
RA_HD int ra_floor(double v) { return v < 0.0 ? (int)floor(v) : (int)v; }                // Geometry.c FLOOR
RA_HD int ra_luma(int r, int g, int b) { return (r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16; }   // convert("L")

// ---- the affine gather: output pixel (x, y) of Image.transform(size, AFFINE, a, resample, fillcolor) -----------------------------
RA_HD double ra_cubic(double v1, double v2, double v3, double v4, double d) {
  const double p1 = v2;
  const double p2 = -v1 + v3;
  const double p3 = 2 * (v1 - v2) + v3 - v4;
  const double p4 = -v1 + v2 - v3 + v4;
  return p1 + d * (p2 + d * (p3 + d * p4));
}

// img: uint8 [H, W, 3]; o: the pixel's 3 bytes; fill: the colour outside the source
RA_HD void ra_affine_pixel(const uint8_t* img, int H, int W, const double* a, bool bicubic, int x, int y, const int* fill,
                           uint8_t* o) {
  const double xc = x + 0.5, yc = y + 0.5;
  double xin = a[0] * xc + a[1] * yc + a[2];
  double yin = a[3] * xc + a[4] * yc + a[5];
  if (!(xin >= 0.0 && xin < W && yin >= 0.0 && yin < H)) {          // outside (or not a number): the fill colour
    o[0] = (uint8_t)fill[0], o[1] = (uint8_t)fill[1], o[2] = (uint8_t)fill[2];
    return;
  }
  xin -= 0.5;
  yin -= 0.5;
  int x0 = ra_floor(xin), y0 = ra_floor(yin);
  const double dx = xin - x0, dy = yin - y0;
  if (!bicubic) {
    const int c0 = ra_clip(x0, W) * 3, c1 = ra_clip(x0 + 1, W) * 3;
    const uint8_t* r0 = img + (long)ra_clip(y0, H) * W * 3;
    const bool below = y0 + 1 >= 0 && y0 + 1 < H;
    const uint8_t* r1 = img + (long)(below ? y0 + 1 : 0) * W * 3;
    for (int c = 0; c < 3; ++c) {
      double v1 = (double)r0[c0 + c] + (double)((int)r0[c1 + c] - (int)r0[c0 + c]) * dx;
      double v2 = v1;
      if (below) v2 = (double)r1[c0 + c] + (double)((int)r1[c1 + c] - (int)r1[c0 + c]) * dx;
      v1 = v1 + (v2 - v1) * dy;
      o[c] = (uint8_t)(int)v1;
    }
    return;
  }
  x0 -= 1;
  y0 -= 1;
  int col[4];
  for (int j = 0; j < 4; ++j) col[j] = ra_clip(x0 + j, W) * 3;
  for (int c = 0; c < 3; ++c) {
    double v[4];
    for (int j = 0; j < 4; ++j) {
      const int yy = y0 + j;
      if (j == 0 || (yy >= 0 && yy < H)) {
        const uint8_t* r = img + (long)(j == 0 ? ra_clip(yy, H) : yy) * W * 3 + c;
        v[j] = ra_cubic((double)r[col[0]], (double)r[col[1]], (double)r[col[2]], (double)r[col[3]], dx);
      } else {
        v[j] = v[j - 1];
      }
    }
    const double r = ra_cubic(v[0], v[1], v[2], v[3], dy);
    o[c] = r <= 0.0 ? 0 : (r >= 255.0 ? 255 : (uint8_t)(int)r);
  }
}

// ---- ImageEnhance: Image.blend(degenerate, image, factor) ------------------------------------------------------------------------
RA_HD uint8_t ra_blend(int d, int s, float f) {
  const float t = (float)d + f * (float)(s - d);
  if (f >= 0.0f && f <= 1.0f) return (uint8_t)(int)t;
  return t <= 0.0f ? 0 : (t >= 255.0f ? 255 : (uint8_t)(int)t);
}

// ImageFilter.SMOOTH at (x, y), channel c.  The float sum of Filter.c is s / 13 + 0.5 up to a few ulp with s an integer; that value is
// an odd multiple of 1 / 26, never closer than 1 / 26 to an integer, so the truncation is that of the exact quotient.
RA_HD int ra_smooth(const uint8_t* img, int H, int W, int x, int y, int c) {
  const uint8_t* p = img + ((long)y * W + x) * 3 + c;
  if (x == 0 || y == 0 || x == W - 1 || y == H - 1) return *p;                             // the border is copied
  const long up = -(long)W * 3, dn = (long)W * 3;
  const int s = p[up - 3] + p[up] + p[up + 3] + p[-3] + 5 * p[0] + p[3] + p[dn - 3] + p[dn] + p[dn + 3];
  return (2 * s + 13) / 26;
}

// ---- tables ----------------------------------------------------------------------------------------------------------------------
// the four that depend on the parameter alone
RA_HD int ra_param_table(int op, int i, int p) {
  switch (op) {
    case RA_INVERT: return 255 - i;
    case RA_POSTERIZE: return p >= 8 ? i : (p <= 0 ? 0 : (i & ~((1 << (8 - p)) - 1)));
    case RA_SOLARIZE: return i < p ? i : 255 - i;
    case RA_SOLARIZE_ADD: return i < 128 ? (i + p > 255 ? 255 : (i + p < 0 ? 0 : i + p)) : i;
    default: return i;
  }
}
// one pass over a channel's 256 bins: before[i] = h[0] + .. + h[i - 1], lo / hi = first / last non-zero bin (256 / -1 if none),
// levels = the non-zero bins, step = (sum of h - the last non-zero bin) / 255
RA_HD void ra_channel_scan(const unsigned* h, long long* before, int* lo, int* hi, int* levels, long long* step) {
  int l = 256, u = -1, n = 0;
  long long total = 0, last = 0;
  for (int i = 0; i < 256; ++i) {
    before[i] = total;
    if (h[i]) {
      if (l == 256) l = i;
      u = i;
      ++n;
      last = h[i];
      total += h[i];
    }
  }
  *lo = l, *hi = u, *levels = n, *step = (total - last) / 255;
}
// ImageOps.autocontrast (cutoff 0): lo / hi = first / last non-zero bin
RA_HD int ra_autocontrast(int i, int lo, int hi) {
  if (hi <= lo) return i;
  const double scale = 255.0 / (double)(hi - lo);
  const double off = (double)(-lo) * scale;
  const int v = (int)((double)i * scale + off);
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}
// ImageOps.equalize: before = h[0] + .. + h[i - 1]; step = (sum of h - last non-zero bin) / 255, 0 or a single level = identity
RA_HD int ra_equalize(int i, long long before, long long step, int levels) {
  if (levels <= 1 || step == 0) return i;
  const long long v = (step / 2 + before) / step;
  return v > 255 ? 255 : (int)v;
}
