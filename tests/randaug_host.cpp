// csrc/randaug_math.h compiled for the HOST: one image per call, a plain loop where the kernels have a thread grid.  Built by
// tests/test_randaug_cpu.py with the host compiler (no contraction) and compared with Pillow, so the arithmetic the kernels inline
// is held to the reference without a GPU.
#include "randaug_math.h"

extern "C" {

void ra_host_affine(const uint8_t* img, int H, int W, const double* a, int bicubic, const int* fill, uint8_t* out) {
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) ra_affine_pixel(img, H, W, a, bicubic != 0, x, y, fill, out + ((long)y * W + x) * 3);
}

int ra_host_mean(const uint8_t* img, int H, int W) {
  long long s = 0;
  for (long i = 0; i < (long)H * W; ++i) s += ra_luma(img[3 * i], img[3 * i + 1], img[3 * i + 2]);
  return (int)((double)s / (double)((long)H * W) + 0.5);
}

void ra_host_enhance(const uint8_t* img, int H, int W, int op, double factor, uint8_t* out) {
  const float f = (float)factor;
  const int mean = op == RA_CONTRAST ? ra_host_mean(img, H, W) : 0;
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      const uint8_t* s = img + ((long)y * W + x) * 3;
      for (int c = 0; c < 3; ++c) {
        int d = 0;
        if (op == RA_COLOR) d = ra_luma(s[0], s[1], s[2]);
        else if (op == RA_CONTRAST) d = mean;
        else if (op == RA_SHARPNESS) d = ra_smooth(img, H, W, x, y, c);
        out[((long)y * W + x) * 3 + c] = ra_blend(d, s[c], f);
      }
    }
}

// the six table ops: table uint8 [3, 256]
void ra_host_table(const uint8_t* img, int H, int W, int op, int p, uint8_t* table) {
  for (int c = 0; c < 3; ++c) {
    unsigned h[256] = {0};
    long long before[256], step;
    int lo, hi, levels;
    for (long i = 0; i < (long)H * W; ++i) ++h[img[3 * i + c]];
    ra_channel_scan(h, before, &lo, &hi, &levels, &step);
    for (int i = 0; i < 256; ++i)
      table[c * 256 + i] = (uint8_t)(op == RA_AUTOCONTRAST ? ra_autocontrast(i, lo, hi)
                                     : op == RA_EQUALIZE   ? ra_equalize(i, before[i], step, levels)
                                                           : ra_param_table(op, i, p));
  }
}
}
