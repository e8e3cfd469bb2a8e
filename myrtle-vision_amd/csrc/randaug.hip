// RandAugment (Cubuk et al. 2020) for a classification batch on the GPU (gfx950): timm's increasing op set (timm.data.auto_augment,
// `rand-m9-mstd0.5-inc1`), restated.  The reference has no call site: it never augments beyond crop and flip.  The worker draws each
// sample's ops and their arguments (datasets/device_transforms.py, the same draws as datasets/transforms.RandAugment); these
// kernels compute the pixels, bit for bit what the Pillow calls of that host chain compute (arithmetic: randaug_math.h).
//
// One slot = one op per sample = two launches over the whole uint8 [B, H, W, 3] batch:
//   mv_randaug_stats   one workgroup per sample; only for AutoContrast, Equalize and Contrast (any other op: the workgroup returns
//                      at once).  Three 256-bin histograms and, for Contrast, the sum of L, with integer LDS atomics -- exact and
//                      order free --, then the 3 x 256 table / the mean, finished in the same launch.  No global atomic, no memset.
//   mv_randaug_apply   one thread per pixel, out of place (Sharpness and the geometric ops read neighbours): writes every byte of dst.
// The op code is uniform within a workgroup (blockIdx.z = the sample), so the switch does not diverge.
#include "mv_common.h"
#include "randaug_math.h"

// compared bit for bit with Pillow's uncontracted arithmetic (the AutoContrast table, the affine coordinates, the fp32 blend)
#pragma clang fp contract(off)

namespace {

constexpr int RA_WAVES = 4;                          // sub-histograms per workgroup: one per wave

// One value per lane into the wave's own histogram.  A flat image sends all 64 lanes to one bin; then one lane adds the count.
// Lane 0 is valid whenever the wave is in the loop.
__device__ __forceinline__ void ra_hist_add(unsigned* h, int v, bool valid, int lane) {
  const int first = __shfl(v, 0, 64);
  const unsigned long long act = __ballot(valid);
  if (__ballot(valid && v != first) == 0ull) {
    if (lane == 0) atomicAdd(h + first, (unsigned)__popcll(act));
  } else if (valid) {
    atomicAdd(h + v, 1u);
  }
}

__global__ __launch_bounds__(256) void randaug_stats_kernel(const uint8_t* __restrict__ src, const int* __restrict__ ops, int num_ops,
                                                            int slot, uint8_t* __restrict__ tables, int* __restrict__ mean, int H, int W) {
  const int b = blockIdx.x;
  const int op = ops[(long)b * num_ops + slot];
  if (!ra_needs_stats(op)) return;
  __shared__ unsigned hist[RA_WAVES][3][256];
  __shared__ long long before[3][256];               // Equalize: the pixels below each level
  __shared__ long long lsum;
  __shared__ int ch_lo[3], ch_hi[3], ch_levels[3];
  __shared__ long long ch_step[3];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int i = threadIdx.x; i < RA_WAVES * 3 * 256; i += 256) (&hist[0][0][0])[i] = 0u;
  if (threadIdx.x == 0) lsum = 0;
  __syncthreads();
  const long n = (long)H * W;
  const uint8_t* img = src + (long)b * n * 3;
  long long mine = 0;
  for (long base = (long)wave * 64; base < n; base += 64 * RA_WAVES) {
    const long i = base + lane;
    const bool valid = i < n;
    int r = 0, g = 0, bl = 0;
    if (valid) { r = img[i * 3]; g = img[i * 3 + 1]; bl = img[i * 3 + 2]; }
    if (op == RA_CONTRAST) {
      if (valid) mine += ra_luma(r, g, bl);
    } else {
      ra_hist_add(hist[wave][0], r, valid, lane);
      ra_hist_add(hist[wave][1], g, valid, lane);
      ra_hist_add(hist[wave][2], bl, valid, lane);
    }
  }
  if (op == RA_CONTRAST) {
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o, 64);
    if (lane == 0) atomicAdd((unsigned long long*)&lsum, (unsigned long long)mine);
    __syncthreads();
    if (threadIdx.x == 0) mean[b] = (int)((double)lsum / (double)n + 0.5);     // ImageStat mean of L, then int(mean + 0.5)
    return;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 3 * 256; i += 256) {                           // the four sub-histograms into the first
    unsigned s = 0;
    for (int w = 0; w < RA_WAVES; ++w) s += (&hist[w][0][0])[i];
    (&hist[0][0][0])[i] = s;
  }
  __syncthreads();
  if (threadIdx.x < 3) {                                                       // per channel: one pass over 256 bins
    const int c = threadIdx.x;
    ra_channel_scan(hist[0][c], before[c], &ch_lo[c], &ch_hi[c], &ch_levels[c], &ch_step[c]);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 3 * 256; i += 256) {
    const int c = i >> 8, v = i & 255;
    const int t = op == RA_AUTOCONTRAST ? ra_autocontrast(v, ch_lo[c], ch_hi[c]) : ra_equalize(v, before[c][v], ch_step[c], ch_levels[c]);
    tables[(long)b * 768 + i] = (uint8_t)t;
  }
}

__global__ __launch_bounds__(256) void randaug_apply_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                            const int* __restrict__ ops, const double* __restrict__ par, int num_ops,
                                                            int slot, const uint8_t* __restrict__ tables, const int* __restrict__ mean,
                                                            int f0, int f1, int f2, int H, int W) {
  const int b = blockIdx.z;
  const int X = blockIdx.x * 64 + (threadIdx.x & 63), Y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (X >= W || Y >= H) return;
  const int op = ops[(long)b * num_ops + slot];
  const double* p = par + ((long)b * num_ops + slot) * 8;
  const uint8_t* img = src + (long)b * H * W * 3;
  const long at = ((long)Y * W + X) * 3;
  uint8_t* o = dst + (long)b * H * W * 3 + at;
  const int s0 = img[at], s1 = img[at + 1], s2 = img[at + 2];
  if (ra_is_geometric(op)) {
    const double a[6] = {p[0], p[1], p[2], p[3], p[4], p[5]};
    const int fill[3] = {f0, f1, f2};
    uint8_t px[3];
    ra_affine_pixel(img, H, W, a, p[6] != 0.0, X, Y, fill, px);
    o[0] = px[0], o[1] = px[1], o[2] = px[2];
  } else if (ra_is_enhance(op)) {
    const float f = (float)p[0];
    int d0 = 0, d1 = 0, d2 = 0;                                                // Brightness: black
    if (op == RA_COLOR) d0 = d1 = d2 = ra_luma(s0, s1, s2);
    else if (op == RA_CONTRAST) d0 = d1 = d2 = mean[b] & 255;
    else if (op == RA_SHARPNESS) { d0 = ra_smooth(img, H, W, X, Y, 0); d1 = ra_smooth(img, H, W, X, Y, 1); d2 = ra_smooth(img, H, W, X, Y, 2); }
    o[0] = ra_blend(d0, s0, f), o[1] = ra_blend(d1, s1, f), o[2] = ra_blend(d2, s2, f);
  } else if (op == RA_AUTOCONTRAST || op == RA_EQUALIZE) {
    const uint8_t* t = tables + (long)b * 768;
    o[0] = t[s0], o[1] = t[256 + s1], o[2] = t[512 + s2];
  } else if (op >= RA_INVERT && op <= RA_SOLARIZE_ADD) {
    const int q = (int)p[0];
    o[0] = (uint8_t)ra_param_table(op, s0, q), o[1] = (uint8_t)ra_param_table(op, s1, q), o[2] = (uint8_t)ra_param_table(op, s2, q);
  } else {                                                                     // a skipped slot (or an unknown code): the copy
    o[0] = (uint8_t)s0, o[1] = (uint8_t)s1, o[2] = (uint8_t)s2;
  }
}

bool ra_shape_ok(int B, int H, int W, int num_ops, int slot) {
  return B >= 0 && B <= 65535 && H > 0 && W > 0 && (long)H * W * 3 <= 0x7fffffffL && mv_cdiv(H, 4) <= 65535 && num_ops >= 1 &&
         slot >= 0 && slot < num_ops;
}

}  // namespace

extern "C" int mv_randaug_stats(const uint8_t* src, const int32_t* ops, int num_ops, int slot, uint8_t* tables, int32_t* mean, int B,
                                int H, int W, mv_stream_t stream) {
  MV_REQUIRE(ra_shape_ok(B, H, W, num_ops, slot), MV_ERR_SHAPE);
  if (B == 0) return MV_OK;
  MV_REQUIRE(src && ops && tables && mean, MV_ERR_ALIGN);
  return mv_launch<randaug_stats_kernel>(MV_HERE, B, 256, 0, (hipStream_t)stream, src, (const int*)ops, num_ops, slot, tables,
                                         (int*)mean, H, W);
}

extern "C" int mv_randaug_apply(const uint8_t* src, uint8_t* dst, const int32_t* ops, const double* par, int num_ops, int slot,
                                const uint8_t* tables, const int32_t* mean, int fill0, int fill1, int fill2, int B, int H, int W,
                                mv_stream_t stream) {
  MV_REQUIRE(ra_shape_ok(B, H, W, num_ops, slot), MV_ERR_SHAPE);
  MV_REQUIRE(fill0 >= 0 && fill0 <= 255 && fill1 >= 0 && fill1 <= 255 && fill2 >= 0 && fill2 <= 255, MV_ERR_UNSUPPORTED);
  if (B == 0) return MV_OK;
  MV_REQUIRE(src && dst && src != dst && ops && par && tables && mean && (reinterpret_cast<uintptr_t>(par) & 7u) == 0, MV_ERR_ALIGN);
  return mv_launch<randaug_apply_kernel>(MV_HERE, dim3(mv_cdiv(W, 64), mv_cdiv(H, 4), B), 256, 0, (hipStream_t)stream, src, dst,
                                         (const int*)ops, par, num_ops, slot, tables, (const int*)mean, fill0, fill1, fill2, H, W);
}
