// Random Erasing (Zhong et al. 2017; a restatement of timm's RandomErasing._erase) for a dense classification batch (gfx950): the
// device-side draw of the boxes and the write-only fill.  Two launches per batch, no host value that changes between calls: the
// (seed, step) pair lives in device memory, the draw bumps the step, so a captured training step erases anew on every replay.
//
// ---- the Philox streams (philox.h; the numpy restatement tests/random_erase_ref.py is written from this comment) -------------
// Every word comes from philox4x32_10(counter = (c0, c1, c2, c3), key = (seed lo, seed hi)) with
//   c0 = index & 0xffffffff,  c1 = (tag << 24) | (index >> 32)  (index < 2^56),  c2 = step lo,  c3 = step hi.
// Three tags, so the three streams of one (seed, step) never share a (counter, key) pair:
//   tag 1, the box draw.   index = b * 128 + j for sample b:
//            j = 0               word 0 = the sample word (erased iff word < thr), word 1 = the count word
//                                (count = min_count + umulhi(word, max_count - min_count + 1)); words 2, 3 unused
//            j = 1 + k * 10 + a  attempt a < 10 of erase k < count <= 8: word 0 = area, 1 = aspect, 2 = top, 3 = left
//   tag 2, the colours of mode `rand`.   index = (b * 8 + k) * Ch + channel: words 0, 1 = (u1, u2) of ONE normal (the cos branch)
//   tag 3, the noise of mode `pixel`.    index = i >> 2 for flat element i = ((b * Ch + c) * H + y) * W + x: words (i & 2, (i & 2) + 1)
//            = (u1, u2); even i takes the cos branch, odd i the sin branch of that pair
// Uniforms: the draw uses u = (word + 0.5) * 2^-32 in fp64; the normals use u = ((word >> 9) + 0.5) * 2^-23, exact in fp32, and
// z = sqrt(-2 ln u1) * {cos, sin}(2 pi u2) in fp32 (Box-Muller).
#include "mv_common.h"
#include "philox.h"

// the draw is compared bit for bit with a numpy restatement: a + b * c stays a product and a sum, never a fused multiply-add
#pragma clang fp contract(off)

namespace {

constexpr unsigned RE_TAG_DRAW = 1u << 24, RE_TAG_COLOUR = 2u << 24, RE_TAG_PIXEL = 3u << 24;
constexpr int RE_MAX_COUNT = 8, RE_ATTEMPTS = 10;

__device__ __forceinline__ void re_philox(unsigned tag, uint64_t index, uint64_t seed, uint64_t step, unsigned (&w)[4]) {
  philox4x32_10((unsigned)index, tag | (unsigned)(index >> 32), (unsigned)step, (unsigned)(step >> 32), (unsigned)seed,
                (unsigned)(seed >> 32), w);
}

// ---- the draw: boxes[b, k] = (top, left, h, w) of erase k of sample b, zeros where nothing is erased ---------------------------
// ONE workgroup draws every sample and then bumps the step: no other workgroup exists that could read the step after the bump, and
// the barrier puts every thread's read in front of it.  used[0..1] = the (seed, step) of THIS draw, for the fill.
__global__ __launch_bounds__(256) void random_erase_draw_kernel(uint64_t* state, int* __restrict__ boxes, uint64_t* __restrict__ used,
                                                                int B, int H, int W, uint64_t thr, double min_area, double max_area,
                                                                double log_lo, double log_hi, int min_count, int max_count) {
  const uint64_t seed = state[0], step = state[1];
  const double area = (double)H * (double)W;
  for (int b = threadIdx.x; b < B; b += 256) {
    unsigned w[4];
    re_philox(RE_TAG_DRAW, (uint64_t)b * 128, seed, step, w);
    const int count = (uint64_t)w[0] < thr ? min_count + (int)__umulhi(w[1], (unsigned)(max_count - min_count + 1)) : 0;
    int4* out = reinterpret_cast<int4*>(boxes) + (long)b * max_count;
    for (int k = 0; k < max_count; ++k) {
      int4 box = make_int4(0, 0, 0, 0);
      if (k < count)
        for (int a = 0; a < RE_ATTEMPTS; ++a) {
          re_philox(RE_TAG_DRAW, (uint64_t)b * 128 + 1 + k * RE_ATTEMPTS + a, seed, step, w);
          const double ua = ((double)w[0] + 0.5) * 0x1p-32, ur = ((double)w[1] + 0.5) * 0x1p-32;
          const double target = (min_area + ua * (max_area - min_area)) * area / (double)count;
          const double ratio = exp(log_lo + ur * (log_hi - log_lo));
          const double hd = rint(sqrt(target * ratio)), wd = rint(sqrt(target / ratio));      // round half to even: python's round
          if (hd < (double)H && wd < (double)W) {                                             // false for a NaN, too
            const int h = (int)hd, ww = (int)wd;
            box = make_int4((int)__umulhi(w[2], (unsigned)(H - h + 1)), (int)__umulhi(w[3], (unsigned)(W - ww + 1)), h, ww);
            break;
          }
        }
      out[k] = box;
    }
  }
  if (threadIdx.x == 0) { used[0] = seed; used[1] = step; }
  __syncthreads();
  if (threadIdx.x == 0) state[1] = step + 1;
}

// ---- the fill -------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void re_store(unsigned* p, float v) { *p = __float_as_uint(v); }
__device__ __forceinline__ void re_store(unsigned short* p, float v) {
  const bf16_t h = (bf16_t)v;                      // round to nearest even, once
  *p = *reinterpret_cast<const unsigned short*>(&h);
}

// one N(0, 1) value from the word pair (a, b): the cos branch, or the sin branch
__device__ __forceinline__ float re_normal(unsigned a, unsigned b, bool sin_branch) {
  const float u1 = ((float)(a >> 9) + 0.5f) * 0x1p-23f, u2 = ((float)(b >> 9) + 0.5f) * 0x1p-23f;
  float s, c;
  sincospif(2.0f * u2, &s, &c);                    // 2 * u2 is exact: the angle is not rounded before the reduction
  return sqrtf(-2.0f * logf(u1)) * (sin_branch ? s : c);
}

// Workgroup (slot = b * max_count + k, band): one wave per (channel, box row), lanes along the row; the Ch * h rows of the box go
// round the band's four waves and the gridDim.y bands.  Nothing is loaded from x.  An element that a LATER non-empty box of the
// same sample covers is skipped: timm writes the boxes in order, so the last one wins, and here no element is written twice.
// The box is clipped to the image before anything is written, whatever the table holds.
// U: the element's bit pattern (unsigned: fp32, unsigned short: bf16).  MODE 0 const, 1 rand, 2 pixel.
constexpr int RE_ROWS_PER_BLOCK = 32, RE_MAX_BANDS = 32;
template <typename U, int MODE>
__global__ __launch_bounds__(256) void random_erase_apply_kernel(U* __restrict__ x, const int* __restrict__ boxes,
                                                                 const uint64_t* __restrict__ used, int Ch, int H, int W,
                                                                 int max_count) {
  const int4* table = reinterpret_cast<const int4*>(boxes);
  const long slot = blockIdx.x;
  const int4 box = table[slot];
  if (box.z <= 0 || box.w <= 0) return;            // an empty slot: 16 bytes read
  const long b = slot / max_count;
  const int k = (int)(slot - b * max_count);
  const long y0 = box.x < 0 ? 0 : box.x, y1 = (long)box.x + box.z < H ? (long)box.x + box.z : H;
  const long x0 = box.y < 0 ? 0 : box.y, x1 = (long)box.y + box.w < W ? (long)box.y + box.w : W;
  const long bh = y1 - y0;
  if (bh <= 0 || x1 <= x0) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint64_t seed = 0, step = 0;
  if (MODE != 0) { seed = used[0]; step = used[1]; }
  const long rows = (long)Ch * bh;
  for (long rr = blockIdx.y * 4L + wave; rr < rows; rr += gridDim.y * 4L) {
    const long c = rr / bh, y = y0 + (rr - c * bh);
    const long base = ((b * Ch + c) * H + y) * W;
    float colour = 0.f;
    if (MODE == 1) {
      unsigned w[4];
      re_philox(RE_TAG_COLOUR, (uint64_t)((b * RE_MAX_COUNT + k) * Ch + c), seed, step, w);
      colour = re_normal(w[0], w[1], false);
    }
    for (long xx = x0 + lane; xx < x1; xx += 64) {
      bool later = false;
      for (int k2 = k + 1; k2 < max_count; ++k2) {
        const int4 o = table[b * max_count + k2];
        later |= o.z > 0 && o.w > 0 && y >= o.x && y < (long)o.x + o.z && xx >= o.y && xx < (long)o.y + o.w;
      }
      if (later) continue;
      float v = colour;
      if (MODE == 2) {
        const uint64_t i = (uint64_t)(base + xx);
        unsigned w[4];
        re_philox(RE_TAG_PIXEL, i >> 2, seed, step, w);
        v = re_normal((i & 2) ? w[2] : w[0], (i & 2) ? w[3] : w[1], i & 1);
      }
      re_store(x + base + xx, v);
    }
  }
}

}  // namespace

extern "C" int mv_random_erase_draw(uint64_t* state, int32_t* boxes, uint64_t* used, int B, int H, int W, uint64_t thr,
                                    const double* area_ratio, int min_count, int max_count, mv_stream_t stream) {
  MV_REQUIRE(B >= 0 && H > 0 && W > 0, MV_ERR_SHAPE);
  MV_REQUIRE(min_count >= 1 && min_count <= max_count && max_count <= RE_MAX_COUNT, MV_ERR_UNSUPPORTED);
  MV_REQUIRE(thr <= (1ull << 32), MV_ERR_UNSUPPORTED);
  if (B == 0) return MV_OK;                        // nothing to draw: state stays as it is, no pointer is looked at
  MV_REQUIRE(area_ratio, MV_ERR_ALIGN);            // a HOST array, read here: the four doubles become launch arguments
  const double min_area = area_ratio[0], max_area = area_ratio[1], log_lo = area_ratio[2], log_hi = area_ratio[3];
  MV_REQUIRE(min_area > 0.0 && min_area <= max_area && max_area <= 1.0 && log_lo <= log_hi && log_lo - log_lo == 0.0 &&
                 log_hi - log_hi == 0.0,           // finite; a NaN fails every one
             MV_ERR_UNSUPPORTED);
  MV_REQUIRE(state && boxes && used && mv_aligned16(state) && mv_aligned16(boxes) && mv_aligned16(used), MV_ERR_ALIGN);
  return mv_launch<random_erase_draw_kernel>(MV_HERE, 1, 256, 0, (hipStream_t)stream, state, (int*)boxes, used, B, H, W, thr,
                                             min_area, max_area, log_lo, log_hi, min_count, max_count);
}

extern "C" int mv_random_erase_apply(void* x, int elem, const int32_t* boxes, const uint64_t* used, int B, int Ch, int H, int W,
                                     int max_count, int mode, mv_stream_t stream) {
  MV_REQUIRE(B >= 0 && Ch > 0 && H > 0 && W > 0, MV_ERR_SHAPE);
  MV_REQUIRE(elem == MV_F32 || elem == MV_BF16, MV_ERR_UNSUPPORTED);
  MV_REQUIRE(mode >= 0 && mode <= 2 && max_count >= 1 && max_count <= RE_MAX_COUNT, MV_ERR_UNSUPPORTED);
  // every Philox index below 2^56 (pixel: numel / 4; colour: B * 8 * Ch), every slot a workgroup of grid.x
  MV_REQUIRE((double)B * Ch * H * W < 0x1p58 && (long)B * max_count <= 0x7fffffffL, MV_ERR_UNSUPPORTED);
  if (B == 0) return MV_OK;
  MV_REQUIRE(x && boxes && used && mv_aligned16(boxes), MV_ERR_ALIGN);           // x: single-element stores, any alignment
  long bands = ((long)Ch * H + RE_ROWS_PER_BLOCK - 1) / RE_ROWS_PER_BLOCK;       // 32 rows of a full-height box per workgroup ...
  if (bands > RE_MAX_BANDS) bands = RE_MAX_BANDS;                                // ... at most 32 bands; the rows go round beyond
  const dim3 grid((unsigned)((long)B * max_count), (unsigned)bands);
  return mv_pick<MV_F32, MV_BF16>(elem, [&](auto D) {
    using U = std::conditional_t<D() == MV_F32, unsigned, unsigned short>;
    return mv_pick<0, 1, 2>(mode, [&](auto M) {
      return mv_launch<random_erase_apply_kernel<U, M()>>(MV_HERE, grid, 256, 0, (hipStream_t)stream, (U*)x, (const int*)boxes, used,
                                                          Ch, H, W, max_count);
    });
  });
}
