// Bicubic resize of the positional-embedding grid (reference vit.py:292-302), forward and backward, token-major (gfx950).
//
// pos [1 + sh*sw, D] -> out [1 + gh*gw, D]: row 0 (the cls slot) passes through, rows 1 + y*gw + x are the (sh, sw) grid resized to
// (gh, gw) exactly as torch's upsample_bicubic2d(align_corners=False) defines it.  The reference's (1, D, sh, sw) view is index
// arithmetic here: every access is a float4 along D, never a transposed copy.  Taps and weights are computed in the kernels from
// the four scalars (sh, sw, gh, gw) and the two scales in / out (divided on the host: one IEEE division each, as torch does it).
#include "mv_common.h"

namespace {

constexpr int PR_MAX_SIDE = 1024;     // per side of either grid: the backward keeps one weight per target row / column in LDS

// The four taps of target index `dst` along one axis: torch's area_pixel_compute_source_index(cubic) + guard_index_and_lambda +
// get_cubic_upsample_coefficients (A = -0.75), operation for operation in fp32 -- no contraction into fma, so that the weights are
// the ones torch's fp32 kernel uses and t == 0 gives (0, 1, 0, 0) exactly.  Indices are clamped to [0, in - 1], src is not.
__device__ __forceinline__ void pr_taps(int dst, float scale, int in, int (&idx)[4], float (&w)[4]) {
#pragma clang fp contract(off)
  const float A = -0.75f;
  const float src = scale * ((float)dst + 0.5f) - 0.5f;
  const float fl = floorf(src);
  const int i = min((int)fl, in - 1);
  const float t = fminf(fmaxf(src - (float)i, 0.f), 1.f);
  const float x0 = t + 1.f, x2 = 1.f - t, x3 = x2 + 1.f;
  w[0] = ((A * x0 - 5.f * A) * x0 + 8.f * A) * x0 - 4.f * A;
  w[1] = ((A + 2.f) * t - (A + 3.f)) * t * t + 1.f;
  w[2] = ((A + 2.f) * x2 - (A + 3.f)) * x2 * x2 + 1.f;
  w[3] = ((A * x3 - 5.f * A) * x3 + 8.f * A) * x3 - 4.f * A;
#pragma unroll
  for (int j = 0; j < 4; ++j) idx[j] = max(min(i + j - 1, in - 1), 0);
}

__device__ __forceinline__ float4 pr_ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ float4 pr_mul(float4 v, float s) { return make_float4(v.x * s, v.y * s, v.z * s, v.w * s); }
__device__ __forceinline__ float4 pr_fma(float4 v, float s, float4 a) {
  return make_float4(a.x + v.x * s, a.y + v.y * s, a.z + v.z * s, a.w + v.w * s);
}

// One thread per (target row, 4 channels): 16 float4 loads from the (L2-resident) source grid, rows first and then across rows, the
// order of torch's separable interpolation.
__global__ __launch_bounds__(256) void pos_resize_fwd_kernel(const float* __restrict__ pos, float* __restrict__ out, int sh, int sw,
                                                             int gh, int gw, int D, float hscale, float wscale) {
  const int d4 = D >> 2;
  const long n = ((long)gh * gw + 1) * d4;
  for (long g = blockIdx.x * 256L + threadIdx.x; g < n; g += gridDim.x * 256L) {
    const long tok = g / d4;
    const int c = (int)(g - tok * d4) * 4;
    float4 acc;
    if (tok == 0) {
      acc = pr_ld4(pos + c);
    } else {
      const int p = (int)(tok - 1), y = p / gw, x = p - y * gw;
      int iy[4], ix[4];
      float wy[4], wx[4];
      pr_taps(y, hscale, sh, iy, wy);
      pr_taps(x, wscale, sw, ix, wx);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float* row = pos + (1 + (long)iy[j] * sw) * D + c;
        float4 r = pr_mul(pr_ld4(row + (long)ix[0] * D), wx[0]);
#pragma unroll
        for (int i = 1; i < 4; ++i) r = pr_fma(pr_ld4(row + (long)ix[i] * D), wx[i], r);
        acc = j == 0 ? pr_mul(r, wy[0]) : pr_fma(r, wy[j], acc);
      }
    }
    *reinterpret_cast<float4*>(out + tok * D + c) = acc;
  }
}

// Transpose of the map above as a gather per SOURCE cell: block (source row q of dpos, 128-column chunk), 32 threads x float4
// across the chunk, 8 thread rows.  Along each axis the block first writes, for every target index, the weight it puts on this
// source cell (the sum of its taps that land here: taps clamped onto a border cell all count for that cell) into an LDS table and
// finds the interval of target indices that touch the cell (the tap positions are monotone in the target index, so it IS an
// interval; integer min / max).  The 8 thread rows then stride the (y, x) pairs of the two intervals in a fixed order and their
// partial sums meet in LDS in a fixed order: no floating-point atomics, the same bits every run.  Block 0 .. chunks-1 is the cls row.
__global__ __launch_bounds__(256) void pos_resize_bwd_kernel(const float* __restrict__ dout, float* __restrict__ dpos, int accumulate,
                                                             int sh, int sw, int gh, int gw, int D, float hscale, float wscale) {
  __shared__ float wy_tab[PR_MAX_SIDE], wx_tab[PR_MAX_SIDE];
  __shared__ int lim[4];                         // ylo, yhi, xlo, xhi (inclusive)
  __shared__ float4 red[8][32];
  const int chunks = (D + 127) / 128;
  const int q = blockIdx.x / chunks, ch = blockIdx.x - q * chunks;
  const int cx = threadIdx.x & 31, ry = threadIdx.x >> 5;
  const int c = ch * 128 + cx * 4;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  if (q == 0) {                                  // block-uniform
    if (ry == 0 && c < D) acc = pr_ld4(dout + c);
  } else {
    const int sy = (q - 1) / sw, sx = (q - 1) - sy * sw;
    if (threadIdx.x == 0) { lim[0] = gh; lim[1] = -1; lim[2] = gw; lim[3] = -1; }
    __syncthreads();
    for (int k = threadIdx.x; k < gh + gw; k += 256) {
      const bool is_y = k < gh;
      const int dst = is_y ? k : k - gh, cell = is_y ? sy : sx;
      int idx[4];
      float w[4];
      pr_taps(dst, is_y ? hscale : wscale, is_y ? sh : sw, idx, w);
      float s = 0.f;
      bool hit = false;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (idx[j] == cell) { s += w[j]; hit = true; }
      (is_y ? wy_tab : wx_tab)[dst] = s;
      if (hit) {
        atomicMin(&lim[is_y ? 0 : 2], dst);
        atomicMax(&lim[is_y ? 1 : 3], dst);
      }
    }
    __syncthreads();
    const int ylo = lim[0], ny = lim[1] - ylo + 1, xlo = lim[2], nx = lim[3] - xlo + 1;
    if (ny > 0 && nx > 0 && c < D) {
      const int pairs = ny * nx;
      for (int k = ry; k < pairs; k += 8) {
        const int yy = k / nx, y = ylo + yy, x = xlo + (k - yy * nx);
        acc = pr_fma(pr_ld4(dout + (1 + (long)y * gw + x) * D + c), wy_tab[y] * wx_tab[x], acc);
      }
    }
  }
  red[ry][cx] = acc;
  __syncthreads();
  if (ry == 0 && c < D) {
    float4 s = red[0][cx];
#pragma unroll
    for (int r = 1; r < 8; ++r) {
      const float4 u = red[r][cx];
      s.x += u.x; s.y += u.y; s.z += u.z; s.w += u.w;
    }
    float4* o = reinterpret_cast<float4*>(dpos + (long)q * D + c);
    if (accumulate) {
      const float4 v = *o;
      s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
    *o = s;
  }
}

inline bool pr_dims_ok(int sh, int sw, int gh, int gw, int D) {
  return sh > 0 && sw > 0 && gh > 0 && gw > 0 && D > 0 && D % 4 == 0;
}
inline bool pr_caps_ok(int sh, int sw, int gh, int gw) {
  return sh <= PR_MAX_SIDE && sw <= PR_MAX_SIDE && gh <= PR_MAX_SIDE && gw <= PR_MAX_SIDE;
}

}  // namespace

extern "C" int mv_pos_resize_fwd(const float* pos, float* out, int sh, int sw, int gh, int gw, int D, mv_stream_t stream) {
  MV_REQUIRE(pr_dims_ok(sh, sw, gh, gw, D), MV_ERR_SHAPE);
  MV_REQUIRE(pr_caps_ok(sh, sw, gh, gw), MV_ERR_UNSUPPORTED);
  MV_REQUIRE(pos && out && mv_aligned16(pos) && mv_aligned16(out), MV_ERR_ALIGN);
  long blocks = (((long)gh * gw + 1) * (D / 4) + 255) / 256;
  if (blocks > 4096) blocks = 4096;              // grid-stride beyond
  return mv_launch<pos_resize_fwd_kernel>(MV_HERE, (int)blocks, 256, 0, (hipStream_t)stream, pos, out, sh, sw, gh, gw, D,
                                          (float)sh / (float)gh, (float)sw / (float)gw);
}

extern "C" int mv_pos_resize_bwd(const float* dout, float* dpos, int accumulate, int sh, int sw, int gh, int gw, int D,
                                 mv_stream_t stream) {
  MV_REQUIRE(pr_dims_ok(sh, sw, gh, gw, D), MV_ERR_SHAPE);
  MV_REQUIRE(pr_caps_ok(sh, sw, gh, gw), MV_ERR_UNSUPPORTED);
  MV_REQUIRE(dout && dpos && mv_aligned16(dout) && mv_aligned16(dpos), MV_ERR_ALIGN);
  const long grid = ((long)sh * sw + 1) * ((D + 127) / 128);
  MV_REQUIRE(grid <= 0x7fffffffL, MV_ERR_UNSUPPORTED);
  return mv_launch<pos_resize_bwd_kernel>(MV_HERE, (int)grid, 256, 0, (hipStream_t)stream, dout, dpos, accumulate, sh, sw, gh, gw,
                                          D, (float)sh / (float)gh, (float)sw / (float)gw);
}
