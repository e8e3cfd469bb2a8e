// Label smoothing, Mixup and CutMix for classification (gfx950): the soft-target cross entropy and the in-place batch mixing.
//
// Both follow timm's batch-mode Mixup: sample i of a batch of B is paired with j = B - 1 - i (x.flip(0)), the target is
// t_i = lam * s(y_i) + (1 - lam) * s(y_j) with s(y) = eps / C everywhere plus (1 - eps) at class y.  The [B, C] target is never
// built: the loss needs the two logits at y_i and y_j and the plain sum of the row, the gradient adds the same three terms back.
// lam and the CutMix box are host scalars (launch arguments): nothing here reads them from the device or copies anything back.
#include "mv_common.h"

namespace {

// One wave per sample, classes strided over the lanes.  Three passes over the row (max / arg-max / class sum, sum of
// exponentials, gradient); a row of 32 768 classes is 128 KiB and stays in L2 between them.  The per-sample loss goes to
// sample_loss[i]; ce_soft_mean_kernel sums those in a fixed order, so no floating-point atomic is involved anywhere.
__global__ __launch_bounds__(256) void ce_soft_kernel(const float* __restrict__ logits, const int64_t* __restrict__ labels,
                                                      float* __restrict__ sample_loss, float* __restrict__ dlogits,
                                                      int64_t* __restrict__ argmax, int B, int C, float lam, float eps,
                                                      int pair_flip, float gscale) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float oml = 1.0f - lam, on = 1.0f - eps, off = eps / (float)C;
  const float w = gscale / (float)B;
  for (int smp = blockIdx.x * 4 + wave; smp < B; smp += gridDim.x * 4) {
    const float* lp = logits + (long)smp * C;
    float mx = -INFINITY, zs = 0.f;
    int am = 0;
    for (int c = lane; c < C; c += 64) {
      const float v = lp[c];
      zs += v;
      if (v > mx) { mx = v; am = c; }
    }
    // wave arg-max, first index wins on ties (torch.argmax semantics, as cross_entropy_kernel)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float om = __shfl_xor(mx, o, 64);
      const int oa = __shfl_xor(am, o, 64);
      if (om > mx || (om == mx && oa < am)) { mx = om; am = oa; }
    }
    zs = wave_sum(zs);
    float s = 0.f;
    for (int c = lane; c < C; c += 64) s += expf(lp[c] - mx);
    s = wave_sum(s);
    const int64_t yi = labels[smp], yj = pair_flip ? labels[B - 1 - smp] : yi;
    const bool valid = yi >= 0 && yi < C && yj >= 0 && yj < C;      // a label outside [0, C) is never used as an index
    const int a = valid ? (int)yi : 0, b = valid ? (int)yj : 0;      // an index inside the row either way
    if (lane == 0) {
      const float lse = mx + logf(s);
      sample_loss[smp] = valid ? lse - on * (lam * lp[a] + oml * lp[b]) - off * zs : __builtin_nanf("");
      if (argmax) argmax[smp] = am;
    }
    if (dlogits) {
      float* dp = dlogits + (long)smp * C;
      for (int c = lane; c < C; c += 64) {
        const float t = off + on * ((c == a ? lam : 0.f) + (c == b ? oml : 0.f));
        dp[c] = valid ? (expf(lp[c] - mx) / s - t) * w : 0.f;       // a poisoned row carries no gradient (mv_cross_entropy)
      }
    }
  }
}

// loss[0] = (sum of sample_loss[0 .. B)) / B by ONE wave: lane l adds rows l, l + 64, ... in order, then the wave butterfly.  The
// order depends on B alone, so the same inputs give the same bits every run; a NaN row makes the mean NaN.
__global__ __launch_bounds__(64) void ce_soft_mean_kernel(const float* __restrict__ sample_loss, float* __restrict__ loss, int B) {
  float s = 0.f;
  for (int i = threadIdx.x; i < B; i += 64) s += sample_loss[i];
  s = wave_sum(s);
  if (threadIdx.x == 0) loss[0] = s / (float)B;
}

// ---- batch mixing -----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float mix_f(unsigned bits) { return __uint_as_float(bits); }
__device__ __forceinline__ float mix_f(unsigned short bits) { return __uint_as_float((unsigned)bits << 16); }
__device__ __forceinline__ void mix_store(unsigned* p, float v) { *p = __float_as_uint(v); }
__device__ __forceinline__ void mix_store(unsigned short* p, float v) {
  const bf16_t h = (bf16_t)v;                    // round to nearest even, once
  *p = *reinterpret_cast<const unsigned short*>(&h);
}

// both new values of one element pair, from both old ones
template <typename U>
__device__ __forceinline__ void mix_pair(U* pa, U* pb, float lam, float oml) {
  const float a = mix_f(*pa), b = mix_f(*pb);
  mix_store(pa, lam * a + oml * b);
  mix_store(pb, lam * b + oml * a);
}

// Mixup, in place: block (chunk, pair p) mixes samples p and B - 1 - p over their flat extent of n elements.  A thread reads the
// SAME element (or 16-byte group) of both samples and then writes both, and no other thread touches either: that is what makes in
// place correct.  The 16-byte body needs both samples at the same offset from a 16-byte boundary (always so when n * sizeof(U)
// is a multiple of 16); the elements in front of the first boundary and behind the last whole group go one by one, and a pair whose
// samples sit at different offsets goes one by one altogether.  U: the element's bit pattern (unsigned: fp32, unsigned short: bf16).
template <typename U>
__global__ __launch_bounds__(256) void mixup_kernel(U* __restrict__ x, int B, long n, float lam) {
  constexpr int VE = 16 / (int)sizeof(U);
  const float oml = 1.0f - lam;
  const int p = blockIdx.y;
  U* pa = x + (long)p * n;
  U* pb = x + (long)(B - 1 - p) * n;
  const int ma = (int)((reinterpret_cast<uintptr_t>(pa) & 15u) / sizeof(U)), mb = (int)((reinterpret_cast<uintptr_t>(pb) & 15u) / sizeof(U));
  long head = n;                                 // block-uniform
  if (ma == mb) head = ma ? (long)(VE - ma) : 0;
  if (head > n) head = n;
  const long nv = (n - head) / VE, rest = n - nv * VE;        // rest = head + tail
  const long t0 = blockIdx.x * 256L + threadIdx.x, step = gridDim.x * 256L;
  for (long v = t0; v < nv; v += step) {
    u32x4* qa = reinterpret_cast<u32x4*>(pa + head + v * VE);
    u32x4* qb = reinterpret_cast<u32x4*>(pb + head + v * VE);
    u32x4 ra = *qa, rb = *qb;
    U* ea = reinterpret_cast<U*>(&ra);
    U* eb = reinterpret_cast<U*>(&rb);
#pragma unroll
    for (int k = 0; k < VE; ++k) mix_pair(ea + k, eb + k, lam, oml);
    *qa = ra;
    *qb = rb;
  }
  for (long k = t0; k < rest; k += step) {
    const long e = k < head ? k : k + nv * VE;
    mix_pair(pa + e, pb + e, lam, oml);
  }
}

// CutMix, in place: one wave per (pair, channel, box row) swaps the bits of columns [x0, x1) between the two samples.  Only the box
// is read or written.  grid.x covers the Ch * (y1 - y0) rows four to a block, grid.y the pairs.
template <typename U>
__global__ __launch_bounds__(256) void cutmix_kernel(U* __restrict__ x, int B, int Ch, int H, int W, int y0, int y1, int x0, int x1) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int bh = y1 - y0;
  const long row = blockIdx.x * 4L + wave;
  if (row >= (long)Ch * bh) return;
  const int c = (int)(row / bh), y = y0 + (int)(row - (long)c * bh);
  const long n = (long)Ch * H * W, at = ((long)c * H + y) * W;
  U* pa = x + (long)blockIdx.y * n + at;
  U* pb = x + (long)(B - 1 - (int)blockIdx.y) * n + at;
  for (int col = x0 + lane; col < x1; col += 64) {
    const U a = pa[col], b = pb[col];
    pa[col] = b;
    pb[col] = a;
  }
}

}  // namespace

extern "C" int mv_cross_entropy_soft(const float* logits, const int64_t* labels, float* loss, float* sample_loss, float* dlogits,
                                     int64_t* argmax, int B, int C, float lam, float eps, int pair_flip, float grad_scale,
                                     mv_stream_t stream) {
  MV_REQUIRE(B >= 0 && C >= 2, MV_ERR_SHAPE);
  MV_REQUIRE(eps >= 0.f && eps < 1.f && lam >= 0.f && lam <= 1.f, MV_ERR_UNSUPPORTED);     // a NaN fails both
  MV_REQUIRE(pair_flip != 0 || lam == 1.f, MV_ERR_UNSUPPORTED);                            // no partner: nothing to blend with
  if (B == 0) return MV_OK;                      // an empty batch has no storage: its pointers may be null
  MV_REQUIRE(logits && labels && loss && sample_loss, MV_ERR_ALIGN);
  hipStream_t s = (hipStream_t)stream;
  int blocks = mv_cdiv(B, 4);
  if (blocks > 4096) blocks = 4096;              // grid-stride beyond
  if (int rc = mv_launch<ce_soft_kernel>(MV_HERE, blocks, 256, 0, s, logits, labels, sample_loss, dlogits, argmax, B, C, lam, eps,
                                         pair_flip, grad_scale))
    return rc;
  return mv_launch<ce_soft_mean_kernel>(MV_HERE, 1, 64, 0, s, (const float*)sample_loss, loss, B);
}

extern "C" int mv_mix_batch(void* x, int elem, int B, int Ch, int H, int W, int mode, float lam, int y0, int y1, int x0, int x1,
                            mv_stream_t stream) {
  MV_REQUIRE(B >= 0 && Ch > 0 && H > 0 && W > 0, MV_ERR_SHAPE);
  MV_REQUIRE(elem == MV_F32 || elem == MV_BF16, MV_ERR_UNSUPPORTED);
  MV_REQUIRE(mode == 0 || mode == 1, MV_ERR_UNSUPPORTED);
  MV_REQUIRE(x && mv_aligned16(x), MV_ERR_ALIGN);
  if (mode == 0) MV_REQUIRE(lam >= 0.f && lam <= 1.f, MV_ERR_UNSUPPORTED);
  else MV_REQUIRE(0 <= y0 && y0 <= y1 && y1 <= H && 0 <= x0 && x0 <= x1 && x1 <= W, MV_ERR_SHAPE);
  const long n = (long)Ch * H * W;
  const int pairs = B / 2;                       // odd B: the middle sample is its own partner and stays as it is
  MV_REQUIRE(pairs <= 65535 && n <= 0x7fffffffL, MV_ERR_UNSUPPORTED);       // grid.y; the rows of one sample index grid.x
  if (pairs == 0) return MV_OK;
  hipStream_t s = (hipStream_t)stream;
  if (mode == 0) {
    if (lam == 1.f) return MV_OK;                // x_i' = x_i: nothing to write
    return mv_pick<MV_F32, MV_BF16>(elem, [&](auto D) {
      using U = std::conditional_t<D() == MV_F32, unsigned, unsigned short>;
      long blocks = (n / (16 / (long)sizeof(U)) + 255) / 256 + 1;                            // + 1: head and tail elements
      if (blocks > 1024) blocks = 1024;          // grid-stride beyond
      return mv_launch<mixup_kernel<U>>(MV_HERE, dim3((unsigned)blocks, (unsigned)pairs), 256, 0, s, (U*)x, B, n, lam);
    });
  }
  if (y0 == y1 || x0 == x1) return MV_OK;        // empty box
  const long rows = (long)Ch * (y1 - y0);
  return mv_pick<MV_F32, MV_BF16>(elem, [&](auto D) {
    using U = std::conditional_t<D() == MV_F32, unsigned, unsigned short>;
    return mv_launch<cutmix_kernel<U>>(MV_HERE, dim3((unsigned)mv_cdiv(rows, 4), (unsigned)pairs), 256, 0, s, (U*)x, B, Ch, H, W, y0, y1,
                                       x0, x1);
  });
}
