// AdamW over the whole parameter arena in ONE launch, with a learning-rate scale and a weight decay per tensor and an optional
// weight EMA (gfx950).  HBM-bound like adamw_kernel (elementwise.hip): 7 x 4 B per element, 9 x 4 B with the EMA.  The work list, the
// EMA line, the grid and the argument checks are those of optim_walk.h, shared with optim_family.hip; see the note at the kernel.
#include "optim_walk.h"

namespace {

// The update of adamw_kernel (elementwise.hip), expression for expression:
//   gr = g * gscale;  p *= 1 - lr * wd;  m = b1 * m + (1 - b1) * gr;  v = b2 * v + (1 - b2) * gr * gr;
//   p -= step * m / (sqrtf(v) * inv_sqrt_bc2 + eps)
// with every fused multiply-add SPELLED OUT, the ones the compiler's contraction makes of those expressions on adamw_kernel's
// float4 path (the only path an arena region takes there: its length is a multiple of 8).  Left to the compiler, which sums
// fuse depends on the code around them -- adamw_kernel's own scalar tail fuses fewer than its float4 body -- and the float4
// body and the tail of one item would round differently.  Spelled out, both paths here and that float4 path write the same
// bits: with lr_scale 1 and the same wd the two kernels agree bit for bit (tests/test_optim_table_gpu.py holds them to that).
__device__ __forceinline__ void adamw_table_one(float& P, float& M, float& V, float G, float gscale, float lr, float wd, float b1,
                                                float b2, float eps, float step, float inv_sqrt_bc2) {
  const float gr = G * gscale;
  const float keep = __builtin_fmaf(-lr, wd, 1.f);                              // 1 - lr * wd
  M = __builtin_fmaf(1.f - b1, gr, b1 * M);
  V = __builtin_fmaf(gr, (1.f - b2) * gr, b2 * V);
  const float q = step * M / __builtin_fmaf(inv_sqrt_bc2, sqrtf(V), eps);
  P = __builtin_fmaf(keep, P, -q);                                              // p * (1 - lr * wd) - q
}

// This kernel keeps its own copy of table_walk's frame (optim_walk.h) -- the item loop, the float4 body, the tail -- because it is the
// one kernel of the work list whose speed the walk did not keep: through table_walk the launch with the EMA measured 0.2 to 0.4 %
// slower in the median than this form, above the slowest run of this form (profiles/optim_walk.txt).  Written out, its machine code
// is digest for digest what it was before the walk existed.  The EMA line, the grid and the argument checks are the shared ones.
template <bool EMA>
__global__ __launch_bounds__(256) void adamw_table_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                          float* __restrict__ v, float* __restrict__ ema,
                                                          const int64_t* __restrict__ item_off, const int32_t* __restrict__ item_len,
                                                          const int32_t* __restrict__ item_seg, long n_items,
                                                          const float* __restrict__ seg_lr_scale, const float* __restrict__ seg_wd,
                                                          const float* __restrict__ hyper, float lr, float b1, float b2, float eps,
                                                          float bc1, float bc2, float gscale, const float* __restrict__ clip_coef,
                                                          float d) {
  if (hyper) {                                // the per-step scalars live on the device (captured launches stay valid)
    lr = hyper[0];
    bc1 = hyper[1];
    bc2 = hyper[2];
  }
  if (clip_coef) gscale *= clip_coef[0];      // clip_grad_norm_'s min(1, max_norm / (norm + 1e-6)), computed on the device
  const float inv_sqrt_bc2 = rsqrtf(bc2);
  for (long it = blockIdx.x; it < n_items; it += gridDim.x) {
    const long off = item_off[it];
    const int len = item_len[it], seg = item_seg[it];
    const float lr_eff = lr * seg_lr_scale[seg], wd = seg_wd[seg];
    const float step = lr_eff / bc1;
    float* __restrict__ ip = p + off;
    const float* __restrict__ ig = g + off;
    float* __restrict__ im = m + off;
    float* __restrict__ iv = v + off;
    float* __restrict__ ie = EMA ? ema + off : nullptr;
    const int n4 = len >> 2;
    for (int i = threadIdx.x; i < n4; i += 256) {
      float4 P = reinterpret_cast<float4*>(ip)[i], M = reinterpret_cast<float4*>(im)[i], V = reinterpret_cast<float4*>(iv)[i];
      const float4 G = reinterpret_cast<const float4*>(ig)[i];
      float4 E = {};
      if (EMA) E = reinterpret_cast<float4*>(ie)[i];
      float* pp = &P.x; float* mm = &M.x; float* vv = &V.x; const float* gg = &G.x; float* ee = &E.x;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        adamw_table_one(pp[e], mm[e], vv[e], gg[e], gscale, lr_eff, wd, b1, b2, eps, step, inv_sqrt_bc2);
        if (EMA) table_ema(ee[e], pp[e], d);
      }
      reinterpret_cast<float4*>(ip)[i] = P;
      reinterpret_cast<float4*>(im)[i] = M;
      reinterpret_cast<float4*>(iv)[i] = V;
      if (EMA) reinterpret_cast<float4*>(ie)[i] = E;
    }
    const int i = (n4 << 2) + threadIdx.x;    // at most 3 tail elements
    if (i < len) {
      float P = ip[i], M = im[i], V = iv[i];
      adamw_table_one(P, M, V, ig[i], gscale, lr_eff, wd, b1, b2, eps, step, inv_sqrt_bc2);
      ip[i] = P; im[i] = M; iv[i] = V;
      if (EMA) table_ema(ie[i], P, d);
    }
  }
}

}  // namespace

extern "C" int mv_adamw_table(float* p, const float* g, float* m, float* v, float* ema, const int64_t* item_off,
                              const int32_t* item_len, const int32_t* item_seg, long n_items, const float* seg_lr_scale,
                              const float* seg_wd, int n_seg, const float* hyper, float lr, float beta1, float beta2, float eps,
                              float bias_corr1, float bias_corr2, float grad_scale, const float* clip_coef, float ema_decay,
                              mv_stream_t stream) {
  const table_list L{item_off, item_len, item_seg, n_items, seg_lr_scale, seg_wd};
  const bool betas_ok = beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f;
  if (int rc = table_check(L, n_seg, betas_ok, ema, ema_decay, {p, g, m, v}); rc != MV_OK || n_items == 0) return rc;
  return mv_pick<0, 1>(ema != nullptr, [&](auto EMA) {
    constexpr auto K = adamw_table_kernel<decltype(EMA)::value != 0>;
    return mv_launch<K>(MV_HERE, table_grid<K>(n_items), 256, 0, (hipStream_t)stream, p, g, m, v, ema, item_off, item_len, item_seg, n_items,
                        seg_lr_scale, seg_wd, hyper, lr, beta1, beta2, eps, bias_corr1, bias_corr2, grad_scale, clip_coef,
                        ema ? ema_decay : 0.f);
  });
}
