// SGD (plain, momentum, Nesterov) and LAMB over the whole parameter arena on the work list of optim_table.hip (gfx950): items of at most
// 4096 elements that never cross a tensor, a (lr_scale, weight_decay) pair per segment, an optional weight EMA in the same pass.
// HBM-bound.  SGD: one launch, 5 x 4 B per element with momentum (3 without), + 2 with the EMA.  LAMB: two launches, 10 x 4 B per
// element (phase 1 reads p g m v and writes m v, phase 2 reads p m v and writes p), + 2 with the EMA; between them one pair of
// doubles per ITEM in a workspace, which every workgroup of phase 2 sums again for its item's tensor -- no atomics, no memset, no
// cross-workgroup communication inside a launch, the same bits on every run and for every grid.
#include "mv_common.h"

namespace {

// ---- SGD -------------------------------------------------------------------------------------------------------------------------
// torch.optim.SGD with dampening 0:  d = gr + wd * p;  buf = mu * buf + d;  d = nesterov ? d + mu * buf : buf;  p -= lr * d.
// A zero buffer makes the first step buf = d, torch's first step.  Every fused multiply-add is SPELLED OUT, as in adamw_table_one
// (optim_table.hip), so that the float4 body and the tail of an item round alike.  MODE 0: no momentum (no buffer is read or written).
enum { SGD_PLAIN = 0, SGD_MOMENTUM = 1, SGD_NESTEROV = 2 };

template <int MODE>
__device__ __forceinline__ void sgd_table_one(float& P, float& B, float G, float gscale, float lr, float wd, float mu) {
  const float gr = G * gscale;
  float d = __builtin_fmaf(wd, P, gr);
  if (MODE != SGD_PLAIN) {
    B = __builtin_fmaf(mu, B, d);
    d = MODE == SGD_NESTEROV ? __builtin_fmaf(mu, B, d) : B;
  }
  P = __builtin_fmaf(-lr, d, P);
}

template <int MODE, bool EMA>
__global__ __launch_bounds__(256) void sgd_table_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf,
                                                        float* __restrict__ ema, const int64_t* __restrict__ item_off,
                                                        const int32_t* __restrict__ item_len, const int32_t* __restrict__ item_seg,
                                                        long n_items, const float* __restrict__ seg_lr_scale,
                                                        const float* __restrict__ seg_wd, const float* __restrict__ hyper, float lr,
                                                        float mu, float gscale, const float* __restrict__ clip_coef, float d) {
  if (hyper) lr = hyper[0];                   // the scheduled rate lives on the device (captured launches stay valid)
  if (clip_coef) gscale *= clip_coef[0];
  for (long it = blockIdx.x; it < n_items; it += gridDim.x) {
    const long off = item_off[it];
    const int len = item_len[it], seg = item_seg[it];
    const float lr_eff = lr * seg_lr_scale[seg], wd = seg_wd[seg];
    float* __restrict__ ip = p + off;
    const float* __restrict__ ig = g + off;
    float* __restrict__ ib = MODE != SGD_PLAIN ? buf + off : nullptr;
    float* __restrict__ ie = EMA ? ema + off : nullptr;
    const int n4 = len >> 2;
    for (int i = threadIdx.x; i < n4; i += 256) {
      float4 P = reinterpret_cast<float4*>(ip)[i];
      const float4 G = reinterpret_cast<const float4*>(ig)[i];
      float4 B = {}, E = {};
      if (MODE != SGD_PLAIN) B = reinterpret_cast<float4*>(ib)[i];
      if (EMA) E = reinterpret_cast<float4*>(ie)[i];
      float* pp = &P.x; float* bb = &B.x; const float* gg = &G.x; float* ee = &E.x;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        sgd_table_one<MODE>(pp[e], bb[e], gg[e], gscale, lr_eff, wd, mu);
        if (EMA) ee[e] = __builtin_fmaf(d, ee[e], (1.f - d) * pp[e]);
      }
      reinterpret_cast<float4*>(ip)[i] = P;
      if (MODE != SGD_PLAIN) reinterpret_cast<float4*>(ib)[i] = B;
      if (EMA) reinterpret_cast<float4*>(ie)[i] = E;
    }
    const int i = (n4 << 2) + threadIdx.x;    // at most 3 tail elements
    if (i < len) {
      float P = ip[i], B = MODE != SGD_PLAIN ? ib[i] : 0.f;
      sgd_table_one<MODE>(P, B, ig[i], gscale, lr_eff, wd, mu);
      ip[i] = P;
      if (MODE != SGD_PLAIN) ib[i] = B;
      if (EMA) ie[i] = __builtin_fmaf(d, ie[i], (1.f - d) * P);
    }
  }
}

// ---- LAMB ------------------------------------------------------------------------------------------------------------------------
// The moments of adamw_table_one, and the update u = (m / bc1) / (sqrt(v) / sqrt(bc2) + eps) + wd * p.  Phase 2 calls lamb_update
// again on the new m, v and the still-unchanged p: one definition, explicit fused operations, the same bits in both launches.
__device__ __forceinline__ float lamb_update(float P, float M, float V, float wd, float bc1, float inv_sqrt_bc2, float eps) {
  const float r = (M / bc1) / __builtin_fmaf(inv_sqrt_bc2, sqrtf(V), eps);
  return __builtin_fmaf(wd, P, r);
}

// Both sums over the 256 threads of the workgroup, in a fixed order, every thread ending with the same bits: a butterfly inside each
// wave (a + b == b + a, so all 64 lanes agree at every level), then the four waves' values through LDS, added 0, 1, 2, 3.
__device__ __forceinline__ void lamb_block_sum2(double& a, double& b, double (*red)[2]) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    a += __shfl_xor(a, o, 64);
    b += __shfl_xor(b, o, 64);
  }
  __syncthreads();                            // the previous item's readers are done with red
  if ((threadIdx.x & 63) == 0) {
    red[threadIdx.x >> 6][0] = a;
    red[threadIdx.x >> 6][1] = b;
  }
  __syncthreads();
  a = ((red[0][0] + red[1][0]) + red[2][0]) + red[3][0];
  b = ((red[0][1] + red[1][1]) + red[2][1]) + red[3][1];
}

// Phase 1: m, v <- the new moments; part[2 it], part[2 it + 1] <- sum of p^2, sum of u^2 over item it (doubles).  A thread adds its
// elements in index order (float4 i = tid, tid + 256, ..., then its tail element), the workgroup as above: the pair depends on the
// item's own data and length and on nothing else.
__global__ __launch_bounds__(256) void lamb_moments_kernel(const float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                           float* __restrict__ v, double* __restrict__ part,
                                                           const int64_t* __restrict__ item_off, const int32_t* __restrict__ item_len,
                                                           const int32_t* __restrict__ item_seg, long n_items,
                                                           const float* __restrict__ seg_wd, const float* __restrict__ hyper, float b1,
                                                           float b2, float eps, float bc1, float bc2, float gscale,
                                                           const float* __restrict__ clip_coef) {
  __shared__ double red[4][2];
  if (hyper) {
    bc1 = hyper[1];
    bc2 = hyper[2];
  }
  if (clip_coef) gscale *= clip_coef[0];
  const float inv_sqrt_bc2 = rsqrtf(bc2);
  for (long it = blockIdx.x; it < n_items; it += gridDim.x) {
    const long off = item_off[it];
    const int len = item_len[it];
    const float wd = seg_wd[item_seg[it]];
    const float* __restrict__ ip = p + off;
    const float* __restrict__ ig = g + off;
    float* __restrict__ im = m + off;
    float* __restrict__ iv = v + off;
    double sp = 0.0, su = 0.0;
    const int n4 = len >> 2;
    for (int i = threadIdx.x; i < n4; i += 256) {
      const float4 P = reinterpret_cast<const float4*>(ip)[i], G = reinterpret_cast<const float4*>(ig)[i];
      float4 M = reinterpret_cast<float4*>(im)[i], V = reinterpret_cast<float4*>(iv)[i];
      const float* pp = &P.x; const float* gg = &G.x; float* mm = &M.x; float* vv = &V.x;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float gr = gg[e] * gscale;
        mm[e] = __builtin_fmaf(1.f - b1, gr, b1 * mm[e]);
        vv[e] = __builtin_fmaf(gr, (1.f - b2) * gr, b2 * vv[e]);
        const double u = (double)lamb_update(pp[e], mm[e], vv[e], wd, bc1, inv_sqrt_bc2, eps), w = (double)pp[e];
        sp = __builtin_fma(w, w, sp);
        su = __builtin_fma(u, u, su);
      }
      reinterpret_cast<float4*>(im)[i] = M;
      reinterpret_cast<float4*>(iv)[i] = V;
    }
    const int i = (n4 << 2) + threadIdx.x;    // at most 3 tail elements
    if (i < len) {
      const float P = ip[i], gr = ig[i] * gscale;
      const float M = __builtin_fmaf(1.f - b1, gr, b1 * im[i]);
      const float V = __builtin_fmaf(gr, (1.f - b2) * gr, b2 * iv[i]);
      im[i] = M;
      iv[i] = V;
      const double u = (double)lamb_update(P, M, V, wd, bc1, inv_sqrt_bc2, eps), w = (double)P;
      sp = __builtin_fma(w, w, sp);
      su = __builtin_fma(u, u, su);
    }
    lamb_block_sum2(sp, su, red);
    if (threadIdx.x == 0) {
      part[2 * it] = sp;
      part[2 * it + 1] = su;
    }
  }
}

// Phase 2, per item again: the workgroup sums the pairs of EVERY item of its item's tensor (thread t takes items first + t, first + t +
// 256, ... in that order, then the workgroup sum above), so each item of a tensor arrives at the same trust ratio with no word
// exchanged between workgroups, whatever the grid and whatever else is in the arena.  trust = ||p|| / ||u|| where the tensor is
// decayed and both norms are positive, else 1 (timm's Lamb, always_adapt off, no trust clip); p -= lr * lr_scale * trust * u.
template <bool EMA>
__global__ __launch_bounds__(256) void lamb_apply_kernel(float* __restrict__ p, const float* __restrict__ m, const float* __restrict__ v,
                                                         float* __restrict__ ema, const double* __restrict__ part,
                                                         const int64_t* __restrict__ item_off, const int32_t* __restrict__ item_len,
                                                         const int32_t* __restrict__ item_seg, const int32_t* __restrict__ item_tensor,
                                                         long n_items, const int32_t* __restrict__ tensor_range,
                                                         const float* __restrict__ seg_lr_scale, const float* __restrict__ seg_wd,
                                                         const float* __restrict__ hyper, float lr, float eps, float bc1, float bc2,
                                                         float d) {
  __shared__ double red[4][2];
  if (hyper) {
    lr = hyper[0];
    bc1 = hyper[1];
    bc2 = hyper[2];
  }
  const float inv_sqrt_bc2 = rsqrtf(bc2);
  for (long it = blockIdx.x; it < n_items; it += gridDim.x) {
    const long off = item_off[it];
    const int len = item_len[it], seg = item_seg[it], t = item_tensor[it];
    const int first = tensor_range[2 * t], count = tensor_range[2 * t + 1];
    const float wd = seg_wd[seg];
    double sp = 0.0, su = 0.0;
    for (int j = threadIdx.x; j < count; j += 256) {
      sp += part[2 * (long)(first + j)];
      su += part[2 * (long)(first + j) + 1];
    }
    lamb_block_sum2(sp, su, red);
    const float trust = (wd != 0.f && sp > 0.0 && su > 0.0) ? (float)(sqrt(sp) / sqrt(su)) : 1.f;
    const float rate = lr * seg_lr_scale[seg] * trust;
    float* __restrict__ ip = p + off;
    const float* __restrict__ im = m + off;
    const float* __restrict__ iv = v + off;
    float* __restrict__ ie = EMA ? ema + off : nullptr;
    const int n4 = len >> 2;
    for (int i = threadIdx.x; i < n4; i += 256) {
      float4 P = reinterpret_cast<float4*>(ip)[i];
      const float4 M = reinterpret_cast<const float4*>(im)[i], V = reinterpret_cast<const float4*>(iv)[i];
      float4 E = {};
      if (EMA) E = reinterpret_cast<float4*>(ie)[i];
      float* pp = &P.x; const float* mm = &M.x; const float* vv = &V.x; float* ee = &E.x;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        pp[e] = __builtin_fmaf(-rate, lamb_update(pp[e], mm[e], vv[e], wd, bc1, inv_sqrt_bc2, eps), pp[e]);
        if (EMA) ee[e] = __builtin_fmaf(d, ee[e], (1.f - d) * pp[e]);
      }
      reinterpret_cast<float4*>(ip)[i] = P;
      if (EMA) reinterpret_cast<float4*>(ie)[i] = E;
    }
    const int i = (n4 << 2) + threadIdx.x;    // at most 3 tail elements
    if (i < len) {
      const float P = __builtin_fmaf(-rate, lamb_update(ip[i], im[i], iv[i], wd, bc1, inv_sqrt_bc2, eps), ip[i]);
      ip[i] = P;
      if (EMA) ie[i] = __builtin_fmaf(d, ie[i], (1.f - d) * P);
    }
  }
}

template <auto K>
int family_grid(long n_items) {
  const long resident = mv_resident_blocks<K>(256, 0);
  return (int)(n_items < resident ? n_items : resident);
}

}  // namespace

extern "C" int mv_sgd_table(float* p, const float* g, float* buf, float* ema, const int64_t* item_off, const int32_t* item_len,
                            const int32_t* item_seg, long n_items, const float* seg_lr_scale, const float* seg_wd, int n_seg,
                            const float* hyper, float lr, float momentum, int nesterov, float grad_scale, const float* clip_coef,
                            float ema_decay, mv_stream_t stream) {
  MV_REQUIRE(n_items >= 0 && n_seg > 0, MV_ERR_SHAPE);
  MV_REQUIRE(momentum >= 0.f && momentum < 1.f && !(nesterov && momentum == 0.f), MV_ERR_UNSUPPORTED);   // a NaN fails every comparison
  MV_REQUIRE(ema == nullptr || (ema_decay >= 0.f && ema_decay < 1.f), MV_ERR_UNSUPPORTED);
  if (n_items == 0) return MV_OK;
  MV_REQUIRE(p && g && (buf || momentum == 0.f) && mv_aligned16(p) && mv_aligned16(g) && mv_aligned16(buf) && mv_aligned16(ema),
             MV_ERR_ALIGN);
  MV_REQUIRE(item_off && item_len && item_seg && seg_lr_scale && seg_wd, MV_ERR_ALIGN);
  const int mode = momentum == 0.f ? SGD_PLAIN : nesterov ? SGD_NESTEROV : SGD_MOMENTUM;
  return mv_pick<SGD_PLAIN, SGD_MOMENTUM, SGD_NESTEROV>(mode, [&](auto MODE) {
    return mv_pick<0, 1>(ema != nullptr, [&](auto EMA) {
      constexpr auto K = sgd_table_kernel<decltype(MODE)::value, decltype(EMA)::value != 0>;
      return mv_launch<K>(MV_HERE, family_grid<K>(n_items), 256, 0, (hipStream_t)stream, p, g, buf, ema, item_off, item_len, item_seg,
                          n_items, seg_lr_scale, seg_wd, hyper, lr, momentum, grad_scale, clip_coef, ema ? ema_decay : 0.f);
    });
  });
}

extern "C" size_t mv_lamb_workspace_bytes(long n_items) { return n_items > 0 ? (size_t)n_items * 2 * sizeof(double) : 0; }

extern "C" int mv_lamb_table(float* p, const float* g, float* m, float* v, float* ema, const int64_t* item_off, const int32_t* item_len,
                             const int32_t* item_seg, const int32_t* item_tensor, long n_items, const int32_t* tensor_range,
                             int n_tensors, const float* seg_lr_scale, const float* seg_wd, int n_seg, const float* hyper, float lr,
                             float beta1, float beta2, float eps, float bias_corr1, float bias_corr2, float grad_scale,
                             const float* clip_coef, float ema_decay, void* workspace, size_t workspace_bytes, mv_stream_t stream) {
  MV_REQUIRE(n_items >= 0 && n_seg > 0 && n_tensors >= 0 && (n_tensors > 0 || n_items == 0), MV_ERR_SHAPE);
  MV_REQUIRE(beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f, MV_ERR_UNSUPPORTED);      // a NaN fails every comparison
  MV_REQUIRE(ema == nullptr || (ema_decay >= 0.f && ema_decay < 1.f), MV_ERR_UNSUPPORTED);
  if (n_items == 0) return MV_OK;
  MV_REQUIRE(p && g && m && v && mv_aligned16(p) && mv_aligned16(g) && mv_aligned16(m) && mv_aligned16(v) && mv_aligned16(ema),
             MV_ERR_ALIGN);
  MV_REQUIRE(item_off && item_len && item_seg && item_tensor && tensor_range && seg_lr_scale && seg_wd, MV_ERR_ALIGN);
  MV_REQUIRE(workspace && mv_aligned16(workspace) && workspace_bytes >= mv_lamb_workspace_bytes(n_items), MV_ERR_ALIGN);
  hipStream_t s = (hipStream_t)stream;
  double* part = static_cast<double*>(workspace);
  if (int rc = mv_launch<lamb_moments_kernel>(MV_HERE, family_grid<lamb_moments_kernel>(n_items), 256, 0, s, p, g, m, v, part, item_off,
                                              item_len, item_seg, n_items, seg_wd, hyper, beta1, beta2, eps, bias_corr1, bias_corr2,
                                              grad_scale, clip_coef))
    return rc;
  return mv_pick<0, 1>(ema != nullptr, [&](auto EMA) {
    constexpr auto K = lamb_apply_kernel<decltype(EMA)::value != 0>;
    return mv_launch<K>(MV_HERE, family_grid<K>(n_items), 256, 0, s, p, m, v, ema, part, item_off, item_len, item_seg, item_tensor,
                        n_items, tensor_range, seg_lr_scale, seg_wd, hyper, lr, eps, bias_corr1, bias_corr2, ema ? ema_decay : 0.f);
  });
}
