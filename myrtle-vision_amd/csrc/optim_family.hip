// SGD (plain, momentum, Nesterov) and LAMB over the whole parameter arena on the work list of optim_table.hip (gfx950): items of at most
// 4096 elements that never cross a tensor, a (lr_scale, weight_decay) pair per segment, an optional weight EMA in the same pass.  Each
// kernel is an operation handed to table_walk (optim_walk.h), which owns the item loop, the float4 body, the tail and the EMA line.
// HBM-bound.  SGD: one launch, 5 x 4 B per element with momentum (3 without), + 2 with the EMA.  LAMB: two launches, 10 x 4 B per
// element (phase 1 reads p g m v and writes m v, phase 2 reads p m v and writes p), + 2 with the EMA; between them one pair of
// doubles per ITEM in a workspace, which every workgroup of phase 2 sums again for its item's tensor -- no atomics, no memset, no
// cross-workgroup communication inside a launch, the same bits on every run and for every grid.
#include "optim_walk.h"

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

// Over the arrays p, g, buf, ema.
template <int MODE, bool EMA>
struct sgd_op : table_op {
  static constexpr unsigned STATE = (MODE != SGD_PLAIN ? 0b0100 : 0) | (EMA ? 0b1000 : 0), READS = 0b0011 | STATE, WRITES = 0b0001 | STATE;
  const float *seg_lr_scale, *seg_wd;
  float lr, mu, gscale, d, lr_eff = 0.f, wd = 0.f;
  __device__ __forceinline__ void begin(long, int seg) {
    lr_eff = lr * seg_lr_scale[seg];
    wd = seg_wd[seg];
  }
  __device__ __forceinline__ void one(float (&x)[4]) {
    sgd_table_one<MODE>(x[0], x[2], x[1], gscale, lr_eff, wd, mu);
    if (EMA) table_ema(x[3], x[0], d);
  }
};

template <int MODE, bool EMA>
__global__ __launch_bounds__(256) void sgd_table_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf,
                                                        float* __restrict__ ema, table_list L, const float* __restrict__ hyper, float lr,
                                                        float mu, float gscale, const float* __restrict__ clip_coef, float d) {
  sgd_op<MODE, EMA> op{{}, L.seg_lr_scale, L.seg_wd, table_hyper(hyper, 0, lr), mu, table_gscale(gscale, clip_coef), d};
  float* const arena[4] = {p, const_cast<float*>(g), buf, ema};
  table_walk(arena, L, op);
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

// Phase 1, over the arrays p, g, m, v: m, v <- the new moments; part[2 it], part[2 it + 1] <- sum of p^2, sum of u^2 over item it
// (doubles).  A thread adds its elements in the walk's index order, the workgroup as above: the pair depends on the item's own data
// and length and on nothing else.
struct lamb_moments_op : table_op {
  static constexpr unsigned READS = 0b1111, WRITES = 0b1100;
  const float* seg_wd;
  double* part;
  double (*red)[2];
  float b1, b2, eps, bc1, inv_sqrt_bc2, gscale, wd = 0.f;
  double sp = 0.0, su = 0.0;
  __device__ __forceinline__ void begin(long, int seg) {
    wd = seg_wd[seg];
    sp = su = 0.0;
  }
  __device__ __forceinline__ void one(float (&x)[4]) {
    const float gr = x[1] * gscale;
    x[2] = __builtin_fmaf(1.f - b1, gr, b1 * x[2]);
    x[3] = __builtin_fmaf(gr, (1.f - b2) * gr, b2 * x[3]);
    const double u = (double)lamb_update(x[0], x[2], x[3], wd, bc1, inv_sqrt_bc2, eps), w = (double)x[0];
    sp = __builtin_fma(w, w, sp);
    su = __builtin_fma(u, u, su);
  }
  __device__ __forceinline__ void end(long it) {
    lamb_block_sum2(sp, su, red);
    if (threadIdx.x == 0) {
      part[2 * it] = sp;
      part[2 * it + 1] = su;
    }
  }
};

__global__ __launch_bounds__(256) void lamb_moments_kernel(const float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                           float* __restrict__ v, double* __restrict__ part, table_list L,
                                                           const float* __restrict__ hyper, float b1, float b2, float eps, float bc1,
                                                           float bc2, float gscale, const float* __restrict__ clip_coef) {
  __shared__ double red[4][2];
  lamb_moments_op op{{}, L.seg_wd, part, red, b1, b2, eps, table_hyper(hyper, 1, bc1), rsqrtf(table_hyper(hyper, 2, bc2)),
                     table_gscale(gscale, clip_coef)};
  float* const arena[4] = {const_cast<float*>(p), const_cast<float*>(g), m, v};
  table_walk(arena, L, op);
}

// Phase 2, over the arrays p, m, v, ema.  In the prologue the workgroup sums the pairs of EVERY item of its item's tensor (thread t
// takes items first + t, first + t + 256, ... in that order, then the workgroup sum above), so each item of a tensor arrives at the
// same trust ratio with no word exchanged between workgroups, whatever the grid and whatever else is in the arena.  trust = ||p|| /
// ||u|| where the tensor is decayed and both norms are positive, else 1 (timm's Lamb, always_adapt off, no trust clip);
// p -= lr * lr_scale * trust * u.
template <bool EMA>
struct lamb_apply_op : table_op {
  static constexpr unsigned READS = EMA ? 0b1111 : 0b0111, WRITES = EMA ? 0b1001 : 0b0001;
  const double* part;
  const int32_t *item_tensor, *tensor_range;
  const float *seg_lr_scale, *seg_wd;
  double (*red)[2];
  float lr, eps, bc1, inv_sqrt_bc2, d, wd = 0.f, rate = 0.f;
  __device__ __forceinline__ void begin(long it, int seg) {
    const int t = item_tensor[it], first = tensor_range[2 * t], count = tensor_range[2 * t + 1];
    wd = seg_wd[seg];
    double sp = 0.0, su = 0.0;
    for (int j = threadIdx.x; j < count; j += 256) {
      sp += part[2 * (long)(first + j)];
      su += part[2 * (long)(first + j) + 1];
    }
    lamb_block_sum2(sp, su, red);
    const float trust = (wd != 0.f && sp > 0.0 && su > 0.0) ? (float)(sqrt(sp) / sqrt(su)) : 1.f;
    rate = lr * seg_lr_scale[seg] * trust;
  }
  __device__ __forceinline__ void one(float (&x)[4]) {
    x[0] = __builtin_fmaf(-rate, lamb_update(x[0], x[1], x[2], wd, bc1, inv_sqrt_bc2, eps), x[0]);
    if (EMA) table_ema(x[3], x[0], d);
  }
};

template <bool EMA>
__global__ __launch_bounds__(256) void lamb_apply_kernel(float* __restrict__ p, const float* __restrict__ m, const float* __restrict__ v,
                                                         float* __restrict__ ema, const double* __restrict__ part, table_list L,
                                                         const int32_t* __restrict__ item_tensor,
                                                         const int32_t* __restrict__ tensor_range, const float* __restrict__ hyper,
                                                         float lr, float eps, float bc1, float bc2, float d) {
  __shared__ double red[4][2];
  lamb_apply_op<EMA> op{{}, part, item_tensor, tensor_range, L.seg_lr_scale, L.seg_wd, red, table_hyper(hyper, 0, lr), eps,
                        table_hyper(hyper, 1, bc1), rsqrtf(table_hyper(hyper, 2, bc2)), d};
  float* const arena[4] = {p, const_cast<float*>(m), const_cast<float*>(v), ema};
  table_walk(arena, L, op);
}

}  // namespace

extern "C" int mv_sgd_table(float* p, const float* g, float* buf, float* ema, const int64_t* item_off, const int32_t* item_len,
                            const int32_t* item_seg, long n_items, const float* seg_lr_scale, const float* seg_wd, int n_seg,
                            const float* hyper, float lr, float momentum, int nesterov, float grad_scale, const float* clip_coef,
                            float ema_decay, mv_stream_t stream) {
  const table_list L{item_off, item_len, item_seg, n_items, seg_lr_scale, seg_wd};
  const bool momentum_ok = momentum >= 0.f && momentum < 1.f && !(nesterov && momentum == 0.f);
  if (int rc = table_check(L, n_seg, momentum_ok, ema, ema_decay, {p, g}); rc != MV_OK || n_items == 0) return rc;
  MV_REQUIRE((buf || momentum == 0.f) && mv_aligned16(buf), MV_ERR_ALIGN);
  const int mode = momentum == 0.f ? SGD_PLAIN : nesterov ? SGD_NESTEROV : SGD_MOMENTUM;
  return mv_pick<SGD_PLAIN, SGD_MOMENTUM, SGD_NESTEROV>(mode, [&](auto MODE) {
    return mv_pick<0, 1>(ema != nullptr, [&](auto EMA) {
      constexpr auto K = sgd_table_kernel<decltype(MODE)::value, decltype(EMA)::value != 0>;
      return mv_launch<K>(MV_HERE, table_grid<K>(n_items), 256, 0, (hipStream_t)stream, p, g, buf, ema, L, hyper, lr, momentum,
                          grad_scale, clip_coef, ema ? ema_decay : 0.f);
    });
  });
}

extern "C" size_t mv_lamb_workspace_bytes(long n_items) { return n_items > 0 ? (size_t)n_items * 2 * sizeof(double) : 0; }

extern "C" int mv_lamb_table(float* p, const float* g, float* m, float* v, float* ema, const int64_t* item_off, const int32_t* item_len,
                             const int32_t* item_seg, const int32_t* item_tensor, long n_items, const int32_t* tensor_range,
                             int n_tensors, const float* seg_lr_scale, const float* seg_wd, int n_seg, const float* hyper, float lr,
                             float beta1, float beta2, float eps, float bias_corr1, float bias_corr2, float grad_scale,
                             const float* clip_coef, float ema_decay, void* workspace, size_t workspace_bytes, mv_stream_t stream) {
  const table_list L{item_off, item_len, item_seg, n_items, seg_lr_scale, seg_wd};
  MV_REQUIRE(n_items >= 0 && n_tensors >= 0 && (n_tensors > 0 || n_items == 0), MV_ERR_SHAPE);
  const bool betas_ok = beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f;
  if (int rc = table_check(L, n_seg, betas_ok, ema, ema_decay, {p, g, m, v}); rc != MV_OK || n_items == 0) return rc;
  MV_REQUIRE(item_tensor && tensor_range, MV_ERR_ALIGN);
  MV_REQUIRE(workspace && mv_aligned16(workspace) && workspace_bytes >= mv_lamb_workspace_bytes(n_items), MV_ERR_ALIGN);
  hipStream_t s = (hipStream_t)stream;
  double* part = static_cast<double*>(workspace);
  if (int rc = mv_launch<lamb_moments_kernel>(MV_HERE, table_grid<lamb_moments_kernel>(n_items), 256, 0, s, p, g, m, v, part, L, hyper,
                                              beta1, beta2, eps, bias_corr1, bias_corr2, grad_scale, clip_coef))
    return rc;
  return mv_pick<0, 1>(ema != nullptr, [&](auto EMA) {
    constexpr auto K = lamb_apply_kernel<decltype(EMA)::value != 0>;
    return mv_launch<K>(MV_HERE, table_grid<K>(n_items), 256, 0, s, p, m, v, ema, part, L, item_tensor, tensor_range, hyper, lr, eps,
                        bias_corr1, bias_corr2, ema ? ema_decay : 0.f);
  });
}
