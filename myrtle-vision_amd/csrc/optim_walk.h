// The walk over the optimizer work list: every kernel of optim_family.hip is an operation handed to table_walk (adamw_table_kernel
// in optim_table.hip keeps the same frame written out, for its speed; it shares everything else here).  Work items never cross a tensor: item it covers elements [off[it], off[it] + len[it]) of the arena, at most 4096 of
// them, starting 32-byte aligned, all of segment seg[it].  Workgroups of 256 threads stride over the items; the alignment gaps
// between tensors are in no item, so nothing reads or writes them.  Every element has one owner: no atomics, the same bits on every run.
#pragma once
#include <initializer_list>
#include "mv_common.h"

// The work list and the per-segment tables, as every entry point receives them.
struct table_list {
  const int64_t* off;
  const int32_t* len;
  const int32_t* seg;
  long n_items;
  const float* seg_lr_scale;
  const float* seg_wd;
};

// The per-step scalars live on the device when `hyper` is given (captured launches stay valid): lr, 1 - beta1^t, 1 - beta2^t.
__device__ __forceinline__ float table_hyper(const float* hyper, int i, float launch_value) { return hyper ? hyper[i] : launch_value; }
// clip_grad_norm_'s min(1, max_norm / (norm + 1e-6)), computed on the device, rides on the gradient scale.
__device__ __forceinline__ float table_gscale(float gscale, const float* clip_coef) { return clip_coef ? gscale * clip_coef[0] : gscale; }
// THE weight EMA, ema = d * ema + (1 - d) * p_new, for every operation that keeps one.
__device__ __forceinline__ void table_ema(float& E, float P, float d) { E = __builtin_fmaf(d, E, (1.f - d) * P); }

// What an operation may leave out: the per-item prologue and the end-of-item hook.
struct table_op {
  __device__ __forceinline__ void begin(long, int) {}
  __device__ __forceinline__ void end(long) {}
};

// An operation Op over N arena arrays declares the arrays it reads and writes (bit k of Op::READS / Op::WRITES: array k; an array in
// neither may be null) and has
//   begin(it, seg)  once per item, by all 256 threads (it may hold a barrier): the item's rates, LAMB's trust ratio;
//   one(x)          once per element, x[k] = that element of array k (0 where array k is not read); what it leaves in x is stored;
//   end(it)         once per item, by all 256 threads: LAMB's partial sums.
// The float4 body and the tail of at most 3 elements go through the SAME one(), whose fused multiply-adds are spelled out: the two
// round alike.  A thread meets its elements in index order (float4 i = tid, tid + 256, ..., then its tail element).
template <int N, typename Op>
__device__ __forceinline__ void table_walk(float* const (&arena)[N], const table_list& L, Op& op) {
  constexpr unsigned USED = Op::READS | Op::WRITES;
  for (long it = blockIdx.x; it < L.n_items; it += gridDim.x) {
    const long off = L.off[it];
    const int len = L.len[it];
    op.begin(it, L.seg[it]);
    float* a[N];
#pragma unroll
    for (int k = 0; k < N; ++k) a[k] = (USED >> k & 1) ? arena[k] + off : nullptr;
    const int n4 = len >> 2;
    for (int i = threadIdx.x; i < n4; i += 256) {
      float4 X[N] = {};
#pragma unroll
      for (int k = 0; k < N; ++k)
        if (Op::READS >> k & 1) X[k] = reinterpret_cast<const float4*>(a[k])[i];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float x[N];
#pragma unroll
        for (int k = 0; k < N; ++k) x[k] = (&X[k].x)[e];
        op.one(x);
#pragma unroll
        for (int k = 0; k < N; ++k) (&X[k].x)[e] = x[k];
      }
#pragma unroll
      for (int k = 0; k < N; ++k)
        if (Op::WRITES >> k & 1) reinterpret_cast<float4*>(a[k])[i] = X[k];
    }
    const int i = (n4 << 2) + threadIdx.x;      // at most 3 tail elements
    if (i < len) {
      float x[N] = {};
#pragma unroll
      for (int k = 0; k < N; ++k)
        if (Op::READS >> k & 1) x[k] = a[k][i];
      op.one(x);
#pragma unroll
      for (int k = 0; k < N; ++k)
        if (Op::WRITES >> k & 1) a[k][i] = x[k];
    }
    op.end(it);
  }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------
// One workgroup per item, at most as many as are resident at once.
template <auto K>
int table_grid(long n_items) {
  const long resident = mv_resident_blocks<K>(256, 0);
  return (int)(n_items < resident ? n_items : resident);
}

// The checks every entry point makes, in their order of precedence: the counts, the optimizer's own `params_ok` and the EMA decay (a
// NaN fails every comparison), then -- only with items to step -- `arrays` non-null, they and the optional `ema` 16-byte aligned,
// and the tables non-null.  MV_OK with L.n_items == 0 means there is nothing to launch.
inline int table_check(const table_list& L, int n_seg, bool params_ok, const float* ema, float ema_decay,
                       std::initializer_list<const void*> arrays) {
  MV_REQUIRE(L.n_items >= 0 && n_seg > 0, MV_ERR_SHAPE);
  MV_REQUIRE(params_ok && (ema == nullptr || (ema_decay >= 0.f && ema_decay < 1.f)), MV_ERR_UNSUPPORTED);
  if (L.n_items == 0) return MV_OK;
  for (const void* a : arrays) MV_REQUIRE(a && mv_aligned16(a), MV_ERR_ALIGN);
  MV_REQUIRE(mv_aligned16(ema), MV_ERR_ALIGN);
  MV_REQUIRE(L.off && L.len && L.seg && L.seg_lr_scale && L.seg_wd, MV_ERR_ALIGN);
  return MV_OK;
}
