// DeiT distillation loss (gfx950): the student's cross entropy and the distillation head's loss against a frozen teacher, with both
// gradients and the student's arg-max, in one launch plus a one-wave fixed-order mean.
//
// Reference: DistillWrapper.forward, models/distill.py:142-151 --
//     loss = F.cross_entropy(student_logits, labels) * alpha
//          + F.kl_div(log_softmax(distill_logits / T), softmax(teacher_logits / T), "batchmean") * T^2 * (1 - alpha)
// The cross entropy term is the per-sample value of mv_cross_entropy_soft (csrc/mixup.hip: same lam / eps / pair_flip, same
// arithmetic in the same order), so the Mixup recipe composes with distillation.  mode MV_DISTILL_HARD is DeiT's hard-label
// variant: the teacher's arg-max is the distillation head's label.  T, alpha, lam and eps are host scalars (launch arguments):
// nothing is read back, nothing synchronises.
#include "mv_common.h"

namespace {

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// wave arg-max, first index wins on ties (torch.argmax semantics, as ce_soft_kernel)
__device__ __forceinline__ void wave_argmax(float& mx, int& am) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float om = __shfl_xor(mx, o, 64);
    const int oa = __shfl_xor(am, o, 64);
    if (om > mx || (om == mx && oa < am)) { mx = om; am = oa; }
  }
}

// One wave per sample, classes strided over the lanes; every row is a few KiB and stays in cache between its passes.  The two
// per-sample losses go to sample[smp] (cross entropy) and sample[B + smp] (distillation); distill_mean_kernel sums those in a fixed
// order, so no floating-point atomic is involved anywhere.  A gradient whose weight (alpha, 1 - alpha) is zero is written as +0.
template <int MODE>
__global__ __launch_bounds__(256) void distill_kernel(const float* __restrict__ student, const float* __restrict__ distill,
                                                      const float* __restrict__ teacher, const int64_t* __restrict__ labels,
                                                      float* __restrict__ sample, float* __restrict__ dstudent,
                                                      float* __restrict__ ddistill, int64_t* __restrict__ argmax, int B, int C,
                                                      float T, float alpha, float lam, float eps, int pair_flip, float gscale) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float oml = 1.0f - lam, on = 1.0f - eps, off = eps / (float)C;
  const float w = gscale / (float)B;
  const float oma = 1.0f - alpha;
  const float ws = alpha * w, wd = oma * w;
  for (int smp = blockIdx.x * 4 + wave; smp < B; smp += gridDim.x * 4) {
    // ---- student: the cross entropy of ce_soft_kernel, term for term
    const float* lp = student + (long)smp * C;
    float mx = -INFINITY, zs = 0.f;
    int am = 0;
    for (int c = lane; c < C; c += 64) {
      const float v = lp[c];
      zs += v;
      if (v > mx) { mx = v; am = c; }
    }
    wave_argmax(mx, am);
    zs = wave_sum(zs);
    float s = 0.f;
    for (int c = lane; c < C; c += 64) s += expf(lp[c] - mx);
    s = wave_sum(s);
    const int64_t yi = labels[smp], yj = pair_flip ? labels[B - 1 - smp] : yi;
    const bool valid = yi >= 0 && yi < C && yj >= 0 && yj < C;      // a label outside [0, C) is never used as an index
    const int a = valid ? (int)yi : 0, b = valid ? (int)yj : 0;      // an index inside the row either way
    if (lane == 0) {
      const float lse = mx + logf(s);
      sample[smp] = valid ? lse - on * (lam * lp[a] + oml * lp[b]) - off * zs : __builtin_nanf("");
      if (argmax) argmax[smp] = am;
    }
    if (dstudent) {
      float* dp = dstudent + (long)smp * C;
      for (int c = lane; c < C; c += 64) {
        const float t = off + on * ((c == a ? lam : 0.f) + (c == b ? oml : 0.f));
        dp[c] = (valid && alpha != 0.f) ? (expf(lp[c] - mx) / s - t) * ws : 0.f;   // a poisoned row carries no gradient
      }
    }

    // ---- distillation head against the teacher
    const float* tp = teacher + (long)smp * C;
    const float* qp = distill + (long)smp * C;
    float* gp = ddistill ? ddistill + (long)smp * C : nullptr;
    float mt = -INFINITY, md = -INFINITY;
    int at = 0;
    for (int c = lane; c < C; c += 64) {
      const float v = tp[c];
      if (v > mt) { mt = v; at = c; }
      md = fmaxf(md, qp[c]);
    }
    wave_argmax(mt, at);
    md = wave_max(md);
    if (MODE == MV_DISTILL_SOFT) {
      float st = 0.f, sd = 0.f;
      for (int c = lane; c < C; c += 64) {
        st += expf((tp[c] - mt) / T);
        sd += expf((qp[c] - md) / T);
      }
      st = wave_sum(st);
      sd = wave_sum(sd);
      const float lst = logf(st), lsd = logf(sd);
      float kd = 0.f;
      for (int c = lane; c < C; c += 64) {
        const float u = (tp[c] - mt) / T, v = (qp[c] - md) / T;
        const float p = expf(u) / st, q = expf(v) / sd;
        if (p > 0.f) kd += p * ((u - lst) - (v - lsd));              // a class the teacher gives no mass adds nothing
        if (gp) gp[c] = oma != 0.f ? T * (q - p) * wd : 0.f;
      }
      kd = wave_sum(kd);
      if (lane == 0) sample[B + smp] = T * T * kd;
    } else {
      float sd = 0.f;
      for (int c = lane; c < C; c += 64) sd += expf(qp[c] - md);
      sd = wave_sum(sd);
      if (lane == 0) sample[B + smp] = md + logf(sd) - qp[at];
      if (gp)
        for (int c = lane; c < C; c += 64) gp[c] = oma != 0.f ? (expf(qp[c] - md) / sd - (c == at ? 1.f : 0.f)) * wd : 0.f;
    }
  }
}

// loss[1] = mean of sample[0 .. B), loss[2] = mean of sample[B .. 2B), loss[0] = alpha * loss[1] + (1 - alpha) * loss[2], by ONE
// wave: lane l adds rows l, l + 64, ... in order, then the wave butterfly.  The order depends on B alone, so the same inputs give the
// same bits every run; a NaN row makes its mean and the total NaN.
__global__ __launch_bounds__(64) void distill_mean_kernel(const float* __restrict__ sample, float* __restrict__ loss, int B,
                                                          float alpha) {
  float ce = 0.f, kd = 0.f;
  for (int i = threadIdx.x; i < B; i += 64) {
    ce += sample[i];
    kd += sample[B + i];
  }
  ce = wave_sum(ce);
  kd = wave_sum(kd);
  if (threadIdx.x == 0) {
    ce /= (float)B;
    kd /= (float)B;
    loss[0] = alpha * ce + (1.0f - alpha) * kd;
    loss[1] = ce;
    loss[2] = kd;
  }
}

}  // namespace

extern "C" int mv_distill_loss(const float* student, const float* distill, const float* teacher, const int64_t* labels, float* loss,
                               float* sample_loss, float* dstudent, float* ddistill, int64_t* argmax, int B, int C, int mode,
                               float T, float alpha, float lam, float eps, int pair_flip, float grad_scale, mv_stream_t stream) {
  MV_REQUIRE(B >= 0 && C >= 2, MV_ERR_SHAPE);
  MV_REQUIRE(mode == MV_DISTILL_SOFT || mode == MV_DISTILL_HARD, MV_ERR_UNSUPPORTED);
  MV_REQUIRE(T > 0.f && T <= 3.0e38f && alpha >= 0.f && alpha <= 1.f, MV_ERR_UNSUPPORTED);  // a NaN fails both
  MV_REQUIRE(eps >= 0.f && eps < 1.f && lam >= 0.f && lam <= 1.f, MV_ERR_UNSUPPORTED);     // the limits of mv_cross_entropy_soft
  MV_REQUIRE(pair_flip != 0 || lam == 1.f, MV_ERR_UNSUPPORTED);                            // no partner: nothing to blend with
  if (B == 0) return MV_OK;                      // an empty batch has no storage: its pointers may be null
  MV_REQUIRE(student && distill && teacher && labels && loss && sample_loss, MV_ERR_ALIGN);
  hipStream_t s = (hipStream_t)stream;
  int blocks = mv_cdiv(B, 4);
  if (blocks > 4096) blocks = 4096;              // grid-stride beyond
  if (int rc = mv_pick<MV_DISTILL_SOFT, MV_DISTILL_HARD>(mode, [&](auto M) {
        return mv_launch<distill_kernel<M()>>(MV_HERE, blocks, 256, 0, s, student, distill, teacher, labels, sample_loss, dstudent,
                                              ddistill, argmax, B, C, T, alpha, lam, eps, pair_flip, grad_scale);
      }))
    return rc;
  return mv_launch<distill_mean_kernel>(MV_HERE, 1, 64, 0, s, (const float*)sample_loss, loss, B, alpha);
}
