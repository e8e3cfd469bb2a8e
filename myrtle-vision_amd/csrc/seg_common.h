// Bilinear-source helpers shared by the fused segmentation tails (seg_tail.hip: plain mean cross entropy; seg_loss.hip: class
// weights, label smoothing, Dice).  Both files interpolate a pixel's logits with THESE expressions, so their lse / arg-max agree
// bit for bit.
#pragma once
#include "mv_common.h"

namespace {

// ATen upsample_bilinear2d, align_corners=False: src = (dst + 0.5) * scale - 0.5, clamped at 0 (same as elementwise.hip)
__device__ __forceinline__ void seg_src(int d, float scale, int in_size, int& i0, int& i1, float& l1) {
  float s = ((float)d + 0.5f) * scale - 0.5f;
  if (s < 0.f) s = 0.f;
  i0 = (int)s;
  if (i0 > in_size - 1) i0 = in_size - 1;
  i1 = i0 + (i0 < in_size - 1 ? 1 : 0);
  l1 = s - (float)i0;
}

__device__ __forceinline__ float seg_interp(const float* s00, const float* s01, const float* s10, const float* s11, int c,
                                            float lx, float ly) {
  const float top = s00[c] * (1.f - lx) + s01[c] * lx;
  const float bot = s10[c] * (1.f - lx) + s11[c] * lx;
  return top * (1.f - ly) + bot * ly;
}

__device__ __forceinline__ void seg_stage_map(float* smap, const float* __restrict__ small, long b, int cells_c) {
  const float* src = small + b * cells_c;
  for (int i = threadIdx.x; i < cells_c; i += blockDim.x) smap[i] = src[i];
}

}  // namespace
