// Fused segmentation tail with a training recipe: per-class weights, label smoothing and a soft Dice term on
//   z = Upsample(size=(H,W), mode="bilinear")(small),  p = softmax(z)
// without materialising the [B, C, H, W] logits or their gradient (the contract is written out in include/myrtle_vision_hip.h).
// Same structure as seg_tail.hip, whose kernels and entry points stay what they are (the plain mean cross entropy runs there):
//
//   forward : one thread per output pixel (4 pixels per thread).  lse and the arg-max come from the expressions of
//             seg_ce_fwd_kernel in the same channel order (bitwise the same).  With smoothing or Dice a third pass over the
//             channels adds  sum_c w_c (lse - z_c)  and the per-class sums P_c = sum p_c, I_c = sum p_c [y = c], held in 2C
//             registers (I_c by a select on the label).  Every float sum has a fixed order: registers, xor-shuffle over the
//             wave, the four waves of the block, then ONE finishing block that walks the per-block rows in a fixed order (in
//             fp64) and forms the loss, the CE denominator and the Dice coefficients a_c, b_c.  Counts (out-of-range labels,
//             intersection / prediction / label areas per class) are integers from end to end: LDS integer adds per block,
//             int32 per block in the row, int64 totals.  No float atomics, no memset, no host read.
//   backward: gather form as seg_ce_bwd_kernel.  Per valid pixel
//               dz_c = [p_c ((1-eps) w_y + (eps/C) sum_k w_k) - (1-eps) w_y [y=c] - (eps/C) w_c] / W
//                      + lam p_c (g_c - sum_k p_k g_k),   g_c = a_c [y=c] + b_c
//             with the per-class factors pre-multiplied into four 32-entry LDS tables.  All zero when W = sum w_y is 0.
#include "seg_common.h"

namespace {

constexpr int SL_CMAX = 32;                   // classes held in registers (P_c, I_c in the forward; the sums of the backward)
constexpr int SL_PX_PER_BLOCK = 1024;
constexpr int SL_NF = 3;                      // leading float columns of a row: CE numerator, smoothing numerator, sum of w_y
constexpr int SL_RED = SL_NF + 2 * SL_CMAX;   // floats a wave hands to the block sum
constexpr int SL_FWD_EXTRA = 400;             // LDS words behind the map: weights [32], wave sums [4][SL_RED], counts [1 + 3*32]
constexpr int SL_BWD_EXTRA = 4 * SL_CMAX;     // LDS words behind map and column sums: w, (eps/C) w / W, lam a, lam b
constexpr size_t SL_LDS_LIMIT = 64 * 1024;

// one row of 4-byte words per forward block:
//   [0] CE numerator  [1] smoothing numerator  [2] sum w_y            (fp32)
//   [3] out-of-range labels  [4 + c] intersect_c  [4 + C + c] pred_c  [4 + 2C + c] label_c   (int32)
//   with Dice: [4 + 3C + c] P_c  [4 + 4C + c] I_c                      (fp32)
__host__ __device__ inline int sl_row_words(int C, bool dice) { return 4 + 3 * C + (dice ? 2 * C : 0); }

template <bool DICE>
__global__ __launch_bounds__(256) void seg_loss_fwd_kernel(const float* __restrict__ small,
                                                           const int64_t* __restrict__ labels,
                                                           const float* __restrict__ class_weight, float eps,
                                                           float* __restrict__ lse, uint8_t* __restrict__ pred,
                                                           float* __restrict__ partials, int C, int h, int w, int H, int W,
                                                           float sh, float sw) {
  extern __shared__ float smem[];
  float* smap = smem;                                   // [h*w][C]
  float* wl = smap + h * w * C;                         // [32] class weights (ones without class_weight)
  float* red = wl + SL_CMAX;                            // [4][SL_RED]
  int* cnt = (int*)(red + 4 * SL_RED);                  // [0] bad, [1 + c] intersect, [1 + C + c] pred, [1 + 2C + c] label
  const long b = blockIdx.y;
  seg_stage_map(smap, small, b, h * w * C);
  if (threadIdx.x < SL_CMAX) wl[threadIdx.x] = (int)threadIdx.x < C ? (class_weight ? class_weight[threadIdx.x] : 1.f) : 0.f;
  for (int i = threadIdx.x; i < 1 + 3 * SL_CMAX; i += 256) cnt[i] = 0;
  __syncthreads();
  const int npix = H * W;
  const int p0 = blockIdx.x * SL_PX_PER_BLOCK;
  const bool third = DICE || eps > 0.f;
  float my_ce = 0.f, my_sm = 0.f, my_w = 0.f;
  float Pc[SL_CMAX], Ic[SL_CMAX];
#pragma unroll
  for (int c = 0; c < SL_CMAX; ++c) Pc[c] = Ic[c] = 0.f;
  for (int p = p0 + threadIdx.x; p < p0 + SL_PX_PER_BLOCK && p < npix; p += 256) {
    const int Y = p / W, X = p - Y * W;
    int y0, y1, x0, x1;
    float ly, lx;
    seg_src(Y, sh, h, y0, y1, ly);
    seg_src(X, sw, w, x0, x1, lx);
    const float *s00 = smap + (y0 * w + x0) * C, *s01 = smap + (y0 * w + x1) * C;
    const float *s10 = smap + (y1 * w + x0) * C, *s11 = smap + (y1 * w + x1) * C;
    // -100 (ignore_index) is skipped and not counted; anything else outside [0, C) poisons the loss and is never an index
    const int64_t yl = labels[b * npix + p];
    const bool valid = yl >= 0 && yl < C;
    const int y = valid ? (int)yl : -1;
    float mx = -INFINITY, vy = 0.f;
    int am = 0;
    for (int c = 0; c < C; ++c) {
      const float v = seg_interp(s00, s01, s10, s11, c, lx, ly);
      if (v > mx) { mx = v; am = c; }
      if (c == y) vy = v;
    }
    float s = 0.f;
    for (int c = 0; c < C; ++c) s += expf(seg_interp(s00, s01, s10, s11, c, lx, ly) - mx);
    const float l = mx + logf(s);
    lse[b * npix + p] = l;
    pred[b * npix + p] = (uint8_t)am;
    const float wy = valid ? wl[y] : 0.f;
    my_ce += valid ? wy * (l - vy) : 0.f;
    my_w += wy;
    if (!valid && yl != -100) atomicAdd(&cnt[0], 1);
    atomicAdd(&cnt[1 + C + am], 1);                     // predictions count over ALL pixels (utils/miou.intersect_and_union)
    if (valid) {
      atomicAdd(&cnt[1 + 2 * C + y], 1);
      if (am == y) atomicAdd(&cnt[1 + y], 1);
    }
    if (third) {                                        // uniform over the grid
      float sm = 0.f;
#pragma unroll
      for (int c = 0; c < SL_CMAX; ++c)
        if (c < C) {
          const float v = seg_interp(s00, s01, s10, s11, c, lx, ly);
          sm += wl[c] * (l - v);
          if (DICE) {
            const float pc = expf(v - l);
            Pc[c] += valid ? pc : 0.f;
            Ic[c] += (c == y) ? pc : 0.f;               // y = -1 for a pixel that is not valid
          }
        }
      my_sm += valid ? sm : 0.f;
    }
  }
  const int wave = threadIdx.x >> 6;
  const bool lead = (threadIdx.x & 63) == 0;
  my_ce = wave_sum(my_ce);
  my_sm = wave_sum(my_sm);
  my_w = wave_sum(my_w);
  if (lead) {
    red[wave * SL_RED] = my_ce;
    red[wave * SL_RED + 1] = my_sm;
    red[wave * SL_RED + 2] = my_w;
  }
  if (DICE) {
#pragma unroll
    for (int c = 0; c < SL_CMAX; ++c)
      if (c < C) {
        const float ps = wave_sum(Pc[c]), is = wave_sum(Ic[c]);
        if (lead) {
          red[wave * SL_RED + SL_NF + c] = ps;
          red[wave * SL_RED + SL_NF + SL_CMAX + c] = is;
        }
      }
  }
  __syncthreads();
  const int R = sl_row_words(C, DICE);
  float* row = partials + (b * gridDim.x + blockIdx.x) * R;
  for (int i = threadIdx.x; i < R; i += 256) {
    if (i >= SL_NF && i < 4 + 3 * C) {
      ((int*)row)[i] = cnt[i - SL_NF];
    } else {
      const int k = i < SL_NF ? i : (i < 4 + 4 * C ? SL_NF + (i - (4 + 3 * C)) : SL_NF + SL_CMAX + (i - (4 + 4 * C)));
      row[i] = (red[k] + red[SL_RED + k]) + (red[2 * SL_RED + k] + red[3 * SL_RED + k]);
    }
  }
}

// ONE block: column sums of the per-block rows in a fixed order (thread <-> (column, row phase); phases combined in order), floats
// in fp64, counts in int64; then stats[8], coef[2C] = (a_c | b_c) and areas[3C] = (intersect | pred | label).
__global__ __launch_bounds__(1024) void seg_loss_finish_kernel(const float* __restrict__ partials, long nblk, int C, int dice,
                                                               float eps, float lam, float smooth, double pixels,
                                                               float* __restrict__ stats, float* __restrict__ coef,
                                                               int64_t* __restrict__ areas) {
  __shared__ double redf[1024];
  __shared__ long long redi[1024];
  __shared__ double totf[4 + 5 * SL_CMAX];
  __shared__ long long toti[4 + 5 * SL_CMAX];
  __shared__ double dterm[SL_CMAX];
  const int R = sl_row_words(C, dice != 0);
  const int nph = 1024 / R;
  const int t = threadIdx.x, col = t % R, ph = t / R;
  const bool isint = col >= SL_NF && col < 4 + 3 * C;
  double f = 0.0;
  long long n = 0;
  if (ph < nph) {
    // one block reads every row (4.5 MB at B = 256, 224^2 with Dice): 16 loads in flight per thread, added in row order
    const unsigned* src = (const unsigned*)partials + col;
    long r = ph;
    for (; r + 15L * nph < nblk; r += 16L * nph) {
      unsigned word[16];
#pragma unroll
      for (int j = 0; j < 16; ++j) word[j] = src[(r + (long)j * nph) * R];
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        if (isint) n += (int)word[j];
        else f += (double)__uint_as_float(word[j]);
      }
    }
    for (; r < nblk; r += nph) {
      const unsigned word = src[r * R];
      if (isint) n += (int)word;
      else f += (double)__uint_as_float(word);
    }
  }
  redf[t] = f;
  redi[t] = n;
  __syncthreads();
  if (t < R) {
    double tf = 0.0;
    long long ti = 0;
    for (int q = 0; q < nph; ++q) {
      tf += redf[q * R + t];
      ti += redi[q * R + t];
    }
    totf[t] = tf;
    toti[t] = ti;
  }
  __syncthreads();
  if (t < C) {
    const long long nc = toti[4 + 2 * C + t];
    if (areas) {
      areas[t] = toti[4 + t];
      areas[C + t] = toti[4 + C + t];
      areas[2 * C + t] = nc;
    }
    double a = 0.0, bq = 0.0, d = 0.0;
    if (dice) {
      const double num = 2.0 * totf[4 + 4 * C + t] + (double)smooth;
      const double U = totf[4 + 3 * C + t] + (double)nc + (double)smooth;
      a = -(2.0 / C) / U;
      bq = num / (U * U) / C;
      d = num / U;
    }
    coef[t] = (float)a;
    coef[C + t] = (float)bq;
    dterm[t] = d;
  }
  __syncthreads();
  if (t == 0) {
    long long hit = 0, ok = 0;
    double ds = 0.0;
    for (int c = 0; c < C; ++c) {
      hit += toti[4 + c];
      ok += toti[4 + 2 * C + c];
      ds += dterm[c];
    }
    const long long bad = toti[SL_NF];
    const double Wsum = totf[2];
    const double e = (double)eps;
    // NaN for lack of a denominator (torch's 0/0) or for a label outside [0, C) that is not -100
    const float ce = (!(Wsum > 0.0) || bad > 0) ? __builtin_nanf("") : (float)(((1.0 - e) * totf[0] + (e / C) * totf[1]) / Wsum);
    const float dl = dice ? (float)(1.0 - ds / C) : 0.f;
    stats[0] = dice ? ce + lam * dl : ce;
    stats[1] = (float)((double)hit / pixels);
    stats[2] = (float)ok;
    stats[3] = (float)bad;
    stats[4] = ce;
    stats[5] = dl;
    stats[6] = (float)Wsum;
    stats[7] = 0.f;
  }
}

// the empty batch: stats[8] and areas[3C] <- 0 (a kernel, not hipMemsetAsync: graph-capture safe, as mv_seg_ce_fwd)
__global__ void seg_loss_clear_kernel(float* __restrict__ stats, int64_t* __restrict__ areas, int C) {
  for (int i = threadIdx.x; i < 8; i += blockDim.x) stats[i] = 0.f;
  if (areas)
    for (int i = threadIdx.x; i < 3 * C; i += blockDim.x) areas[i] = 0;
}

template <typename DT, bool DICE>
__global__ __launch_bounds__(256) void seg_loss_bwd_kernel(const float* __restrict__ small,
                                                           const int64_t* __restrict__ labels,
                                                           const float* __restrict__ class_weight, float eps, float lam,
                                                           const float* __restrict__ lse, const float* __restrict__ stats,
                                                           const float* __restrict__ coef, DT* __restrict__ dsmall, int ld_ds,
                                                           float gscale, int C, int h, int w, int H, int W, float sh, float sw) {
  extern __shared__ float smem[];
  float* smap = smem;                                   // [h*w][C]
  float* colacc = smem + h * w * C;                     // [W][C]
  float* wl = colacc + W * C;                           // [32] w_c
  float* ew = wl + SL_CMAX;                             // [32] (eps/C) w_c / W
  float* ca = ew + SL_CMAX;                             // [32] lam a_c
  float* cb = ca + SL_CMAX;                             // [32] lam b_c
  const long b = blockIdx.y;
  const int sy = blockIdx.x;
  seg_stage_map(smap, small, b, h * w * C);
  // W = sum of w_y over the valid pixels (stats[6] of the forward); without it the loss is NaN and the gradient is zero
  const float Wsum = stats[6];
  const bool live = Wsum > 0.f;
  const float invW = live ? 1.f / Wsum : 0.f;
  const float eC = eps / (float)C;
  if (threadIdx.x < SL_CMAX) {
    const int c = threadIdx.x;
    const float wc = c < C ? (class_weight ? class_weight[c] : 1.f) : 0.f;
    wl[c] = wc;
    ew[c] = eC * wc * invW;
    ca[c] = (DICE && live && c < C) ? lam * coef[c] : 0.f;
    cb[c] = (DICE && live && c < C) ? lam * coef[C + c] : 0.f;
  }
  __syncthreads();
  float sumw = 0.f;
  for (int c = 0; c < C; ++c) sumw += wl[c];
  const float one_m = (1.f - eps) * invW, epsw = eC * sumw * invW;
  const int npix = H * W;
  // candidate output rows: a superset of those whose y0 or y1 can equal sy (same bound as seg_ce_bwd_kernel)
  int Ylo = (int)floorf(((float)sy - 1.f + 0.5f) / sh - 0.5f) - 1, Yhi = (int)ceilf(((float)sy + 1.f + 0.5f) / sh - 0.5f) + 1;
  if (Ylo < 0) Ylo = 0;
  if (Yhi > H - 1) Yhi = H - 1;
  for (int X = threadIdx.x; X < W; X += 256) {
    int x0, x1;
    float lx;
    seg_src(X, sw, w, x0, x1, lx);
    float acc[SL_CMAX];
#pragma unroll
    for (int c = 0; c < SL_CMAX; ++c) acc[c] = 0.f;
    for (int Y = Ylo; Y <= Yhi; ++Y) {
      int y0, y1;
      float ly;
      seg_src(Y, sh, h, y0, y1, ly);
      float wy = 0.f;
      if (y0 == sy) wy += 1.f - ly;
      if (y1 == sy) wy += ly;
      if (wy == 0.f) continue;                          // uniform over the workgroup
      const float *s00 = smap + (y0 * w + x0) * C, *s01 = smap + (y0 * w + x1) * C;
      const float *s10 = smap + (y1 * w + x0) * C, *s11 = smap + (y1 * w + x1) * C;
      const long pix = b * npix + (long)Y * W + X;
      const int64_t yl = labels[pix];
      if (yl < 0 || yl >= C) continue;                  // ignored (or bad) label: no gradient from this pixel
      const int y = (int)yl;
      const float l = lse[pix];
      const float by = one_m * wl[y];                   // (1-eps) w_y / W
      const float Aw = by + epsw;                       // ((1-eps) w_y + (eps/C) sum_k w_k) / W
      if (DICE) {
        float pc[SL_CMAX];
        float G = 0.f;
#pragma unroll
        for (int c = 0; c < SL_CMAX; ++c)
          if (c < C) {
            pc[c] = expf(seg_interp(s00, s01, s10, s11, c, lx, ly) - l);
            G += pc[c] * (cb[c] + (c == y ? ca[c] : 0.f));
          }
#pragma unroll
        for (int c = 0; c < SL_CMAX; ++c)
          if (c < C) acc[c] += wy * (pc[c] * (Aw + (cb[c] - G)) - ew[c] + (c == y ? pc[c] * ca[c] - by : 0.f));
      } else {
#pragma unroll
        for (int c = 0; c < SL_CMAX; ++c)
          if (c < C) acc[c] += wy * (expf(seg_interp(s00, s01, s10, s11, c, lx, ly) - l) * Aw - ew[c] - (c == y ? by : 0.f));
      }
    }
#pragma unroll
    for (int c = 0; c < SL_CMAX; ++c)
      if (c < C) colacc[X * C + c] = acc[c];
  }
  __syncthreads();
  for (int i = threadIdx.x; i < w * ld_ds; i += 256) {
    const int sx = i / ld_ds, c = i - sx * ld_ds;
    float s = 0.f;
    if (c < C) {
      int Xlo = (int)floorf(((float)sx - 1.f + 0.5f) / sw - 0.5f) - 1, Xhi = (int)ceilf(((float)sx + 1.f + 0.5f) / sw - 0.5f) + 1;
      if (Xlo < 0) Xlo = 0;
      if (Xhi > W - 1) Xhi = W - 1;
      for (int X = Xlo; X <= Xhi; ++X) {
        int x0, x1;
        float lx;
        seg_src(X, sw, w, x0, x1, lx);
        float wx = 0.f;
        if (x0 == sx) wx += 1.f - lx;
        if (x1 == sx) wx += lx;
        if (wx != 0.f) s += wx * colacc[X * C + c];
      }
    }
    dsmall[(b * h * w + (long)sy * w + sx) * ld_ds + c] = (DT)(s * gscale);
  }
}

inline int sl_check_scalars(float label_smoothing, float dice_weight, float dice_smooth) {
  if (!(label_smoothing >= 0.f && label_smoothing < 1.f)) return MV_ERR_UNSUPPORTED;
  if (!(dice_weight >= 0.f)) return MV_ERR_UNSUPPORTED;
  if (dice_weight > 0.f && !(dice_smooth > 0.f)) return MV_ERR_UNSUPPORTED;
  return MV_OK;
}

}  // namespace

extern "C" long mv_seg_loss_partials(int B, int C, int H, int W) {
  if (B <= 0 || C <= 0 || H <= 0 || W <= 0) return 0;
  return (long)B * (((long)H * W + SL_PX_PER_BLOCK - 1) / SL_PX_PER_BLOCK) * sl_row_words(C, true);
}

extern "C" int mv_seg_loss_fwd(const float* small, const int64_t* labels, const float* class_weight, float label_smoothing,
                               float dice_weight, float dice_smooth, float* lse, uint8_t* pred, float* partials, float* stats,
                               float* coef, int64_t* areas, int B, int C, int h, int w, int H, int W, mv_stream_t stream) {
  MV_REQUIRE(B >= 0 && C > 0 && h > 0 && w > 0 && H > 0 && W > 0, MV_ERR_SHAPE);
  MV_REQUIRE(B <= 65535, MV_ERR_SHAPE);
  MV_REQUIRE(C <= SL_CMAX, MV_ERR_UNSUPPORTED);
  const size_t lds = ((size_t)h * w * C + SL_FWD_EXTRA) * sizeof(float);
  MV_REQUIRE(lds <= SL_LDS_LIMIT, MV_ERR_UNSUPPORTED);
  MV_REQUIRE(sl_check_scalars(label_smoothing, dice_weight, dice_smooth) == MV_OK, MV_ERR_UNSUPPORTED);
  hipStream_t s = (hipStream_t)stream;
  if (B == 0) return mv_launch<seg_loss_clear_kernel>(MV_HERE, 1, 128, 0, s, stats, areas, C);
  const int bpi = (int)(((long)H * W + SL_PX_PER_BLOCK - 1) / SL_PX_PER_BLOCK);
  const int dice = dice_weight > 0.f ? 1 : 0;
  if (int rc = mv_pick<0, 1>(dice, [&](auto D) {
        return mv_launch<seg_loss_fwd_kernel<D() != 0>>(MV_HERE, dim3(bpi, B), 256, lds, s, small, labels, class_weight, label_smoothing,
                                                        lse, pred, partials, C, h, w, H, W, (float)h / (float)H, (float)w / (float)W);
      }))
    return rc;
  return mv_launch<seg_loss_finish_kernel>(MV_HERE, 1, 1024, 0, s, (const float*)partials, (long)bpi * B, C, dice, label_smoothing,
                                           dice_weight, dice_smooth, (double)B * (double)H * (double)W, stats, coef, areas);
}

extern "C" int mv_seg_loss_bwd(const float* small, const int64_t* labels, const float* class_weight, float label_smoothing,
                               float dice_weight, const float* lse, const float* stats, const float* coef, void* dsmall,
                               int ds_elem, int ld_ds, float grad_scale, int B, int C, int h, int w, int H, int W,
                               mv_stream_t stream) {
  MV_REQUIRE(B >= 0 && C > 0 && h > 0 && w > 0 && H > 0 && W > 0 && ld_ds >= C, MV_ERR_SHAPE);
  MV_REQUIRE(B <= 65535, MV_ERR_SHAPE);
  MV_REQUIRE(ds_elem == MV_F32 || ds_elem == MV_BF16, MV_ERR_UNSUPPORTED);
  MV_REQUIRE(C <= SL_CMAX, MV_ERR_UNSUPPORTED);
  const size_t lds = ((size_t)h * w * C + (size_t)W * C + SL_BWD_EXTRA) * sizeof(float);
  MV_REQUIRE(lds <= SL_LDS_LIMIT, MV_ERR_UNSUPPORTED);
  MV_REQUIRE(sl_check_scalars(label_smoothing, dice_weight, 1.f) == MV_OK, MV_ERR_UNSUPPORTED);
  if (B == 0) return MV_OK;
  MV_REQUIRE(stats != nullptr && (dice_weight == 0.f || coef != nullptr), MV_ERR_ALIGN);
  const int dice = dice_weight > 0.f ? 1 : 0;
  return mv_pick<MV_F32, MV_BF16>(ds_elem, [&](auto E) {
    using T = mv_elem_t<E()>;
    return mv_pick<0, 1>(dice, [&](auto D) {
      return mv_launch<seg_loss_bwd_kernel<T, D() != 0>>(MV_HERE, dim3(h, B), 256, lds, (hipStream_t)stream, small, labels, class_weight,
                                                         label_smoothing, dice_weight, lse, stats, coef, (T*)dsmall, ld_ds, grad_scale, C,
                                                         h, w, H, W, (float)h / (float)H, (float)w / (float)W);
    });
  });
}
