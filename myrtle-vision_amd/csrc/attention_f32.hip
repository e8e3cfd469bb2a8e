// Fused fp32 attention core on the f32-input matrix cores (gfx950, v_mfma_f32_16x16x4_f32):
//
//   out[b, n, h, :] = softmax(q k^T * scale) v        (reference: Attention.forward, models/vit.py:92-96)
//
// for the EXACT-arithmetic paths that run without autograd: the converted PyTorchINT8 model (q, k, v come out of an 8-bit
// Linear as fp32, the result goes into the next 8-bit quantiser; BASELINE config 5) and evaluation in precision="fp32".
// Every product and sum is an fp32 fma / add with one rounding, exactly as in the materialised path
// (mv_gemm_f32 + mv_softmax_fwd + mv_gemm_f32), which it replaces there: the two differ only in summation ORDER.  What it
// removes is the [B, H, N, N] probability tensor (1.9 GB per layer at batch 1024) and three launches whose 197 x 197 x 64
// products ran at 15 TFLOP/s: the materialised attention was 2/3 of the converted model's forward pass.
//
// One workgroup (8 waves) per (image, head).  K [keys][64] and V^T [64][keys] of the head sit in LDS (fp32, 2 x 53 KB at
// N <= 208); a wave owns query tiles of 16 rows.  Orientation is chosen so that nothing but V is ever transposed:
//   S^T tile = K_tile (A operand) x Q^T (B operand): a lane holds ONE query (lane & 15) and, per key tile, the four keys
//       4 (lane >> 4) + r -- the softmax statistics of a row are an in-lane reduction plus two shuffles (xor 16, 32);
//   O^T tile = V^T_tile (A) x P^T (B): the B operand of k-block (T, r) is exactly the lane's probability register (T, r)
//       -- P never leaves the registers; the lane ends with four consecutive output features of its query: float4 stores.
// Both operands of a product use the same k-assignment (lane group g supplies k = 16 c + 4 g + kk in step (c, kk)), so any
// assignment gives the same sum; this one makes every fragment a 16-byte access (global for Q, LDS for K and V^T).
// LDS images: K rows of 256 B with the 16-byte slot index XORed with (key & 15); V^T rows of NK floats with the slot index
// XORed with vt_sw(d) = {0, 0, 3, 3}[(d >> 2) & 3]: both fragment reads are conflict-free under the ds_read_b128 banking rules
// (MI355X_MICROARCH.md: a b128 read is served in the lane groups {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31}, ... -- a group
// holds every row d & 15 once, with lane group g or g ^ 1 depending on whether (d >> 2) & 3 is 1 or 2; the plain XOR with
// (d >> 2) & 3, right for 16 CONTIGUOUS lanes, was 2-way conflicted: SQ_LDS_BANK_CONFLICT = 1.3 x the kernel's LDS-active cycles).
#include "mv_common.h"

namespace {

constexpr int AF_DH = 64;
__device__ __forceinline__ int vt_sw(int d) { return (0xF0 >> (((d >> 2) & 3) * 2)) & 3; }   // {0, 0, 3, 3}[(d >> 2) & 3]
constexpr float AF_LOG2E = 1.4426950408889634f, AF_LN2 = 0.6931471805599453f;

// NT = key/query tiles of 16 (13: N <= 208, i.e. 197 tokens; 17: N <= 272, i.e. 257 tokens)
// Q8 = true: the result goes straight into to_out's quint8 quantiser and leaves as int8 codes q - 128 ([B, N, H*64] int8)
template <int NT, bool Q8 = false>
__global__ __launch_bounds__(512) void attn_fwd_f32_kernel(const float* __restrict__ qkv, float* __restrict__ out, int N,
                                                           int H, float scale, float q_inv = 0.f, float q_zp = 0.f,
                                                           float* __restrict__ lse = nullptr, int n_items = 0) {
  constexpr int NK = NT * 16;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* const Ks = smem;                    // [NK][64]
  float* const Vt = smem + NK * AF_DH;       // [64][NK]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long row = 3L * H * AF_DH;           // floats between consecutive tokens

  // ---- staging of K (row-major, swizzled slots) and V^T of one (image, head); keys >= N are zero rows / columns.
  // The kernel is PERSISTENT (grid = #CUs, one workgroup per CU by LDS): a workgroup walks items blockIdx.x, + gridDim.x, ...
  // and the 16-byte global loads of the NEXT item's K and V (7 + 7 per thread at 197 tokens) are issued before the current
  // item's products and land under them; only the LDS writes (between two barriers) stay exposed.  With one item per
  // workgroup the staging loads were 108 of 511 us at batch 256 (phase ablation, tools/ablate_attn_f32.sh): nothing else
  // runs on a CU whose only workgroup waits for memory.  NT = 17 (257 tokens) has no registers to spare: its next item's
  // loads are issued after the current item's products.
  constexpr int NIT = (NK * 16 + 511) / 512;
  constexpr bool PREFETCH = NT <= 13;
  f32x4 kst[NIT], vst[NIT];
  auto issue_loads = [&](int item) {
    const int ib = item / H, ih = item % H;
    const float* const kb = qkv + (long)ib * N * row + (long)ih * AF_DH + (long)H * AF_DH;
    const float* const vb = kb + (long)H * AF_DH;
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int i = tid + 512 * it;
      const int kkey = i >> 4, kj = i & 15;
      const int vkey = i % NK, vj = i / NK;
      kst[it] = (f32x4){0.f, 0.f, 0.f, 0.f};
      vst[it] = (f32x4){0.f, 0.f, 0.f, 0.f};
      if (i < NK * 16 && kkey < N) kst[it] = *reinterpret_cast<const f32x4*>(kb + kkey * row + 4 * kj);
      if (i < NK * 16 && vkey < N) vst[it] = *reinterpret_cast<const f32x4*>(vb + vkey * row + 4 * vj);
    }
  };
  auto write_lds = [&]() {
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int i = tid + 512 * it;
      if (i < NK * 16) {
        const int key = i >> 4, j = i & 15;
        *reinterpret_cast<f32x4*>(Ks + key * AF_DH + ((j ^ (key & 15)) << 2)) = kst[it];
      }
    }
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int i = tid + 512 * it;
      if (i < NK * 16) {
        const int key = i % NK, j = i / NK;    // lanes walk the keys: the transposed writes below are conflict-free
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int d = 4 * j + e;
          Vt[d * NK + ((((key >> 2) ^ vt_sw(d))) << 2) + (key & 3)] = vst[it][e];
        }
      }
    }
  };
  issue_loads(blockIdx.x);
  write_lds();
  __syncthreads();

  const int q16 = lane & 15, g = lane >> 4;
  const float sl2 = scale * AF_LOG2E;
  for (int item = blockIdx.x; item < n_items; item += gridDim.x) {
  const int b = item / H, h = item % H;
  const float* const qb = qkv + (long)b * N * row + (long)h * AF_DH;
  const bool has_next = item + (int)gridDim.x < n_items;      // workgroup-uniform
  if (PREFETCH && has_next) issue_loads(item + gridDim.x);
  for (int qt = wave; qt * 16 < N; qt += 8) {
    const int q = qt * 16 + q16;
    const float* qrow = qb + (long)(q < N ? q : N - 1) * row + 4 * g;       // clamped: rows >= N are never stored
    f32x4 qf[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) qf[c] = *reinterpret_cast<const f32x4*>(qrow + 16 * c);

    // ---- S^T = K Q^T: acc[T][r] = score of (query q, key 16 T + 4 g + r).  Fragments are prefetched ONE tile ahead by hand
    // and sched_barriers keep the compiler from hoisting all 52 tile loads to the top (that version spilled 255 VGPRs).
    f32x4 acc[NT];
    f32x4 kf[4], kn[4];
    auto load_k = [&](f32x4 (&dst)[4], int T) {
      const int key = T * 16 + q16;          // this lane's row of the A operand
#pragma unroll
      for (int c = 0; c < 4; ++c)
        dst[c] = *reinterpret_cast<const f32x4*>(Ks + key * AF_DH + (((4 * c + g) ^ (key & 15)) << 2));
    };
    load_k(kf, 0);
#pragma unroll
    for (int T = 0; T < NT; ++T) {
      if (T + 1 < NT) load_k(kn, T + 1);
      acc[T] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
          acc[T] = __builtin_amdgcn_mfma_f32_16x16x4f32(kf[c][kk], qf[c][kk], acc[T], 0, 0, 0);
        }
#pragma unroll
      for (int c = 0; c < 4; ++c) kf[c] = kn[c];
      __builtin_amdgcn_sched_barrier(0);
    }
    // ---- softmax over the keys (vit.py:92-93: (q k^T) * scale, then softmax): max, exp, sum, normalise
    float mx = -INFINITY;
#pragma unroll
    for (int T = 0; T < NT; ++T)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int key = T * 16 + 4 * g + r;
        const float x = key < N ? acc[T][r] * sl2 : -INFINITY;        // scores in log2 units: exp2 is one instruction
        acc[T][r] = x;
        mx = fmaxf(mx, x);
      }
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    float s = 0.f;
#pragma unroll
    for (int T = 0; T < NT; ++T)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float e = __builtin_amdgcn_exp2f(acc[T][r] - mx);      // exp2(-inf) = 0 for the padded keys
        acc[T][r] = e;
        s += e;
      }
    s += __shfl_xor(s, 16, 64);
    s += __shfl_xor(s, 32, 64);
    const float inv = 1.0f / s;
#pragma unroll
    for (int T = 0; T < NT; ++T) acc[T] *= inv;
    if (lse && g == 0 && q < N) lse[((long)b * H + h) * N + q] = (mx + __builtin_amdgcn_logf(s)) * AF_LN2;     // ln sum_j exp(scale q.k_j)

    // ---- O^T = V^T P^T: o[dt][r] = out(query q, feature 16 dt + 4 g + r)
    f32x4 o[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) o[dt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    f32x4 vf[4], vn[4];
    auto load_v = [&](f32x4 (&dst)[4], int T) {
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        const int d = dt * 16 + q16;
        dst[dt] = *reinterpret_cast<const f32x4*>(Vt + d * NK + (((4 * T + g) ^ vt_sw(d)) << 2));
      }
    };
    load_v(vf, 0);
#pragma unroll
    for (int T = 0; T < NT; ++T) {
      if (T + 1 < NT) load_v(vn, T + 1);
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
          o[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(vf[dt][r], acc[T][r], o[dt], 0, 0, 0);
        }
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) vf[dt] = vn[dt];
      __builtin_amdgcn_sched_barrier(0);
    }
    if (q < N) {
      if constexpr (Q8) {
        int8_t* op = reinterpret_cast<int8_t*>(out) + ((long)b * N + q) * H * AF_DH + (long)h * AF_DH + 4 * g;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt)
          *reinterpret_cast<unsigned*>(op + 16 * dt) = affine_i8_pack4<0>(o[dt][0], o[dt][1], o[dt][2], o[dt][3], q_inv, q_zp);
      } else {
        float* op = out + ((long)b * N + q) * H * AF_DH + (long)h * AF_DH + 4 * g;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) *reinterpret_cast<f32x4*>(op + 16 * dt) = o[dt];
      }
    }
  }
  if (has_next) {
    __syncthreads();                          // every wave is done reading this item's K / V^T
    if (!PREFETCH) issue_loads(item + gridDim.x);
    write_lds();
    __syncthreads();
  }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Backward of the same core in fp32 (training in precision="fp32"): dq, dk, dv from q, k, v, out, d(out) and the saved
// log-sum-exp -- no [B, H, N, N] tensor in either direction (the materialised path wrote and re-read 1.4 GB of scores,
// probabilities and their gradients per layer at batch 64, with 197 x 197 x 64 products at 27-47 TFLOP/s).
// One workgroup (8 waves) per (image, head), two passes over the SAME two LDS regions, no barrier inside a pass:
//   pass A (dQ):    R0 = K, R1 = V (row-major, the forward kernel's K image).  A wave owns 16 queries: S^T = K Q^T and
//                   dP^T = V dO^T (a lane holds one query and four keys per key tile), P^T = exp(scale S^T - lse),
//                   delta = rowsum(dO * out) from the query's own fragments, dS^T = P^T (dP^T - delta) scale is at once the
//                   A operand of dQ[q][d] += dS[q][key] K[key][d] (B operand: 4-byte reads of K rows).
//   pass B (dK/dV): R0 = Q, R1 = dO.  A wave owns 16 keys (K, V fragments in registers): S = Q K^T and dP = dO V^T (a lane
//                   holds one key and four queries per query tile), P and dS are the A operands of dV[key][d] += P[q][key]
//                   dO[q][d] and dK[key][d] += dS[q][key] Q[q][d].
// S and dP are computed in both passes (7 products instead of 5): the f32 matrix pipe is the bound either way, and nothing
// crosses between waves but delta (written in pass A, read after the one barrier pair between the passes).
// Same k-assignment rule as the forward kernel: lane group g supplies k = 16 c + 4 g + kk in step (c, kk) on both operands.
// ---------------------------------------------------------------------------------------------------------------------
template <int NT>
__global__ __launch_bounds__(512) void attn_bwd_f32_kernel(const float* __restrict__ qkv, const float* __restrict__ out,
                                                           const float* __restrict__ dout, const float* __restrict__ lse,
                                                           float* __restrict__ dqkv, int N, int H, float scale) {
  constexpr int NK = NT * 16;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* const R0 = smem;                    // [NK][64]: K, then Q
  float* const R1 = smem + NK * AF_DH;       // [NK][64]: V, then dO
  float* const sLse = R1 + NK * AF_DH;       // [NK]; +inf for rows >= N (their probabilities are exactly 0)
  float* const sDelta = sLse + NK;           // [NK]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int q16 = lane & 15, g = lane >> 4;
  const float sl2 = scale * AF_LOG2E;
  const int b = blockIdx.x / H, h = blockIdx.x % H;
  const long row = 3L * H * AF_DH, orow = (long)H * AF_DH;
  const float* const qb = qkv + (long)b * N * row + (long)h * AF_DH;
  const float* const kb = qb + orow;
  const float* const vb = kb + orow;
  const float* const ob = out + (long)b * N * orow + (long)h * AF_DH;
  const float* const dob = dout + (long)b * N * orow + (long)h * AF_DH;
  float* const dqb = dqkv + (long)b * N * row + (long)h * AF_DH;

  // rows of two [N][64] operands -> R0, R1 (swizzled 16-byte slots, rows >= N zero); every load of the thread is issued
  // before the first LDS write (see the forward kernel)
  constexpr int NIT = (NK * 16 + 511) / 512;
  auto stage2 = [&](const float* src0, long ld0, const float* src1, long ld1) {
    f32x4 a[NIT], c[NIT];
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int i = tid + 512 * it, r = i >> 4, j = i & 15;
      a[it] = (f32x4){0.f, 0.f, 0.f, 0.f};
      c[it] = (f32x4){0.f, 0.f, 0.f, 0.f};
      if (i < NK * 16 && r < N) {
        a[it] = *reinterpret_cast<const f32x4*>(src0 + r * ld0 + 4 * j);
        c[it] = *reinterpret_cast<const f32x4*>(src1 + r * ld1 + 4 * j);
      }
    }
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int i = tid + 512 * it, r = i >> 4, j = i & 15;
      if (i < NK * 16) {
        *reinterpret_cast<f32x4*>(R0 + r * AF_DH + ((j ^ (r & 15)) << 2)) = a[it];
        *reinterpret_cast<f32x4*>(R1 + r * AF_DH + ((j ^ (r & 15)) << 2)) = c[it];
      }
    }
  };
  // A-operand fragments of the 16 rows of tile T: lane (row q16, group g) gets floats 16 c + 4 g .. + 3
  auto load_rows = [&](f32x4 (&dst)[4], const float* R, int T) {
    const int r = T * 16 + q16;
#pragma unroll
    for (int c = 0; c < 4; ++c) dst[c] = *reinterpret_cast<const f32x4*>(R + r * AF_DH + (((4 * c + g) ^ (r & 15)) << 2));
  };
  // B operand of the products that contract over ROWS: element (row 16 T + 4 g + r, column 16 dt + q16)
  auto elem = [&](const float* R, int T, int r, int dt) -> float {
    const int rr = T * 16 + 4 * g + r, d = 16 * dt + q16;
    return R[rr * AF_DH + ((((d >> 2) ^ (rr & 15)) << 2) | (d & 3))];
  };
  // B-operand fragments of one global row (clamped; masked through lse / key < N)
  auto load_global = [&](f32x4 (&dst)[4], const float* base, long ld, int r) {
    const float* p = base + (long)(r < N ? r : N - 1) * ld + 4 * g;
#pragma unroll
    for (int c = 0; c < 4; ++c) dst[c] = *reinterpret_cast<const f32x4*>(p + 16 * c);
  };

  stage2(kb, row, vb, row);
  for (int i = tid; i < NK; i += 512) {
    sLse[i] = i < N ? lse[((long)b * H + h) * N + i] * AF_LOG2E : INFINITY;     // log2 units, like the scores below
    sDelta[i] = 0.f;
  }
  __syncthreads();

  // ---------------- pass A: dQ ----------------
  for (int qt = wave; qt * 16 < N; qt += 8) {
    const int q = qt * 16 + q16;
    f32x4 qf[4], dof[4], of[4];
    load_global(qf, qb, row, q);
    load_global(dof, dob, orow, q);
    load_global(of, ob, orow, q);
    float dl = 0.f;
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int e = 0; e < 4; ++e) dl += dof[c][e] * of[c][e];
    dl += __shfl_xor(dl, 16, 64);
    dl += __shfl_xor(dl, 32, 64);
    if (g == 0) sDelta[q] = dl;                  // q < NK always; pass B reads it after the barrier
    const float l = sLse[q];
    f32x4 dq[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) dq[dt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    f32x4 kf[4], vf[4], kn[4], vn[4];
    load_rows(kf, R0, 0);
    load_rows(vf, R1, 0);
#pragma unroll 1
    for (int T = 0; T < NT; ++T) {
      if (T + 1 < NT) {
        load_rows(kn, R0, T + 1);
        load_rows(vn, R1, T + 1);
      }
      f32x4 st = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
          st = __builtin_amdgcn_mfma_f32_16x16x4f32(kf[c][kk], qf[c][kk], st, 0, 0, 0);
          dp = __builtin_amdgcn_mfma_f32_16x16x4f32(vf[c][kk], dof[c][kk], dp, 0, 0, 0);
        }
      f32x4 ds;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int key = T * 16 + 4 * g + r;
        const float p = key < N ? __builtin_amdgcn_exp2f(st[r] * sl2 - l) : 0.f;
        ds[r] = p * (dp[r] - dl) * scale;
      }
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) dq[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(ds[r], elem(R0, T, r, dt), dq[dt], 0, 0, 0);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        kf[c] = kn[c];
        vf[c] = vn[c];
      }
    }
    // dq[dt][r] = dQ(query 16 qt + 4 g + r, feature 16 dt + q16)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int qq = qt * 16 + 4 * g + r;
      if (qq < N) {
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) dqb[(long)qq * row + 16 * dt + q16] = dq[dt][r];
      }
    }
  }

  // ---------------- the same LDS bytes now hold Q and dO ----------------
  __syncthreads();
  stage2(qb, row, dob, orow);
  __syncthreads();

  // ---------------- pass B: dK, dV ----------------
  for (int kt = wave; kt * 16 < N; kt += 8) {
    const int key = kt * 16 + q16;
    f32x4 kf[4], vf[4];
    load_global(kf, kb, row, key);
    load_global(vf, vb, row, key);
    f32x4 dk[4], dv[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      dk[dt] = (f32x4){0.f, 0.f, 0.f, 0.f};
      dv[dt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
    f32x4 qa[4], da[4], qn[4], dn[4];
    load_rows(qa, R0, 0);
    load_rows(da, R1, 0);
#pragma unroll 1
    for (int T = 0; T < NT; ++T) {
      if (T + 1 < NT) {
        load_rows(qn, R0, T + 1);
        load_rows(dn, R1, T + 1);
      }
      const f32x4 l4 = *reinterpret_cast<const f32x4*>(sLse + T * 16 + 4 * g);
      const f32x4 d4 = *reinterpret_cast<const f32x4*>(sDelta + T * 16 + 4 * g);
      f32x4 sv = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
          sv = __builtin_amdgcn_mfma_f32_16x16x4f32(qa[c][kk], kf[c][kk], sv, 0, 0, 0);
          dp = __builtin_amdgcn_mfma_f32_16x16x4f32(da[c][kk], vf[c][kk], dp, 0, 0, 0);
        }
      f32x4 p, ds;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float e = key < N ? __builtin_amdgcn_exp2f(sv[r] * sl2 - l4[r]) : 0.f;   // lse = +inf for padded queries: 0
        p[r] = e;
        ds[r] = e * (dp[r] - d4[r]) * scale;
      }
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
          dv[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(p[r], elem(R1, T, r, dt), dv[dt], 0, 0, 0);
          dk[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(ds[r], elem(R0, T, r, dt), dk[dt], 0, 0, 0);
        }
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        qa[c] = qn[c];
        da[c] = dn[c];
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int kk = kt * 16 + 4 * g + r;
      if (kk < N) {
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
          dqb[(long)kk * row + orow + 16 * dt + q16] = dk[dt][r];
          dqb[(long)kk * row + 2 * orow + 16 * dt + q16] = dv[dt][r];
        }
      }
    }
  }
}

template <int NT>
int launch_attn_bwd_f32(const float* qkv, const float* out, const float* dout, const float* lse, float* dqkv, int B, int N,
                        int H, float scale, hipStream_t s) {
  constexpr size_t lds = ((size_t)2 * NT * 16 * AF_DH + 2 * NT * 16) * sizeof(float);
  return mv_launch<attn_bwd_f32_kernel<NT>>(MV_HERE, B * H, 512, lds, s, qkv, out, dout, lse, dqkv, N, H, scale);
}

template <int NT, bool Q8>
int launch_attn_f32(const float* qkv, void* out, int B, int N, int H, float scale, float q_inv, float q_zp, hipStream_t s,
                    float* lse = nullptr) {
  constexpr size_t lds = (size_t)2 * NT * 16 * AF_DH * sizeof(float);
  const int n_cu = mv_cu_count();                         // of the current device (one cached value per device)
  const int items = B * H;
  return mv_launch<attn_fwd_f32_kernel<NT, Q8>>(MV_HERE, items < n_cu ? items : n_cu, 512, lds, s, qkv, (float*)out, N, H, scale,
                                                q_inv, q_zp, lse, items);
}

// ---------------------------------------------------------------------------------------------------------------------
// N > 272: key-tiled kernels of the same core (mv_attention_fwd_long_f32 / _q8, mv_attention_bwd_long_f32), any 1 <= N <= 8192
// ---------------------------------------------------------------------------------------------------------------------
// The kernels above hold a head's whole K and V^T in LDS and stop at 272 tokens; at 577 (384^2 fine-tuning) or 1 025 (512^2
// segmentation) the fp32 and bf16x3 modes fell back to the materialised path and its [B, H, N, N] probability tensor.  Here the
// operands that are swept stream through LDS in 64-row blocks, a two-stage ring loaded one block ahead (the global loads are
// issued before a block's products, written to the other stage after them, one barrier per block), and nothing of size N^2
// exists.  A workgroup is 8 waves that each own one 16-row tile: 128 queries (forward, dQ) or keys (dK / dV).
//   forward : S^T = K_blk Q^T and O^T = V^T_blk P^T in the orientation of attn_fwd_f32_kernel (a lane holds one query; P is the
//             B operand straight from the registers), with an online softmax in fp32: running maximum m, lane-local running sum,
//             O^T *= exp2(m_old - m_new) per block, O divided by the sum once at the end.  Keys >= N of the last block are -inf.
//             The 64-key V^T block has K's row length, so it takes K's slot swizzle (XOR with row & 15): its fragment reads are
//             then exactly the K reads, conflict-free under the b128 rules (vt_sw above is for rows of NK = 208 / 272 floats).
//   dK / dV : a wave owns 16 keys (K, V fragments and dK, dV accumulators in registers) and sweeps the query blocks (Q, dO in
//             LDS): pass B of attn_bwd_f32_kernel, with lse and delta of the block staged beside them.
//   dQ      : a wave owns 16 queries (Q, dO fragments in registers) and sweeps the key blocks (K, V in LDS): its pass A.
// delta = rowsum(dO * O) comes from attn_delta_long_f32_kernel (workspace [B, H, N]).  Every output element has one owner:
// no atomics, bitwise reproducible.  The rows contracted in dV, dK and dQ are read from the row-major images as 4-byte LDS
// loads (attn_bwd_f32_kernel's elem): at the f32 matrix rate one ds_read_b32 per MFMA is free, and nothing is transposed.
constexpr int LF_MAX_N = 8192;
constexpr int LF_ROWS = 128;                  // queries / keys owned by a workgroup (8 waves x 16)
constexpr int LF_BLK = 64;                    // rows per streamed block
constexpr int LF_STAGE = 2 * LF_BLK * AF_DH;  // floats per ring stage: two [64][64] fp32 images = 32 KiB
constexpr int LF_OUT_PLAIN = 0, LF_OUT_LSE = 1, LF_OUT_Q8 = 2;

// rows row0 .. row0 + 63 of a [*, ld] fp32 tensor (64 features at src): two 16-byte pieces per thread, zero past N
__device__ __forceinline__ void lf_load_rows(f32x4 (&dst)[2], const float* src, long ld, int row0, int N, int tid) {
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const int i = tid + 512 * it, r = row0 + (i >> 4);
    dst[it] = (f32x4){0.f, 0.f, 0.f, 0.f};
    if (r < N) dst[it] = *reinterpret_cast<const f32x4*>(src + (long)r * ld + 4 * (i & 15));
  }
}
// ... into a [64][64] image with the 16-byte slot XORed with row & 15 (the K image of attn_fwd_f32_kernel)
__device__ __forceinline__ void lf_write_rows(float* dst, const f32x4 (&v)[2], int tid) {
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const int i = tid + 512 * it, r = i >> 4, j = i & 15;
    *reinterpret_cast<f32x4*>(dst + r * AF_DH + ((j ^ (r & 15)) << 2)) = v[it];
  }
}
// A-operand fragments of the 16 rows of tile T of a row image: lane (row q16, group g) gets floats 16 c + 4 g .. + 3
__device__ __forceinline__ void lf_frag_rows(f32x4 (&dst)[4], const float* R, int T, int q16, int g) {
  const int r = T * 16 + q16;
#pragma unroll
  for (int c = 0; c < 4; ++c) dst[c] = *reinterpret_cast<const f32x4*>(R + r * AF_DH + (((4 * c + g) ^ (r & 15)) << 2));
}
// B operand of the products that contract over ROWS of a row image: element (row 16 T + 4 g + r, column 16 dt + q16)
__device__ __forceinline__ float lf_elem(const float* R, int T, int r, int dt, int q16, int g) {
  const int rr = T * 16 + 4 * g + r, d = 16 * dt + q16;
  return R[rr * AF_DH + ((((d >> 2) ^ (rr & 15)) << 2) | (d & 3))];
}

template <int OUT>
__global__ __launch_bounds__(512) void attn_fwd_long_f32_kernel(const float* __restrict__ qkv, void* __restrict__ out,
                                                                float* __restrict__ lse, int N, int H, int nqb, float sl2,
                                                                float q_inv, float q_zp) {
  extern __shared__ __attribute__((aligned(16))) float smem[];     // stage s: K [64][64] | V^T [64][64]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, q16 = lane & 15, g = lane >> 4;
  const int bh = blockIdx.x / nqb, qblk = blockIdx.x % nqb;
  const int b = bh / H, h = bh % H;
  const long row = 3L * H * AF_DH, orow = (long)H * AF_DH;
  const float* const qb = qkv + (long)b * N * row + (long)h * AF_DH;
  const float* const kb = qb + orow;
  const float* const vb = kb + orow;
  const int nkb = (N + LF_BLK - 1) / LF_BLK;

  // K rows as lf_load_rows; V with the lanes walking the keys, so that the transposed LDS writes are conflict-free
  f32x4 kst[2], vst[2];
  auto issue = [&](int blk) {
    lf_load_rows(kst, kb, row, blk * LF_BLK, N, tid);
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      const int i = tid + 512 * it, key = blk * LF_BLK + (i & 63);
      vst[it] = (f32x4){0.f, 0.f, 0.f, 0.f};
      if (key < N) vst[it] = *reinterpret_cast<const f32x4*>(vb + (long)key * row + 4 * (i >> 6));
    }
  };
  auto write = [&](int blk) {
    float* const Ks = smem + (blk & 1) * LF_STAGE;
    float* const Vt = Ks + LF_BLK * AF_DH;
    lf_write_rows(Ks, kst, tid);
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      const int i = tid + 512 * it, key = i & 63, j = i >> 6;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int d = 4 * j + e;
        Vt[d * LF_BLK + (((key >> 2) ^ (d & 15)) << 2) + (key & 3)] = vst[it][e];
      }
    }
  };
  issue(0);
  write(0);

  const int q0 = qblk * LF_ROWS + 16 * wave, q = q0 + q16;
  const bool active = q0 < N;                  // wave-uniform; an idle wave still stages and meets the barriers
  f32x4 qf[4];
  {
    const float* qrow = qb + (long)(q < N ? q : N - 1) * row + 4 * g;     // clamped: rows >= N are never stored
#pragma unroll
    for (int c = 0; c < 4; ++c) qf[c] = *reinterpret_cast<const f32x4*>(qrow + 16 * c);
  }
  f32x4 o[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) o[dt] = (f32x4){0.f, 0.f, 0.f, 0.f};
  float m = -INFINITY, l = 0.f;                // l: this lane's share of the running sum (its four keys per tile)
  __syncthreads();

  for (int blk = 0; blk < nkb; ++blk) {
    const bool has_next = blk + 1 < nkb;       // workgroup-uniform
    if (has_next) issue(blk + 1);
    if (active) {
      const float* const Ks = smem + (blk & 1) * LF_STAGE;
      const float* const Vt = Ks + LF_BLK * AF_DH;
      // ---- S^T = K Q^T: st[T][r] = score of (query q, key 64 blk + 16 T + 4 g + r), in log2 units
      f32x4 st[4];
#pragma unroll
      for (int T = 0; T < 4; ++T) {
        f32x4 kf[4];
        lf_frag_rows(kf, Ks, T, q16, g);
        st[T] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
          for (int kk = 0; kk < 4; ++kk) st[T] = __builtin_amdgcn_mfma_f32_16x16x4f32(kf[c][kk], qf[c][kk], st[T], 0, 0, 0);
      }
      // ---- online softmax
      float mb = -INFINITY;
#pragma unroll
      for (int T = 0; T < 4; ++T)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int key = blk * LF_BLK + T * 16 + 4 * g + r;
          const float x = key < N ? st[T][r] * sl2 : -INFINITY;
          st[T][r] = x;
          mb = fmaxf(mb, x);
        }
      mb = fmaxf(mb, __shfl_xor(mb, 16, 64));
      mb = fmaxf(mb, __shfl_xor(mb, 32, 64));
      const float mn = fmaxf(m, mb);           // finite: block 0 holds key 0
      const float alpha = __builtin_amdgcn_exp2f(m - mn);      // exp2(-inf) = 0 on the first block
      m = mn;
      float s = l * alpha;
#pragma unroll
      for (int T = 0; T < 4; ++T)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float p = __builtin_amdgcn_exp2f(st[T][r] - mn);     // 0 for the keys past N
          st[T][r] = p;
          s += p;
        }
      l = s;
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) o[dt] *= alpha;
      // ---- O^T += V^T P^T: o[dt][r] = out(query q, feature 16 dt + 4 g + r)
#pragma unroll
      for (int T = 0; T < 4; ++T) {
        f32x4 vf[4];
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
          const int d = dt * 16 + q16;
          vf[dt] = *reinterpret_cast<const f32x4*>(Vt + d * LF_BLK + (((4 * T + g) ^ (d & 15)) << 2));
        }
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int dt = 0; dt < 4; ++dt) o[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(vf[dt][r], st[T][r], o[dt], 0, 0, 0);
      }
    }
    if (has_next) write(blk + 1);              // the stage every wave finished reading before the last barrier
    __syncthreads();
  }
  if (!active) return;
  float s = l;
  s += __shfl_xor(s, 16, 64);
  s += __shfl_xor(s, 32, 64);
  const float inv = 1.0f / s;
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) o[dt] *= inv;
  if (q < N) {
    if constexpr (OUT == LF_OUT_Q8) {
      int8_t* op = reinterpret_cast<int8_t*>(out) + ((long)b * N + q) * orow + (long)h * AF_DH + 4 * g;
#pragma unroll
      for (int dt = 0; dt < 4; ++dt)
        *reinterpret_cast<unsigned*>(op + 16 * dt) = affine_i8_pack4<0>(o[dt][0], o[dt][1], o[dt][2], o[dt][3], q_inv, q_zp);
    } else {
      float* op = reinterpret_cast<float*>(out) + ((long)b * N + q) * orow + (long)h * AF_DH + 4 * g;
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) *reinterpret_cast<f32x4*>(op + 16 * dt) = o[dt];
      if (OUT == LF_OUT_LSE && g == 0) lse[((long)b * H + h) * N + q] = (m + __builtin_amdgcn_logf(s)) * AF_LN2;
    }
  }
}

// delta[b, h, n] = sum_d dO[b, n, h, d] O[b, n, h, d] in fp32: 16 consecutive threads per (token, head), a fixed shuffle tree
__global__ __launch_bounds__(256) void attn_delta_long_f32_kernel(const float* __restrict__ out, const float* __restrict__ dout,
                                                                  float* __restrict__ delta, long rows, int N, int H) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;     // = ((b N + n) H + h) 16 + chunk
  const long rh = idx >> 4;
  float d = 0.f;
  if (rh < rows) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(dout + idx * 4), o = *reinterpret_cast<const f32x4*>(out + idx * 4);
    d = a[0] * o[0] + a[1] * o[1] + a[2] * o[2] + a[3] * o[3];
  }
  d += __shfl_xor(d, 1, 64);
  d += __shfl_xor(d, 2, 64);
  d += __shfl_xor(d, 4, 64);
  d += __shfl_xor(d, 8, 64);
  if (rh < rows && (idx & 15) == 0) {
    const long bn = rh / H;
    const int h = (int)(rh % H);
    const long b = bn / N, n = bn % N;
    delta[(b * H + h) * N + n] = d;
  }
}

__global__ __launch_bounds__(512) void attn_bwd_dkdv_long_f32_kernel(const float* __restrict__ qkv, const float* __restrict__ dout,
                                                                     const float* __restrict__ lse, const float* __restrict__ delta,
                                                                     float* __restrict__ dqkv, int N, int H, int nkb, float scale) {
  extern __shared__ __attribute__((aligned(16))) float smem[];     // stage s: Q [64][64] | dO [64][64]; then sRow
  float* const sRow = smem + 2 * LF_STAGE;                         // [stage][lse * log2(e) (+inf past N) | delta (0 past N)][64]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, q16 = lane & 15, g = lane >> 4;
  const int bh = blockIdx.x / nkb, kblk = blockIdx.x % nkb;
  const int b = bh / H, h = bh % H;
  const long row = 3L * H * AF_DH, orow = (long)H * AF_DH;
  const float* const qb = qkv + (long)b * N * row + (long)h * AF_DH;
  const float* const kb = qb + orow;
  const float* const vb = kb + orow;
  const float* const dob = dout + (long)b * N * orow + (long)h * AF_DH;
  const float* const lrow = lse + ((long)b * H + h) * N;
  const float* const drow = delta + ((long)b * H + h) * N;
  float* const dkb = dqkv + (long)b * N * row + (long)h * AF_DH + orow;
  const float sl2 = scale * AF_LOG2E;
  const int nqb = (N + LF_BLK - 1) / LF_BLK;

  f32x4 qst[2], dst[2];
  float rst = 0.f;                             // threads 0..63: the block's lse, 64..127: its delta
  auto issue = [&](int blk) {
    lf_load_rows(qst, qb, row, blk * LF_BLK, N, tid);
    lf_load_rows(dst, dob, orow, blk * LF_BLK, N, tid);
    const int qq = blk * LF_BLK + (tid & 63);
    if (tid < 64) rst = qq < N ? lrow[qq] * AF_LOG2E : INFINITY;   // log2 units, like the scores below
    else if (tid < 128) rst = qq < N ? drow[qq] : 0.f;
  };
  auto write = [&](int blk) {
    float* const Qs = smem + (blk & 1) * LF_STAGE;
    lf_write_rows(Qs, qst, tid);
    lf_write_rows(Qs + LF_BLK * AF_DH, dst, tid);
    if (tid < 128) sRow[(blk & 1) * 2 * LF_BLK + tid] = rst;
  };
  issue(0);
  write(0);

  const int k0 = kblk * LF_ROWS + 16 * wave, key = k0 + q16;
  const bool active = k0 < N;                  // wave-uniform
  f32x4 kf[4], vf[4];
  {
    const long kr = key < N ? key : N - 1;     // clamped: masked below, never stored
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      kf[c] = *reinterpret_cast<const f32x4*>(kb + kr * row + 16 * c + 4 * g);
      vf[c] = *reinterpret_cast<const f32x4*>(vb + kr * row + 16 * c + 4 * g);
    }
  }
  f32x4 dk[4], dv[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) {
    dk[dt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    dv[dt] = (f32x4){0.f, 0.f, 0.f, 0.f};
  }
  __syncthreads();

  for (int blk = 0; blk < nqb; ++blk) {
    const bool has_next = blk + 1 < nqb;
    if (has_next) issue(blk + 1);
    if (active) {
      const float* const Qs = smem + (blk & 1) * LF_STAGE;
      const float* const Ds = Qs + LF_BLK * AF_DH;
      const float* const sL = sRow + (blk & 1) * 2 * LF_BLK;
      const float* const sD = sL + LF_BLK;
#pragma unroll 1
      for (int T = 0; T < 4; ++T) {            // 16-query tiles of the block
        f32x4 qa[4], da[4];
        lf_frag_rows(qa, Qs, T, q16, g);
        lf_frag_rows(da, Ds, T, q16, g);
        // sv[r] = S(query 16 T + 4 g + r, key), dp[r] = dP(same)
        f32x4 sv = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
          for (int kk = 0; kk < 4; ++kk) {
            sv = __builtin_amdgcn_mfma_f32_16x16x4f32(qa[c][kk], kf[c][kk], sv, 0, 0, 0);
            dp = __builtin_amdgcn_mfma_f32_16x16x4f32(da[c][kk], vf[c][kk], dp, 0, 0, 0);
          }
        const f32x4 l4 = *reinterpret_cast<const f32x4*>(sL + T * 16 + 4 * g);
        const f32x4 d4 = *reinterpret_cast<const f32x4*>(sD + T * 16 + 4 * g);
        f32x4 p, ds;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float e = key < N ? __builtin_amdgcn_exp2f(sv[r] * sl2 - l4[r]) : 0.f;   // lse = +inf past N: 0
          p[r] = e;
          ds[r] = e * (dp[r] - d4[r]) * scale;
        }
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int dt = 0; dt < 4; ++dt) {
            dv[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(p[r], lf_elem(Ds, T, r, dt, q16, g), dv[dt], 0, 0, 0);
            dk[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(ds[r], lf_elem(Qs, T, r, dt, q16, g), dk[dt], 0, 0, 0);
          }
      }
    }
    if (has_next) write(blk + 1);
    __syncthreads();
  }
  // dk[dt][r] = dK(key k0 + 4 g + r, feature 16 dt + q16); dV likewise, D floats further on
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int kk = k0 + 4 * g + r;
    if (kk < N) {
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        dkb[(long)kk * row + 16 * dt + q16] = dk[dt][r];
        dkb[(long)kk * row + orow + 16 * dt + q16] = dv[dt][r];
      }
    }
  }
}

__global__ __launch_bounds__(512) void attn_bwd_dq_long_f32_kernel(const float* __restrict__ qkv, const float* __restrict__ dout,
                                                                   const float* __restrict__ lse, const float* __restrict__ delta,
                                                                   float* __restrict__ dqkv, int N, int H, int nqb, float scale) {
  extern __shared__ __attribute__((aligned(16))) float smem[];     // stage s: K [64][64] | V [64][64]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, q16 = lane & 15, g = lane >> 4;
  const int bh = blockIdx.x / nqb, qblk = blockIdx.x % nqb;
  const int b = bh / H, h = bh % H;
  const long row = 3L * H * AF_DH, orow = (long)H * AF_DH;
  const float* const qb = qkv + (long)b * N * row + (long)h * AF_DH;
  const float* const kb = qb + orow;
  const float* const vb = kb + orow;
  const float* const dob = dout + (long)b * N * orow + (long)h * AF_DH;
  float* const dqb = dqkv + (long)b * N * row + (long)h * AF_DH;
  const float sl2 = scale * AF_LOG2E;
  const int nkb = (N + LF_BLK - 1) / LF_BLK;

  f32x4 kst[2], vst[2];
  auto issue = [&](int blk) {
    lf_load_rows(kst, kb, row, blk * LF_BLK, N, tid);
    lf_load_rows(vst, vb, row, blk * LF_BLK, N, tid);
  };
  auto write = [&](int blk) {
    float* const Ks = smem + (blk & 1) * LF_STAGE;
    lf_write_rows(Ks, kst, tid);
    lf_write_rows(Ks + LF_BLK * AF_DH, vst, tid);
  };
  issue(0);
  write(0);

  const int q0 = qblk * LF_ROWS + 16 * wave, q = q0 + q16;
  const bool active = q0 < N;                  // wave-uniform
  const long qr = q < N ? q : N - 1;           // clamped: rows >= N are never stored
  f32x4 qf[4], dof[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    qf[c] = *reinterpret_cast<const f32x4*>(qb + qr * row + 16 * c + 4 * g);
    dof[c] = *reinterpret_cast<const f32x4*>(dob + qr * orow + 16 * c + 4 * g);
  }
  const float l = lse[((long)b * H + h) * N + qr] * AF_LOG2E;
  const float dl = delta[((long)b * H + h) * N + qr];
  f32x4 dq[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) dq[dt] = (f32x4){0.f, 0.f, 0.f, 0.f};
  __syncthreads();

  for (int blk = 0; blk < nkb; ++blk) {
    const bool has_next = blk + 1 < nkb;
    if (has_next) issue(blk + 1);
    if (active) {
      const float* const Ks = smem + (blk & 1) * LF_STAGE;
      const float* const Vs = Ks + LF_BLK * AF_DH;
#pragma unroll 1
      for (int T = 0; T < 4; ++T) {            // 16-key tiles of the block
        f32x4 ka[4], va[4];
        lf_frag_rows(ka, Ks, T, q16, g);
        lf_frag_rows(va, Vs, T, q16, g);
        // st[r] = S(query q, key 64 blk + 16 T + 4 g + r), dp[r] = dP(same)
        f32x4 st = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
          for (int kk = 0; kk < 4; ++kk) {
            st = __builtin_amdgcn_mfma_f32_16x16x4f32(ka[c][kk], qf[c][kk], st, 0, 0, 0);
            dp = __builtin_amdgcn_mfma_f32_16x16x4f32(va[c][kk], dof[c][kk], dp, 0, 0, 0);
          }
        f32x4 ds;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int key = blk * LF_BLK + T * 16 + 4 * g + r;
          const float p = key < N ? __builtin_amdgcn_exp2f(st[r] * sl2 - l) : 0.f;
          ds[r] = p * (dp[r] - dl) * scale;
        }
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int dt = 0; dt < 4; ++dt)
            dq[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(ds[r], lf_elem(Ks, T, r, dt, q16, g), dq[dt], 0, 0, 0);
      }
    }
    if (has_next) write(blk + 1);
    __syncthreads();
  }
  // dq[dt][r] = dQ(query q0 + 4 g + r, feature 16 dt + q16)
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int qq = q0 + 4 * g + r;
    if (qq < N) {
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) dqb[(long)qq * row + 16 * dt + q16] = dq[dt][r];
    }
  }
}

template <int OUT>
int launch_attn_fwd_long_f32(const float* qkv, void* out, float* lse, int B, int N, int H, float scale, float q_inv,
                             float q_zp, hipStream_t s) {
  constexpr int lds = 2 * LF_STAGE * (int)sizeof(float);
  const long nqb = (N + LF_ROWS - 1) / LF_ROWS;
  return mv_launch<attn_fwd_long_f32_kernel<OUT>>(MV_HERE, (unsigned)(nqb * B * H), 512, lds, s, qkv, out, lse, N, H, (int)nqb,
                                                  scale * AF_LOG2E, q_inv, q_zp);
}

}  // namespace

extern "C" int mv_attention_fwd_f32(const float* qkv, float* out, int B, int N, int H, float scale, mv_stream_t stream) {
  MV_REQUIRE(B >= 0 && N > 0 && H > 0 && (long)B * H < (1L << 31), MV_ERR_SHAPE);
  MV_REQUIRE(N <= 272, MV_ERR_UNSUPPORTED);
  MV_REQUIRE(mv_aligned16(qkv) && mv_aligned16(out), MV_ERR_ALIGN);
  if (B == 0) return MV_OK;
  hipStream_t s = (hipStream_t)stream;
  return N <= 208 ? launch_attn_f32<13, false>(qkv, out, B, N, H, scale, 0.f, 0.f, s)
                  : launch_attn_f32<17, false>(qkv, out, B, N, H, scale, 0.f, 0.f, s);
}

extern "C" int mv_attention_fwd_f32_q8(const float* qkv, void* codes, int B, int N, int H, float scale, float q_scale,
                                       int q_zero_point, mv_stream_t stream) {
  MV_REQUIRE(B >= 0 && N > 0 && H > 0 && (long)B * H < (1L << 31) && q_scale > 0.f, MV_ERR_SHAPE);
  MV_REQUIRE(N <= 272 && q_zero_point >= 0 && q_zero_point <= 255, MV_ERR_UNSUPPORTED);
  MV_REQUIRE(mv_aligned16(qkv) && mv_aligned16(codes), MV_ERR_ALIGN);
  if (B == 0) return MV_OK;
  hipStream_t s = (hipStream_t)stream;
  const float inv = 1.0f / q_scale, fz = (float)q_zero_point;
  return N <= 208 ? launch_attn_f32<13, true>(qkv, codes, B, N, H, scale, inv, fz, s)
                  : launch_attn_f32<17, true>(qkv, codes, B, N, H, scale, inv, fz, s);
}

extern "C" int mv_attention_fwd_f32_lse(const float* qkv, float* out, float* lse, int B, int N, int H, float scale,
                                        mv_stream_t stream) {
  MV_REQUIRE(B >= 0 && N > 0 && H > 0 && (long)B * H < (1L << 31), MV_ERR_SHAPE);
  MV_REQUIRE(N <= 272, MV_ERR_UNSUPPORTED);
  MV_REQUIRE(mv_aligned16(qkv) && mv_aligned16(out) && lse, MV_ERR_ALIGN);
  if (B == 0) return MV_OK;
  hipStream_t s = (hipStream_t)stream;
  return N <= 208 ? launch_attn_f32<13, false>(qkv, out, B, N, H, scale, 0.f, 0.f, s, lse)
                  : launch_attn_f32<17, false>(qkv, out, B, N, H, scale, 0.f, 0.f, s, lse);
}

extern "C" int mv_attention_bwd_f32(const float* qkv, const float* out, const float* dout, const float* lse, float* dqkv,
                                    int B, int N, int H, float scale, mv_stream_t stream) {
  MV_REQUIRE(B >= 0 && N > 0 && H > 0 && (long)B * H < (1L << 31), MV_ERR_SHAPE);
  MV_REQUIRE(N <= 272, MV_ERR_UNSUPPORTED);
  MV_REQUIRE(mv_aligned16(qkv) && mv_aligned16(out) && mv_aligned16(dout) && mv_aligned16(dqkv) && lse, MV_ERR_ALIGN);
  if (B == 0) return MV_OK;
  hipStream_t s = (hipStream_t)stream;
  return N <= 208 ? launch_attn_bwd_f32<13>(qkv, out, dout, lse, dqkv, B, N, H, scale, s)
                  : launch_attn_bwd_f32<17>(qkv, out, dout, lse, dqkv, B, N, H, scale, s);
}

// ---------------------------------------------------------------------------------------------------------------------
// any 1 <= N <= 8192: the key-tiled kernels (ops.attention_fwd_f32 / _f32_lse / _f32_q8 / attention_bwd_f32_fused route N > 272 here)
// ---------------------------------------------------------------------------------------------------------------------
extern "C" int mv_attention_fwd_long_f32(const float* qkv, float* out, float* lse, int B, int N, int H, float scale,
                                         mv_stream_t stream) {
  MV_REQUIRE(B >= 0 && N > 0 && H > 0, MV_ERR_SHAPE);
  MV_REQUIRE(N <= LF_MAX_N, MV_ERR_UNSUPPORTED);
  MV_REQUIRE((long)(N + LF_ROWS - 1) / LF_ROWS * B * H < (1L << 31), MV_ERR_SHAPE);
  MV_REQUIRE(mv_aligned16(qkv) && mv_aligned16(out), MV_ERR_ALIGN);
  if (B == 0) return MV_OK;
  hipStream_t s = (hipStream_t)stream;
  return lse ? launch_attn_fwd_long_f32<LF_OUT_LSE>(qkv, out, lse, B, N, H, scale, 0.f, 0.f, s)
             : launch_attn_fwd_long_f32<LF_OUT_PLAIN>(qkv, out, nullptr, B, N, H, scale, 0.f, 0.f, s);
}

extern "C" int mv_attention_fwd_long_f32_q8(const float* qkv, void* codes, int B, int N, int H, float scale, float q_scale,
                                            int q_zero_point, mv_stream_t stream) {
  MV_REQUIRE(B >= 0 && N > 0 && H > 0 && q_scale > 0.f, MV_ERR_SHAPE);
  MV_REQUIRE(N <= LF_MAX_N && q_zero_point >= 0 && q_zero_point <= 255, MV_ERR_UNSUPPORTED);
  MV_REQUIRE((long)(N + LF_ROWS - 1) / LF_ROWS * B * H < (1L << 31), MV_ERR_SHAPE);
  MV_REQUIRE(mv_aligned16(qkv) && mv_aligned16(codes), MV_ERR_ALIGN);
  if (B == 0) return MV_OK;
  return launch_attn_fwd_long_f32<LF_OUT_Q8>(qkv, codes, nullptr, B, N, H, scale, 1.0f / q_scale, (float)q_zero_point,
                                             (hipStream_t)stream);
}

extern "C" int mv_attention_bwd_long_f32(const float* qkv, const float* out, const float* dout, const float* lse, float* delta_ws,
                                         float* dqkv, int B, int N, int H, float scale, mv_stream_t stream) {
  MV_REQUIRE(B >= 0 && N > 0 && H > 0, MV_ERR_SHAPE);
  MV_REQUIRE(N <= LF_MAX_N, MV_ERR_UNSUPPORTED);
  const long nb = (N + LF_ROWS - 1) / LF_ROWS, rows = (long)B * N * H;
  MV_REQUIRE(nb * B * H < (1L << 31) && (rows * 16 + 255) / 256 < (1L << 31), MV_ERR_SHAPE);
  MV_REQUIRE(mv_aligned16(qkv) && mv_aligned16(out) && mv_aligned16(dout) && mv_aligned16(dqkv) && lse && delta_ws, MV_ERR_ALIGN);
  if (B == 0) return MV_OK;
  hipStream_t s = (hipStream_t)stream;
  constexpr int lds_dkdv = (2 * LF_STAGE + 4 * LF_BLK) * (int)sizeof(float), lds_dq = 2 * LF_STAGE * (int)sizeof(float);
  const unsigned grid = (unsigned)(nb * B * H);
  if (int rc = mv_launch<attn_delta_long_f32_kernel>(MV_HERE, (unsigned)((rows * 16 + 255) / 256), 256, 0, s, out, dout, delta_ws, rows, N, H))
    return rc;
  const int rc = mv_launch<attn_bwd_dkdv_long_f32_kernel>(MV_HERE, grid, 512, lds_dkdv, s, qkv, dout, lse, delta_ws, dqkv, N, H, (int)nb, scale);
  if (rc != MV_OK) return rc;
  return mv_launch<attn_bwd_dq_long_f32_kernel>(MV_HERE, grid, 512, lds_dq, s, qkv, dout, lse, delta_ws, dqkv, N, H, (int)nb, scale);
}
