// Fused bf16 attention core for head widths other than 64: dim_head 32 and 128, any 1 <= N <= 8 192 (reference: Attention.forward
// vit.py:85-99 with the dim_head constructor argument; attention.hip holds the 64-wide kernels and the derivations).
//
// These are the key-tiled kernels of attention.hip (attn_fwd_long_kernel<false>, attn_bwd_dkdv_long_kernel<false>,
// attn_bwd_dq_long_kernel<false>) with the feature width DH a template parameter: K / V (forward, dQ) or Q / dO (dK / dV) stream
// through a two-stage LDS ring in 64-row blocks filled by LDS-DMA one block ahead, the softmax is online in fp32 on exp2 with
// scale * log2(e) folded in, P and dS are rounded to bf16 in front of their products, every accumulator is fp32, every output element
// has one owner (S and dP are computed in both backward kernels): no atomics, bitwise reproducible.  Orientations and fragment maps
// are attention.hip's (S^T = K Q^T in the forward and in dQ, S = Q K^T in dK / dV; transposed operands by ds_read_b64_tr_b16 in the
// accumulator's k order).  What the width changes:
//   * the contraction of S and dP has KS = DH / 32 MFMA k-steps and O / dQ / dK / dV have DT = DH / 16 feature tiles; both are
//     compile-time loop bounds, nothing branches on the width at run time;
//   * LDS rows are 2 DH bytes, so the 128-byte-row image does not carry over.  16-byte chunk ch of row r sits at chunk
//     ch ^ swz(r):  DH = 32 (64-byte rows):  swz = ((r >> 2) & 1) << 1;  DH = 128 (256-byte rows): swz = (r & 7) << 1.
//     Both keep ds_read_b128 row fragments (4 cycles) and ds_read_b64_tr_b16 fragments (2 cycles) conflict-free
//     (tools/lds_bank_sim.py, "dh" cases);
//   * rows per wave.  DH = 32: S is ONE MFMA per 16 x 16 tile against 16 exponentials per lane, so the kernels are bound by the
//     softmax arithmetic, not the matrix cores; a wave owns 64 rows (RT = 4 tiles) to halve the barriers and staging per row.
//     DH = 128: a wave owns 32 rows as in the 64-wide kernels.  The forward (O^T: 64 accumulator registers) and dQ fit two waves
//     per SIMD without spilling (225 / 234 VGPRs).  dK / dV holds dK^T and dV^T (128 registers) and the K / V fragments (64) for
//     the whole sweep and does not: it is built for one wave per SIMD, where the compiler keeps the accumulators in the AGPR half
//     of the register file (no scratch in any instantiation: tools/kernel_resources.py).  LDS: a ring stage is 32 KiB, 64 KiB per
//     workgroup, two workgroups per CU.
// Rows >= N: loads are clamped to row N - 1; keys >= N are -inf before the exponential (forward) or p = 0 (backward); queries
// >= N are never stored (forward, dQ) or carry lse = +inf, i.e. p = 0 (dK / dV).
#include "mv_common.h"

namespace {

constexpr float LOG2E = 1.4426950408889634f;
constexpr float LN2 = 0.6931471805599453f;
constexpr int ATTN_DH_MAX_N = 8192;
constexpr int DBLK = 64;     // rows per streamed LDS block

template <int DH>
struct DhCfg {
  static_assert(DH == 32 || DH == 128, "instantiated widths");
  static constexpr int KS = DH / 32;            // MFMA k-steps of a contraction over the features
  static constexpr int DT = DH / 16;            // 16-feature tiles
  static constexpr int RB = 2 * DH;             // bytes per LDS row
  static constexpr int CPR = DH / 8;            // 16-byte chunks per row
  static constexpr int RT = DH == 32 ? 4 : 2;   // 16-row tiles a wave owns
  static constexpr int WGROWS = 4 * 16 * RT;    // rows per workgroup (4 waves)
  static constexpr int TILE = DBLK * RB;        // one [64][DH] image
  static constexpr int STAGE = 2 * TILE;        // one ring stage: two images
  static constexpr int DKDV_WAVES_PER_SIMD = DH == 128 ? 1 : 2;   // launch bound of the dK / dV kernel (forward, dQ: 2)
};

template <int DH>
__device__ __forceinline__ int swz(int row) {
  return DH == 32 ? ((row >> 2) & 1) << 1 : (row & 7) << 1;
}

__device__ __forceinline__ bf16x8 cat8(bf16x4 a, bf16x4 b) { return __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7); }
__device__ __forceinline__ bf16x4 tr_read(const char* p) { return __builtin_amdgcn_ds_read_tr16_b64_v4bf16(LDS_PTR(bf16x4, p)); }
__device__ __forceinline__ bf16x8 pack8(f32x4 a, f32x4 b) {
  bf16x8 r = {(bf16_t)a[0], (bf16_t)a[1], (bf16_t)a[2], (bf16_t)a[3], (bf16_t)b[0], (bf16_t)b[1], (bf16_t)b[2], (bf16_t)b[3]};
  return r;
}
__device__ __forceinline__ bf16x4 pack4(f32x4 a) {
  bf16x4 r = {(bf16_t)a[0], (bf16_t)a[1], (bf16_t)a[2], (bf16_t)a[3]};
  return r;
}
__device__ __forceinline__ f32x4 mma(bf16x8 a, bf16x8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
// attention.hip's 16-byte output stores: after v_permlane16_swap lane group g holds 8 consecutive features of tile j0 + (g & 1),
// from feature 8 (g >> 1).  Every lane of the wave must execute pair16.
__device__ __forceinline__ u32x4 pair16(f32x4 a, f32x4 b) {
  typedef unsigned u32x2_t __attribute__((ext_vector_type(2)));
  const u32x2_t pa = __builtin_bit_cast(u32x2_t, pack4(a)), pb = __builtin_bit_cast(u32x2_t, pack4(b));
  const u32x2_t r0 = __builtin_amdgcn_permlane16_swap(pa[0], pb[0], false, false);
  const u32x2_t r1 = __builtin_amdgcn_permlane16_swap(pa[1], pb[1], false, false);
  return (u32x4){r0[0], r1[0], r0[1], r1[1]};
}
__device__ __forceinline__ int pair16_off(int j0, int g) { return 16 * (j0 + (g & 1)) + 8 * (g >> 1); }

// Per-lane LDS offsets of the fragment reads.  Tile bases are multiples of 16 rows, so swz() depends on the lane only; the k-step
// (4 ks) and the feature tile (2 dt) occupy chunk bits the lane term leaves zero, so they go in with one XOR per read instead of
// one register per (ks, dt).
struct LaneOff {
  int rf;   // row fragment: row (lane & 15), chunk g ^ swz; k-step ks: ^ (ks << 6)
  int tr;   // transposed fragment: row 4 g + q, chunk (p >> 1) ^ swz, + 8 (p & 1); feature tile dt: ^ (dt << 5)
};
template <int DH>
__device__ __forceinline__ LaneOff make_lane_off(int lane) {
  constexpr int RB = DhCfg<DH>::RB;
  const int g = lane >> 4, q = (lane >> 2) & 3, p = lane & 3, r = lane & 15, rt = 4 * g + q;
  LaneOff L;
  L.rf = r * RB + ((g ^ swz<DH>(r)) << 4);
  L.tr = rt * RB + (((p >> 1) ^ swz<DH>(rt)) << 4) + 8 * (p & 1);
  return L;
}
// 8 consecutive features (k-step ks) of row row_base + (lane & 15); row_base % 16 == 0
template <int DH>
__device__ __forceinline__ bf16x8 row_frag(const char* tile, int row_base, const LaneOff& L, int ks) {
  return *reinterpret_cast<const bf16x8*>(tile + row_base * DhCfg<DH>::RB + (L.rf ^ (ks << 6)));
}
// feature (lane & 15) of tile dt; k slots 8 g + e <-> rows row_base + 4 g + e (e < 4), row_base + 16 + 4 g + (e - 4)
template <int DH>
__device__ __forceinline__ bf16x8 tr_frag(const char* tile, int row_base, const LaneOff& L, int dt) {
  const char* p0 = tile + row_base * DhCfg<DH>::RB + (L.tr ^ (dt << 5));
  return cat8(tr_read(p0), tr_read(p0 + 16 * DhCfg<DH>::RB));
}

// rows row0 .. row0 + 63 of a [*, ld] bf16 tensor (DH features from src) -> one swizzled [64][DH] image.  A DMA piece is 1 KiB =
// 1024 / RB whole rows; the waves take pieces round-robin; rows >= N are clamped to N - 1 (masked by the caller).  Hidden from the
// compiler's wait bookkeeping like attention.hip's stage_blk64: the caller's s_waitcnt vmcnt(0) + barrier orders it.
template <int DH>
__device__ __forceinline__ void stage_blk(const bf16_t* src, long ld, int row0, int N, char* dst, int wave, int lane) {
  using C = DhCfg<DH>;
  constexpr int PIECES = C::TILE / 1024, RPP = 1024 / C::RB;
  const int prow = lane / C::CPR, pch = lane % C::CPR;
#pragma unroll
  for (int i = 0; i < PIECES / 4; ++i) {
    const int pc = wave + 4 * i;
    const int row = RPP * pc + prow, gr = row0 + row;
    const long rr = gr < N ? gr : N - 1;
    glds16_hidden(src + rr * ld + (pch ^ swz<DH>(row)) * 8, dst + pc * 1024);
  }
}

// ------------------------------------------------------------------------------------------------
// forward: a wave owns 16 RT queries; per 64-key block S^T = K Q^T, online softmax, O^T += V^T P^T
// ------------------------------------------------------------------------------------------------
template <int DH>
__global__ __launch_bounds__(256, 2) void attn_fwd_dh_kernel(const bf16_t* __restrict__ qkv,
                                                                                    bf16_t* __restrict__ out,
                                                                                    float* __restrict__ lse, int N, int H, int nqb,
                                                                                    float scale_log2e) {
  using C = DhCfg<DH>;
  constexpr int KS = C::KS, DT = C::DT, RT = C::RT;
  extern __shared__ __attribute__((aligned(16))) char smem[];       // stage s: K [64][DH] | V [64][DH]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4;
  const LaneOff L = make_lane_off<DH>(lane);
  const int bh = blockIdx.x / nqb, qb = blockIdx.x % nqb;
  const int b = bh / H, h = bh % H;
  const long D = (long)H * DH;
  const bf16_t* base = qkv + (long)b * N * 3 * D + h * DH;
  const int nkb = (N + DBLK - 1) / DBLK;
  auto stage = [&](int kb) __attribute__((always_inline)) {
    char* s = smem + (kb & 1) * C::STAGE;
    stage_blk<DH>(base + D, 3 * D, kb * DBLK, N, s, wave, lane);
    stage_blk<DH>(base + 2 * D, 3 * D, kb * DBLK, N, s + C::TILE, wave, lane);
  };
  stage(0);
  const int q0 = qb * C::WGROWS + 16 * RT * wave;
  const bool active = q0 < N;                          // wave-uniform; an idle wave still takes part in staging and barriers
  bf16x8 qf[RT][KS];                                   // rows >= N clamped: never stored
#pragma unroll
  for (int t = 0; t < RT; ++t) {
    const int qrow = q0 + 16 * t + (lane & 15);
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
      qf[t][ks] = *reinterpret_cast<const bf16x8*>(base + (long)(qrow < N ? qrow : N - 1) * 3 * D + 32 * ks + 8 * g);
  }
  f32x4 o[RT][DT];
  float m[RT], l[RT];                                  // l: this lane's share of the running sum (its 4 keys per tile)
#pragma unroll
  for (int t = 0; t < RT; ++t) {
    m[t] = -INFINITY;
    l[t] = 0.f;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) o[t][dt] = (f32x4){0.f, 0.f, 0.f, 0.f};
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  for (int kb = 0; kb < nkb; ++kb) {
    const char* sK = smem + (kb & 1) * C::STAGE;
    const char* sV = sK + C::TILE;
    if (kb + 1 < nkb) stage(kb + 1);                   // into the stage every wave finished reading before the last barrier
    if (active) {
      f32x4 st[RT][4];
#pragma unroll
      for (int kt = 0; kt < 4; ++kt) {
        bf16x8 kf[KS];
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) kf[ks] = row_frag<DH>(sK, kt * 16, L, ks);
#pragma unroll
        for (int t = 0; t < RT; ++t) {
          f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int ks = 0; ks < KS; ++ks) acc = mma(kf[ks], qf[t][ks], acc);
          st[t][kt] = acc;
        }
      }
      const bool ragged = (kb + 1) * DBLK > N;         // only the last block can hold keys >= N
#pragma unroll
      for (int t = 0; t < RT; ++t) {
        float mb = -INFINITY;
#pragma unroll
        for (int kt = 0; kt < 4; ++kt)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            float v = st[t][kt][r] * scale_log2e;
            if (ragged) v = kb * DBLK + kt * 16 + 4 * g + r < N ? v : -INFINITY;
            st[t][kt][r] = v;
            mb = fmaxf(mb, v);
          }
        mb = fmaxf(mb, __shfl_xor(mb, 16, 64));
        mb = fmaxf(mb, __shfl_xor(mb, 32, 64));
        const float mn = fmaxf(m[t], mb);              // finite: every block holds at least one key < N
        const float alpha = __builtin_amdgcn_exp2f(m[t] - mn);   // exp2(-inf) = 0 on the first block
        m[t] = mn;
        float s = l[t] * alpha;
#pragma unroll
        for (int kt = 0; kt < 4; ++kt)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float p = __builtin_amdgcn_exp2f(st[t][kt][r] - mn);
            st[t][kt][r] = p;
            s += p;
          }
        l[t] = s;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) o[t][dt] *= alpha;
      }
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        bf16x8 pf[RT];
#pragma unroll
        for (int t = 0; t < RT; ++t) pf[t] = pack8(st[t][2 * u], st[t][2 * u + 1]);
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
          const bf16x8 vf = tr_frag<DH>(sV, 32 * u, L, dt);
#pragma unroll
          for (int t = 0; t < RT; ++t) o[t][dt] = mma(vf, pf[t], o[t][dt]);
        }
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's pieces of block kb + 1 have landed
    __syncthreads();                                   // ... everyone's, and nobody reads stage kb & 1 any more
  }
  if (!active) return;
#pragma unroll
  for (int t = 0; t < RT; ++t) {
    float s = l[t];
    s += __shfl_xor(s, 16, 64);
    s += __shfl_xor(s, 32, 64);
    const float inv = 1.0f / s;
    const int qrow = q0 + 16 * t + (lane & 15);
    bf16_t* orow = out + ((long)b * N + qrow) * D + h * DH;
#pragma unroll
    for (int dp = 0; dp < DT; dp += 2) {
      const u32x4 w = pair16(o[t][dp] * inv, o[t][dp + 1] * inv);     // every lane (lane exchange)
      if (qrow < N) *reinterpret_cast<u32x4*>(orow + pair16_off(dp, g)) = w;
    }
    if (qrow < N && g == 0) lse[((long)b * H + h) * N + qrow] = (m[t] + __builtin_amdgcn_logf(s)) * LN2;
  }
}

// delta[b, h, n] = sum_d dO[b, n, h, d] O[b, n, h, d] in fp32: DH / 8 consecutive threads per (token, head), a fixed shuffle tree
template <int DH>
__global__ __launch_bounds__(256) void attn_delta_dh_kernel(const bf16_t* __restrict__ out, const bf16_t* __restrict__ dout,
                                                            float* __restrict__ delta, long rows, int N, int H) {
  constexpr int CPR = DhCfg<DH>::CPR;
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;     // = ((b N + n) H + h) CPR + chunk
  const long rh = idx / CPR;
  float d = 0.f;
  if (rh < rows) {
    const bf16x8 a = *reinterpret_cast<const bf16x8*>(dout + idx * 8), o = *reinterpret_cast<const bf16x8*>(out + idx * 8);
#pragma unroll
    for (int e = 0; e < 8; ++e) d += (float)a[e] * (float)o[e];
  }
#pragma unroll
  for (int w = 1; w < CPR; w <<= 1) d += __shfl_xor(d, w, 64);
  if (rh < rows && idx % CPR == 0) {
    const long bn = rh / H;
    const int h = (int)(rh % H);
    const long b = bn / N, n = bn % N;
    delta[(b * H + h) * N + n] = d;
  }
}

// ------------------------------------------------------------------------------------------------
// dK / dV: a wave owns 16 RT keys (K, V fragments and dK^T, dV^T accumulators in registers) and sweeps the query blocks
// ------------------------------------------------------------------------------------------------
template <int DH>
__global__ __launch_bounds__(256, DhCfg<DH>::DKDV_WAVES_PER_SIMD) void attn_bwd_dkdv_dh_kernel(
    const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ dout, const float* __restrict__ lse, const float* __restrict__ delta,
    bf16_t* __restrict__ dqkv, int N, int H, int nkb, float scale) {
  using C = DhCfg<DH>;
  constexpr int KS = C::KS, DT = C::DT, KT = C::RT;
  extern __shared__ __attribute__((aligned(16))) char smem[];       // stage s: Q [64][DH] | dO [64][DH]; then sRow
  float* sRow = reinterpret_cast<float*>(smem + 2 * C::STAGE);      // [stage][lse * log2(e) (+inf past N) | delta (0 past N)][64]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4;
  const LaneOff L = make_lane_off<DH>(lane);
  const int bh = blockIdx.x / nkb, kblk = blockIdx.x % nkb;
  const int b = bh / H, h = bh % H;
  const long D = (long)H * DH;
  const bf16_t* base = qkv + (long)b * N * 3 * D + h * DH;
  const bf16_t* dobase = dout + (long)b * N * D + h * DH;
  bf16_t* dbase = dqkv + (long)b * N * 3 * D + h * DH;
  const float* lrow = lse + ((long)b * H + h) * N;
  const float* drow = delta + ((long)b * H + h) * N;
  const float c2 = scale * LOG2E;
  const int nqb = (N + DBLK - 1) / DBLK;
  auto stage = [&](int qb) __attribute__((always_inline)) {
    char* s = smem + (qb & 1) * C::STAGE;
    stage_blk<DH>(base, 3 * D, qb * DBLK, N, s, wave, lane);
    stage_blk<DH>(dobase, D, qb * DBLK, N, s + C::TILE, wave, lane);
  };
  // threads 0..63 carry the block's lse, 64..127 its delta (a register load one block ahead, written before the barrier)
  auto load_row = [&](int qb) -> float {
    const int q = qb * DBLK + (tid & 63);
    if (tid < 64) return q < N ? lrow[q] * LOG2E : INFINITY;
    if (tid < 128) return q < N ? drow[q] : 0.f;
    return 0.f;
  };
  auto put_row = [&](int qb, float v) {
    if (tid < 128) sRow[(qb & 1) * 2 * DBLK + tid] = v;
  };
  stage(0);
  put_row(0, load_row(0));
  const int k0 = kblk * C::WGROWS + 16 * KT * wave;
  const bool active = k0 < N;                          // wave-uniform; an idle wave still takes part in staging and barriers
  bf16x8 kf[KT][KS], vf[KT][KS];
#pragma unroll
  for (int i = 0; i < KT; ++i) {
    const int krow = k0 + 16 * i + (lane & 15);
    const long rr = krow < N ? krow : N - 1;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      kf[i][ks] = *reinterpret_cast<const bf16x8*>(base + rr * 3 * D + D + 32 * ks + 8 * g);
      vf[i][ks] = *reinterpret_cast<const bf16x8*>(base + rr * 3 * D + 2 * D + 32 * ks + 8 * g);
    }
  }
  f32x4 adk[KT][DT], adv[KT][DT];
#pragma unroll
  for (int i = 0; i < KT; ++i)
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
      adk[i][dt] = (f32x4){0.f, 0.f, 0.f, 0.f};
      adv[i][dt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  for (int qb = 0; qb < nqb; ++qb) {
    const char* sQ = smem + (qb & 1) * C::STAGE;
    const char* sDO = sQ + C::TILE;
    const float* sL = sRow + (qb & 1) * 2 * DBLK;
    const float* sD = sL + DBLK;
    float nrow = 0.f;
    if (qb + 1 < nqb) {
      stage(qb + 1);
      nrow = load_row(qb + 1);
    }
    if (active) {
#pragma unroll 1
      for (int u = 0; u < 2; ++u) {                    // 32-query halves of the block
        bf16x8 pf[KT], dsf[KT];                        // P and dS of the half, queries on the k slots
        {
          bf16x8 qrf[2][KS], dorf[2][KS];
          f32x4 l2v[2], dlv[2];
#pragma unroll
          for (int t = 0; t < 2; ++t) {
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
              qrf[t][ks] = row_frag<DH>(sQ, 32 * u + 16 * t, L, ks);
              dorf[t][ks] = row_frag<DH>(sDO, 32 * u + 16 * t, L, ks);
            }
            l2v[t] = *reinterpret_cast<const f32x4*>(sL + 32 * u + 16 * t + 4 * g);
            dlv[t] = *reinterpret_cast<const f32x4*>(sD + 32 * u + 16 * t + 4 * g);
          }
#pragma unroll
          for (int i = 0; i < KT; ++i) {
            const int key = k0 + 16 * i + (lane & 15);
            f32x4 pp[2], ds[2];
#pragma unroll
            for (int t = 0; t < 2; ++t) {
              f32x4 sv = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
              for (int ks = 0; ks < KS; ++ks) {
                sv = mma(qrf[t][ks], kf[i][ks], sv);
                dp = mma(dorf[t][ks], vf[i][ks], dp);
              }
#pragma unroll
              for (int r = 0; r < 4; ++r) {
                float p = __builtin_amdgcn_exp2f(sv[r] * c2 - l2v[t][r]);     // queries >= N: lse = +inf -> p = 0
                p = key < N ? p : 0.f;
                pp[t][r] = p;
                ds[t][r] = p * (dp[r] - dlv[t][r]) * scale;
              }
            }
            pf[i] = pack8(pp[0], pp[1]);
            dsf[i] = pack8(ds[0], ds[1]);
          }
        }
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
          const bf16x8 dotr = tr_frag<DH>(sDO, 32 * u, L, dt), qtr = tr_frag<DH>(sQ, 32 * u, L, dt);
#pragma unroll
          for (int i = 0; i < KT; ++i) {
            adv[i][dt] = mma(dotr, pf[i], adv[i][dt]);
            adk[i][dt] = mma(qtr, dsf[i], adk[i][dt]);
          }
        }
      }
    }
    if (qb + 1 < nqb) put_row(qb + 1, nrow);           // the stage qb + 1 & 1 was last read before the previous barrier
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }
  if (!active) return;
#pragma unroll
  for (int i = 0; i < KT; ++i) {
    const int key = k0 + 16 * i + (lane & 15);
#pragma unroll
    for (int dp = 0; dp < DT; dp += 2) {
      const u32x4 wk = pair16(adk[i][dp], adk[i][dp + 1]), wv = pair16(adv[i][dp], adv[i][dp + 1]);
      if (key < N) {
        *reinterpret_cast<u32x4*>(dbase + (long)key * 3 * D + D + pair16_off(dp, g)) = wk;
        *reinterpret_cast<u32x4*>(dbase + (long)key * 3 * D + 2 * D + pair16_off(dp, g)) = wv;
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------
// dQ: a wave owns 16 RT queries (Q, dO fragments and dQ^T accumulators in registers) and sweeps the key blocks
// ------------------------------------------------------------------------------------------------
template <int DH>
__global__ __launch_bounds__(256, 2) void attn_bwd_dq_dh_kernel(
    const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ dout, const float* __restrict__ lse, const float* __restrict__ delta,
    bf16_t* __restrict__ dqkv, int N, int H, int nqb, float scale) {
  using C = DhCfg<DH>;
  constexpr int KS = C::KS, DT = C::DT, QT = C::RT;
  extern __shared__ __attribute__((aligned(16))) char smem[];       // stage s: K [64][DH] | V [64][DH]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4;
  const LaneOff L = make_lane_off<DH>(lane);
  const int bh = blockIdx.x / nqb, qblk = blockIdx.x % nqb;
  const int b = bh / H, h = bh % H;
  const long D = (long)H * DH;
  const bf16_t* base = qkv + (long)b * N * 3 * D + h * DH;
  const bf16_t* dobase = dout + (long)b * N * D + h * DH;
  bf16_t* dbase = dqkv + (long)b * N * 3 * D + h * DH;
  const float c2 = scale * LOG2E;
  const int nkb = (N + DBLK - 1) / DBLK;
  auto stage = [&](int kb) __attribute__((always_inline)) {
    char* s = smem + (kb & 1) * C::STAGE;
    stage_blk<DH>(base + D, 3 * D, kb * DBLK, N, s, wave, lane);
    stage_blk<DH>(base + 2 * D, 3 * D, kb * DBLK, N, s + C::TILE, wave, lane);
  };
  stage(0);
  const int q0 = qblk * C::WGROWS + 16 * QT * wave;
  const bool active = q0 < N;
  bf16x8 qf[QT][KS], dof[QT][KS];
  float l2[QT], dl[QT];
#pragma unroll
  for (int t = 0; t < QT; ++t) {
    const int qrow = q0 + 16 * t + (lane & 15);
    const long rr = qrow < N ? qrow : N - 1;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      qf[t][ks] = *reinterpret_cast<const bf16x8*>(base + rr * 3 * D + 32 * ks + 8 * g);
      dof[t][ks] = *reinterpret_cast<const bf16x8*>(dobase + rr * D + 32 * ks + 8 * g);
    }
    l2[t] = qrow < N ? lse[((long)b * H + h) * N + rr] * LOG2E : INFINITY;     // padded queries: p = 0, never stored
    dl[t] = qrow < N ? delta[((long)b * H + h) * N + rr] : 0.f;
  }
  f32x4 dq[QT][DT];
#pragma unroll
  for (int t = 0; t < QT; ++t)
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) dq[t][dt] = (f32x4){0.f, 0.f, 0.f, 0.f};
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  for (int kb = 0; kb < nkb; ++kb) {
    const char* sK = smem + (kb & 1) * C::STAGE;
    const char* sV = sK + C::TILE;
    if (kb + 1 < nkb) stage(kb + 1);
    if (active) {
#pragma unroll 1
      for (int u = 0; u < 2; ++u) {                    // 32-key halves of the block
        bf16x8 dsf[QT];                                // dS^T of the half, keys on the k slots
        {
          bf16x8 kr[2][KS], vr[2][KS];
#pragma unroll
          for (int kk = 0; kk < 2; ++kk)
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
              kr[kk][ks] = row_frag<DH>(sK, 32 * u + 16 * kk, L, ks);
              vr[kk][ks] = row_frag<DH>(sV, 32 * u + 16 * kk, L, ks);
            }
#pragma unroll
          for (int t = 0; t < QT; ++t) {
            f32x4 ds[2];
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) {
              f32x4 st = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
              for (int ks = 0; ks < KS; ++ks) {
                st = mma(kr[kk][ks], qf[t][ks], st);
                dp = mma(vr[kk][ks], dof[t][ks], dp);
              }
#pragma unroll
              for (int r = 0; r < 4; ++r) {
                const int key = kb * DBLK + 32 * u + 16 * kk + 4 * g + r;
                const float p = key < N ? __builtin_amdgcn_exp2f(st[r] * c2 - l2[t]) : 0.f;
                ds[kk][r] = p * (dp[r] - dl[t]) * scale;
              }
            }
            dsf[t] = pack8(ds[0], ds[1]);
          }
        }
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
          const bf16x8 ktr = tr_frag<DH>(sK, 32 * u, L, dt);
#pragma unroll
          for (int t = 0; t < QT; ++t) dq[t][dt] = mma(ktr, dsf[t], dq[t][dt]);
        }
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }
  if (!active) return;
#pragma unroll
  for (int t = 0; t < QT; ++t) {
    const int qrow = q0 + 16 * t + (lane & 15);
#pragma unroll
    for (int dp = 0; dp < DT; dp += 2) {
      const u32x4 w = pair16(dq[t][dp], dq[t][dp + 1]);
      if (qrow < N) *reinterpret_cast<u32x4*>(dbase + (long)qrow * 3 * D + pair16_off(dp, g)) = w;
    }
  }
}

// colsum[b][c] = sum_n dqkv[b, n, c] (c < C = 3 H DH) in fp32, in the fixed order of attention.hip's attn_colsum_long_kernel: thread
// (phase = tid >> 5, 8 columns from 8 (tid & 31)) adds rows phase, phase + 8, ...; the eight phase sums are added in order.
__global__ __launch_bounds__(256) void attn_colsum_dh_kernel(const bf16_t* __restrict__ dqkv, float* __restrict__ colsum, int N,
                                                             int C) {
  __shared__ float red[8][256];
  const int tid = threadIdx.x, ph = tid >> 5, c8 = 8 * (tid & 31);
  const int c = blockIdx.x * 256 + c8, b = blockIdx.y;
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (c < C) {
    const bf16_t* p = dqkv + (long)b * N * C + c;
    for (int n = ph; n < N; n += 8) {
      const bf16x8 v = *reinterpret_cast<const bf16x8*>(p + (long)n * C);
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] += (float)v[e];
    }
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) red[ph][c8 + e] = acc[e];
  __syncthreads();
  const int cc = blockIdx.x * 256 + tid;
  if (cc < C) {
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) s += red[k][tid];
    colsum[(long)b * C + cc] = s;
  }
}

template <typename K>
int set_smem(K kernel, int bytes) {
  return hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, bytes) == hipSuccess
             ? 0
             : -1;
}

template <int DH>
int launch_fwd(const void* qkv, void* out, float* lse, int B, int N, int H, float scale, hipStream_t s) {
  using C = DhCfg<DH>;
  constexpr int smem = 2 * C::STAGE;
  const long nqb = (N + C::WGROWS - 1) / C::WGROWS;
  MV_REQUIRE(nqb * B * H < (1L << 31), MV_ERR_SHAPE);
  if (MV_ONCE_PER_DEVICE(set_smem(attn_fwd_dh_kernel<DH>, smem))) return MV_ERR_LAUNCH;
  attn_fwd_dh_kernel<DH><<<(unsigned)(nqb * B * H), 256, smem, s>>>((const bf16_t*)qkv, (bf16_t*)out, lse, N, H, (int)nqb,
                                                                    scale * LOG2E);
  MV_CHECK_LAUNCH();
  return MV_OK;
}

template <int DH>
int launch_bwd(const void* qkv, const void* out, const void* dout, const float* lse, float* delta_ws, void* dqkv, float* colsum,
               int B, int N, int H, float scale, hipStream_t s) {
  using C = DhCfg<DH>;
  constexpr int smem_kv = 2 * C::STAGE + 2 * 2 * DBLK * 4, smem_q = 2 * C::STAGE;
  const long nb = (N + C::WGROWS - 1) / C::WGROWS, chunks = (long)B * N * H * C::CPR;
  MV_REQUIRE(nb * B * H < (1L << 31) && (chunks + 255) / 256 < (1L << 31) && B < 65536, MV_ERR_SHAPE);
  if (MV_ONCE_PER_DEVICE(set_smem(attn_bwd_dkdv_dh_kernel<DH>, smem_kv) | set_smem(attn_bwd_dq_dh_kernel<DH>, smem_q)))
    return MV_ERR_LAUNCH;
  attn_delta_dh_kernel<DH><<<(unsigned)((chunks + 255) / 256), 256, 0, s>>>((const bf16_t*)out, (const bf16_t*)dout, delta_ws,
                                                                          (long)B * N * H, N, H);
  attn_bwd_dkdv_dh_kernel<DH><<<(unsigned)(nb * B * H), 256, smem_kv, s>>>((const bf16_t*)qkv, (const bf16_t*)dout, lse, delta_ws,
                                                                         (bf16_t*)dqkv, N, H, (int)nb, scale);
  attn_bwd_dq_dh_kernel<DH><<<(unsigned)(nb * B * H), 256, smem_q, s>>>((const bf16_t*)qkv, (const bf16_t*)dout, lse, delta_ws,
                                                                      (bf16_t*)dqkv, N, H, (int)nb, scale);
  if (colsum) {
    const int Cc = 3 * H * DH;
    attn_colsum_dh_kernel<<<dim3((Cc + 255) / 256, B), 256, 0, s>>>((const bf16_t*)dqkv, colsum, N, Cc);
  }
  MV_CHECK_LAUNCH();
  return MV_OK;
}

}  // namespace

extern "C" int mv_attention_fwd_dh(const void* qkv, void* out, float* lse, int B, int N, int H, int dim_head, float scale,
                                   mv_stream_t stream) {
  MV_REQUIRE(B >= 0 && N > 0 && H > 0 && N <= ATTN_DH_MAX_N, MV_ERR_SHAPE);
  MV_REQUIRE(dim_head == 32 || dim_head == 128, MV_ERR_UNSUPPORTED);
  MV_REQUIRE(mv_aligned16(qkv) && mv_aligned16(out) && lse, MV_ERR_ALIGN);
  if (B == 0) return MV_OK;
  return dim_head == 32 ? launch_fwd<32>(qkv, out, lse, B, N, H, scale, (hipStream_t)stream)
                        : launch_fwd<128>(qkv, out, lse, B, N, H, scale, (hipStream_t)stream);
}

extern "C" int mv_attention_bwd_dh(const void* qkv, const void* out, const void* dout, const float* lse, float* delta_ws,
                                   void* dqkv, float* colsum, int B, int N, int H, int dim_head, float scale, mv_stream_t stream) {
  MV_REQUIRE(B >= 0 && N > 0 && H > 0 && N <= ATTN_DH_MAX_N, MV_ERR_SHAPE);
  MV_REQUIRE(dim_head == 32 || dim_head == 128, MV_ERR_UNSUPPORTED);
  MV_REQUIRE(mv_aligned16(qkv) && mv_aligned16(out) && mv_aligned16(dout) && mv_aligned16(dqkv) && lse && delta_ws, MV_ERR_ALIGN);
  if (B == 0) return MV_OK;
  return dim_head == 32 ? launch_bwd<32>(qkv, out, dout, lse, delta_ws, dqkv, colsum, B, N, H, scale, (hipStream_t)stream)
                        : launch_bwd<128>(qkv, out, dout, lse, delta_ws, dqkv, colsum, B, N, H, scale, (hipStream_t)stream);
}
