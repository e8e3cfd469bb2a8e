// Key-tiled attention core on 2-byte operands for head widths 32, 64 and 128, any 1 <= N <= 8 192 (reference: Attention.forward
// vit.py:85-99 with the dim_head constructor argument).  One source for three families of entry points:
//   mv_attention_{fwd,bwd}_long       64-wide bf16 (ops.attention_fwd / _bwd route N > 320 here; attention.hip holds the whole-head
//                                     kernels for N <= 320 and the derivations of the orientations and fragment maps)
//   mv_attention_{fwd,bwd}_long_f16   64-wide IEEE half, precision "bf16x3h" past 288 tokens
//   mv_attention_{fwd,bwd}_dh         bf16 at widths 32 and 128
//
// A head's K and V do not fit in LDS past 320 tokens (577 at 384^2, 1 025 for 512^2 segmentation).  Here K / V (forward, dQ) or
// Q / dO (dK / dV) stream through a two-stage LDS ring in 64-row blocks filled by LDS-DMA one block ahead, and nothing of size N^2
// exists anywhere.  The kernels are templated on <DH, F16, SPLIT>:
//   forward : a wave owns 16 RT queries (Q fragments in registers).  Per 64-key block S^T = K Q^T (keys on accumulator rows: the
//             row maximum over keys is in-lane plus two shuffles), a running maximum m and a lane-local running sum l per query in
//             fp32 on exp2 with scale * log2(e) folded in, O^T *= exp2(m_old - m_new), O^T += V^T P^T with P rounded to the operand
//             type (as the whole-head kernels round it); O is divided by l and rounded once.  Keys >= N of the ragged last block
//             are -inf.
//   dK / dV : a wave owns 16 RT keys (K, V fragments and dK^T, dV^T accumulators in registers) and sweeps the query blocks: S, dP
//             with the key on the lane, P from the saved lse, dS = P (dP - delta) scale -- the pass B of attn_bwd2p_kernel.
//   dQ      : a wave owns 16 RT queries (Q, dO fragments in registers) and sweeps the key blocks: S^T, dP^T, dS^T is at once the B
//             operand of dQ^T += K^T dS^T -- the pass A of attn_bwd2p_kernel.
// S and dP are computed twice (seven products instead of five); in exchange every output has exactly one owner: no atomics, no
// cross-workgroup order, bitwise reproducible.  delta = rowsum(dO * O) comes from attn_delta_kernel (workspace [B, H, N]), the
// to_qkv bias-gradient column sums from attn_colsum_kernel: a fixed-order pass over the rounded dqkv.  Transposed operands come by
// ds_read_b64_tr_b16 in the accumulator's k order.  What the width changes:
//   * the contraction of S and dP has KS = DH / 32 MFMA k-steps and O / dQ / dK / dV have DT = DH / 16 feature tiles; both are
//     compile-time loop bounds, nothing branches on the width at run time;
//   * LDS rows are 2 DH bytes.  16-byte chunk ch of row r sits at chunk ch ^ swz(r):
//       DH = 32 (64-byte rows): swz = ((r >> 2) & 1) << 1;   DH = 64 (128-byte rows): swz = ((r >> 1) & 3) << 1, the sw128 image of
//       attention.hip;   DH = 128 (256-byte rows): swz = (r & 7) << 1.
//     All keep ds_read_b128 row fragments (4 cycles) and ds_read_b64_tr_b16 fragments (2 cycles) conflict-free
//     (tools/lds_bank_sim.py, the sw128 and "dh" cases);
//   * rows per wave.  DH = 32: S is ONE MFMA per 16 x 16 tile against 16 exponentials per lane, so the kernels are bound by the
//     softmax arithmetic, not the matrix cores; a wave owns 64 rows (RT = 4 tiles) to halve the barriers and staging per row.
//     DH = 64 and 128: a wave owns 32 rows.  At 128 the forward (O^T: 64 accumulator registers) and dQ fit two waves per SIMD
//     without spilling (225 / 234 VGPRs).  dK / dV holds dK^T and dV^T (128 registers) and the K / V fragments (64) for the whole
//     sweep and does not: it is built for one wave per SIMD, where the compiler keeps the accumulators in the AGPR half of the
//     register file (no scratch in any instantiation: tools/kernel_resources.py).  LDS: a ring stage is 8 / 16 / 32 KiB.
// F16 and SPLIT exist at DH = 64 only.  F16 selects the matrix instruction and the P / dS rounding (mma32 / pack8t), with the
// conventions of attn_fwd13_kernel<true> and attn_bwd2p_kernel<9, true, SPLIT>: half q / k / v, fp32 out; backward on dO16 =
// dO * gscale (a power of two per (image, head)) with delta from attn_bwd_prep_f16_kernel, dS formed without the softmax scale and
// clamped to half's range, the scale and 1 / gscale applied to the fp32 accumulators at the store (exact for gscale); SPLIT = 0
// writes fp32 dqkv, SPLIT = 3 / 6 the bf16 pieces of exactly those values (attn_put4_f16).  Column sums: every dK / dV and dQ
// workgroup writes the sums of its own 128 rows of the fp32 values to a workspace [B, nblk, 3 D]; attn_colsum_ws_kernel adds the
// nblk partials in order.
// Rows >= N: loads are clamped to row N - 1; keys >= N are -inf before the exponential (forward) or p = 0 (backward); queries
// >= N are never stored (forward, dQ) or carry lse = +inf, i.e. p = 0 (dK / dV).  A wave whose rows are all >= N skips the
// arithmetic (not in the 64-wide forward: DhCfg::FWD_SKIPS_IDLE) and still takes part in staging and barriers.
#include "attention_common.h"

namespace {

constexpr int ATTN_TILED_MAX_N = 8192;
constexpr int DBLK = 64;     // rows per streamed LDS block

template <int DH>
struct DhCfg {
  static_assert(DH == 32 || DH == 64 || DH == 128, "instantiated widths");
  static constexpr int KS = DH / 32;            // MFMA k-steps of a contraction over the features
  static constexpr int DT = DH / 16;            // 16-feature tiles
  static constexpr int RB = 2 * DH;             // bytes per LDS row
  static constexpr int CPR = DH / 8;            // 16-byte chunks per row
  static constexpr int RT = DH == 32 ? 4 : 2;   // 16-row tiles a wave owns
  static constexpr int WGROWS = 4 * 16 * RT;    // rows per workgroup (4 waves)
  static constexpr int TILE = DBLK * RB;        // one [64][DH] image
  static constexpr int STAGE = 2 * TILE;        // one ring stage: two images
  static constexpr int RING = 2 * STAGE;        // the ring: two stages (static LDS; dK / dV adds 1 KiB of lse / delta rows)
  static constexpr int DKDV_WAVES_PER_SIMD = DH == 128 ? 1 : 2;   // launch bound of the dK / dV kernel (forward, dQ: 2)
  // The backward kernels read the transposed fragments of a 32-row half (dK / dV: dO and Q, DT x 2 fragments; dQ: K, DT) above
  // the tile loop that forms P / dS, live across it, or per feature tile after it (P and dS of all the wave's tiles live
  // instead).  128: the first does not fit dK / dV's registers; 64: the order the 64-wide kernels were tuned with
  static constexpr bool BWD_TR_FIRST = DH == 64;
  // The forward skips the arithmetic of a wave whose queries are all >= N at 32 and 128.  At 64 the branch around the block's
  // arithmetic costs the half forward its schedule (N = 4 097, four workgroups per CU: + 1 ... 3 % in four alternating runs)
  static constexpr bool FWD_SKIPS_IDLE = DH != 64;
};

template <int DH>
__device__ __forceinline__ int swz(int row) {
  return DH == 32 ? ((row >> 2) & 1) << 1 : DH == 64 ? ((row >> 1) & 3) << 1 : (row & 7) << 1;
}

// Per-lane LDS offsets of the fragment reads.  Tile bases are multiples of 16 rows, so swz() depends on the lane only.  The chunk
// of a fragment is (4 ks + g) ^ swz or (2 dt + (p >> 1)) ^ swz; g < 4 and p >> 1 < 2 leave the bits of 4 ks and 2 dt zero, so the
// sum is an XOR, XOR is associative, and the k-step / feature tile goes in on top of the lane's (g ^ swz) term -- whichever bits swz
// itself sets -- with one XOR per read instead of one register per (ks, dt).  The compiler hoists those XORs out of the block loop.
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
// 1024 / RB whole rows; the waves take pieces round-robin; rows >= N are clamped to N - 1 (masked by the caller).  The DMA is hidden
// from the compiler's wait bookkeeping (glds16_hidden): the caller's own s_waitcnt vmcnt(0) + barrier orders it, and the transposed
// LDS reads of the other stage are not held behind it.
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

// F16 outputs of the backward: four consecutive fp32 features v at (row = b N + token, col < 3 D) of dqkv [B N, 3 D] (SPLIT = 0),
// or their bf16 pieces in rows of SPLIT * 3 D, segments 3 D apart (mv_split2_bf16 / mv_split3_bf16 role 0) -- attn_bwd2p_kernel's put4
template <int SPLIT>
__device__ __forceinline__ void attn_put4_f16(bf16_t* __restrict__ dqkv, long row, long col, long C, f32x4 v) {
  if constexpr (SPLIT == 0) {
    *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(dqkv) + row * C + col) = v;
  } else {
    bf16_t* o = dqkv + row * (SPLIT * C) + col;
    bf16x4 p[3];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const bf16_t p0 = (bf16_t)v[e];
      const float r1 = v[e] - (float)p0;
      const bf16_t p1 = (bf16_t)r1;
      p[0][e] = p0;
      p[1][e] = p1;
      p[2][e] = (bf16_t)(r1 - (float)p1);
    }
    constexpr int order[6] = {0, 0, 1, 0, 1, 2};
#pragma unroll
    for (int sg = 0; sg < SPLIT; ++sg) *reinterpret_cast<bf16x4*>(o + (long)sg * C) = p[order[sg]];
  }
}

// ------------------------------------------------------------------------------------------------
// forward: a wave owns 16 RT queries; per 64-key block S^T = K Q^T, online softmax, O^T += V^T P^T
// ------------------------------------------------------------------------------------------------
template <int DH, bool F16 = false>   // F16: half operands, fp32 out
__global__ __launch_bounds__(256, 2) void attn_fwd_kernel(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ out,
                                                          float* __restrict__ lse, int N, int H, int nqb, float scale_log2e) {
  static_assert(!F16 || DH == 64, "the half form exists at width 64 only");
  using C = DhCfg<DH>;
  constexpr int KS = C::KS, DT = C::DT, RT = C::RT;
  __shared__ __attribute__((aligned(16))) char smem[C::RING];       // stage s: K [64][DH] | V [64][DH]
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
  const bool active = !C::FWD_SKIPS_IDLE || q0 < N;    // wave-uniform; an idle wave still takes part in staging and barriers
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
          for (int ks = 0; ks < KS; ++ks) acc = mma32<F16>(kf[ks], qf[t][ks], acc, 0, 0, 0);
          st[t][kt] = acc;
        }
      }
#pragma unroll
      for (int t = 0; t < RT; ++t) {
        float mb = -INFINITY;
#pragma unroll
        for (int kt = 0; kt < 4; ++kt)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            // only the last block can hold keys >= N; every block is masked: a test per block costs a second select per score
            const float v = kb * DBLK + kt * 16 + 4 * g + r < N ? st[t][kt][r] * scale_log2e : -INFINITY;
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
        for (int t = 0; t < RT; ++t) pf[t] = pack8t<F16>(st[t][2 * u], st[t][2 * u + 1]);
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
          const bf16x8 vf = tr_frag<DH>(sV, 32 * u, L, dt);
#pragma unroll
          for (int t = 0; t < RT; ++t) o[t][dt] = mma32<F16>(vf, pf[t], o[t][dt], 0, 0, 0);
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
    if constexpr (F16) {                               // fp32 output: the lane's four features of each 16-feature tile
      float* orow = reinterpret_cast<float*>(out) + ((long)b * N + qrow) * D + h * DH;
#pragma unroll
      for (int dt = 0; dt < DT; ++dt)
        if (qrow < N) *reinterpret_cast<f32x4*>(orow + 16 * dt + 4 * g) = o[t][dt] * inv;
    } else {
      bf16_t* orow = out + ((long)b * N + qrow) * D + h * DH;
#pragma unroll
      for (int dp = 0; dp < DT; dp += 2) {
        const u32x4 w = pair16(o[t][dp] * inv, o[t][dp + 1] * inv);     // every lane (lane exchange)
        if (qrow < N) *reinterpret_cast<u32x4*>(orow + pair16_off(dp, g)) = w;
      }
    }
    if (qrow < N && g == 0) lse[((long)b * H + h) * N + qrow] = (m[t] + __builtin_amdgcn_logf(s)) * LN2;
  }
}

// delta[b, h, n] = sum_d dO[b, n, h, d] O[b, n, h, d] in fp32: CPR = DH / 8 consecutive threads per (token, head), a fixed shuffle
// tree
template <int CPR>
__global__ __launch_bounds__(256) void attn_delta_kernel(const bf16_t* __restrict__ out, const bf16_t* __restrict__ dout,
                                                         float* __restrict__ delta, long rows, int N, int H) {
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
template <int DH, bool F16 = false, int SPLIT = 0>   // F16: dout = dO16 (scaled by gscale), dqkv fp32 or SPLIT pieces, colsum_ws partials
__global__ __launch_bounds__(256, DhCfg<DH>::DKDV_WAVES_PER_SIMD) void attn_bwd_dkdv_kernel(
    const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ dout, const float* __restrict__ lse, const float* __restrict__ delta,
    bf16_t* __restrict__ dqkv, int N, int H, int nkb, float scale, const float* __restrict__ gscale = nullptr,
    float* __restrict__ colsum_ws = nullptr) {
  static_assert(!F16 || DH == 64, "the half form exists at width 64 only");
  using C = DhCfg<DH>;
  constexpr int KS = C::KS, DT = C::DT, KT = C::RT;
  __shared__ __attribute__((aligned(16))) char smem[C::RING];       // stage s: Q [64][DH] | dO [64][DH]
  __shared__ __attribute__((aligned(16))) float sRow[2 * 2 * DBLK];  // [stage][lse * log2(e) (+inf past N) | delta (0 past N)][64]
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
        [[maybe_unused]] bf16x8 dotr[DT], qtr[DT];
        if constexpr (C::BWD_TR_FIRST) {
#pragma unroll
          for (int dt = 0; dt < DT; ++dt) {
            dotr[dt] = tr_frag<DH>(sDO, 32 * u, L, dt);
            qtr[dt] = tr_frag<DH>(sQ, 32 * u, L, dt);
          }
        }
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
                sv = mma32<F16>(qrf[t][ks], kf[i][ks], sv, 0, 0, 0);
                dp = mma32<F16>(dorf[t][ks], vf[i][ks], dp, 0, 0, 0);
              }
#pragma unroll
              for (int r = 0; r < 4; ++r) {
                float p = __builtin_amdgcn_exp2f(sv[r] * c2 - l2v[t][r]);     // queries >= N: lse = +inf -> p = 0
                p = key < N ? p : 0.f;
                pp[t][r] = p;
                ds[t][r] = F16 ? __builtin_amdgcn_fmed3f(p * (dp[r] - dlv[t][r]), -65000.f, 65000.f) : p * (dp[r] - dlv[t][r]) * scale;
              }
            }
            pf[i] = pack8t<F16>(pp[0], pp[1]);
            dsf[i] = pack8t<F16>(ds[0], ds[1]);
            if constexpr (C::BWD_TR_FIRST) {
#pragma unroll
              for (int dt = 0; dt < DT; ++dt) {
                adv[i][dt] = mma32<F16>(dotr[dt], pf[i], adv[i][dt], 0, 0, 0);
                adk[i][dt] = mma32<F16>(qtr[dt], dsf[i], adk[i][dt], 0, 0, 0);
              }
            }
          }
        }
        if constexpr (!C::BWD_TR_FIRST) {
#pragma unroll
          for (int dt = 0; dt < DT; ++dt) {
            const bf16x8 dot = tr_frag<DH>(sDO, 32 * u, L, dt), qt = tr_frag<DH>(sQ, 32 * u, L, dt);
#pragma unroll
            for (int i = 0; i < KT; ++i) {
              adv[i][dt] = mma32<F16>(dot, pf[i], adv[i][dt], 0, 0, 0);
              adk[i][dt] = mma32<F16>(qt, dsf[i], adk[i][dt], 0, 0, 0);
            }
          }
        }
      }
    }
    if (qb + 1 < nqb) put_row(qb + 1, nrow);           // the stage qb + 1 & 1 was last read before the previous barrier
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }
  if constexpr (F16) {
    const float inv_s = 1.0f / gscale[bh], inv_ss = inv_s * scale;
#pragma unroll
    for (int i = 0; i < KT; ++i) {
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) {
        adk[i][dt] *= inv_ss;
        adv[i][dt] *= inv_s;
      }
      const int key = k0 + 16 * i + (lane & 15);
      if (key < N) {
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
          attn_put4_f16<SPLIT>(dqkv, (long)b * N + key, D + h * DH + 16 * dt + 4 * g, 3 * D, adk[i][dt]);
          attn_put4_f16<SPLIT>(dqkv, (long)b * N + key, 2 * D + h * DH + 16 * dt + 4 * g, 3 * D, adv[i][dt]);
        }
      }
    }
    if (colsum_ws) {                                   // padded keys and idle waves: exact zeros
      float* sCs = reinterpret_cast<float*>(smem);     // [4 waves][dK 64 | dV 64]; the ring is idle after the last barrier
#pragma unroll
      for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float vk = rowsum16(adk[0][dt][r] + adk[1][dt][r]), vv = rowsum16(adv[0][dt][r] + adv[1][dt][r]);
          if ((lane & 15) == 0) {
            sCs[wave * 128 + dt * 16 + 4 * g + r] = vk;
            sCs[wave * 128 + 64 + dt * 16 + 4 * g + r] = vv;
          }
        }
      __syncthreads();
      if (tid < 128)
        colsum_ws[((long)b * nkb + kblk) * 3 * D + (1 + (tid >> 6)) * D + h * 64 + (tid & 63)] =
            ((sCs[tid] + sCs[128 + tid]) + sCs[256 + tid]) + sCs[384 + tid];
    }
  } else {
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
}

// ------------------------------------------------------------------------------------------------
// dQ: a wave owns 16 RT queries (Q, dO fragments and dQ^T accumulators in registers) and sweeps the key blocks
// ------------------------------------------------------------------------------------------------
template <int DH, bool F16 = false, int SPLIT = 0>   // F16: as attn_bwd_dkdv_kernel
__global__ __launch_bounds__(256, 2) void attn_bwd_dq_kernel(
    const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ dout, const float* __restrict__ lse, const float* __restrict__ delta,
    bf16_t* __restrict__ dqkv, int N, int H, int nqb, float scale, const float* __restrict__ gscale = nullptr,
    float* __restrict__ colsum_ws = nullptr) {
  static_assert(!F16 || DH == 64, "the half form exists at width 64 only");
  using C = DhCfg<DH>;
  constexpr int KS = C::KS, DT = C::DT, QT = C::RT;
  __shared__ __attribute__((aligned(16))) char smem[C::RING];       // stage s: K [64][DH] | V [64][DH]
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
        [[maybe_unused]] bf16x8 ktr[DT];
        {
          bf16x8 kr[2][KS], vr[2][KS];
#pragma unroll
          for (int kk = 0; kk < 2; ++kk)
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
              kr[kk][ks] = row_frag<DH>(sK, 32 * u + 16 * kk, L, ks);
              vr[kk][ks] = row_frag<DH>(sV, 32 * u + 16 * kk, L, ks);
            }
          if constexpr (C::BWD_TR_FIRST) {
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) ktr[dt] = tr_frag<DH>(sK, 32 * u, L, dt);
          }
#pragma unroll
          for (int t = 0; t < QT; ++t) {
            f32x4 ds[2];
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) {
              f32x4 st = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
              for (int ks = 0; ks < KS; ++ks) {
                st = mma32<F16>(kr[kk][ks], qf[t][ks], st, 0, 0, 0);
                dp = mma32<F16>(vr[kk][ks], dof[t][ks], dp, 0, 0, 0);
              }
#pragma unroll
              for (int r = 0; r < 4; ++r) {
                const int key = kb * DBLK + 32 * u + 16 * kk + 4 * g + r;
                const float p = key < N ? __builtin_amdgcn_exp2f(st[r] * c2 - l2[t]) : 0.f;
                ds[kk][r] = F16 ? __builtin_amdgcn_fmed3f(p * (dp[r] - dl[t]), -65000.f, 65000.f) : p * (dp[r] - dl[t]) * scale;
              }
            }
            dsf[t] = pack8t<F16>(ds[0], ds[1]);
            if constexpr (C::BWD_TR_FIRST) {
#pragma unroll
              for (int dt = 0; dt < DT; ++dt) dq[t][dt] = mma32<F16>(ktr[dt], dsf[t], dq[t][dt], 0, 0, 0);
            }
          }
        }
        if constexpr (!C::BWD_TR_FIRST) {
#pragma unroll
          for (int dt = 0; dt < DT; ++dt) {
            const bf16x8 kt = tr_frag<DH>(sK, 32 * u, L, dt);
#pragma unroll
            for (int t = 0; t < QT; ++t) dq[t][dt] = mma32<F16>(kt, dsf[t], dq[t][dt], 0, 0, 0);
          }
        }
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }
  if constexpr (F16) {
    const float inv_ss = 1.0f / gscale[bh] * scale;
#pragma unroll
    for (int t = 0; t < QT; ++t) {
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) dq[t][dt] *= inv_ss;
      const int qrow = q0 + 16 * t + (lane & 15);
      if (qrow < N) {
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) attn_put4_f16<SPLIT>(dqkv, (long)b * N + qrow, h * DH + 16 * dt + 4 * g, 3 * D, dq[t][dt]);
      }
    }
    if (colsum_ws) {                                   // padded queries (lse = +inf) and idle waves: exact zeros
      float* sCs = reinterpret_cast<float*>(smem);     // [4 waves][dQ 64]; the ring is idle after the last barrier
#pragma unroll
      for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float vq = rowsum16(dq[0][dt][r] + dq[1][dt][r]);
          if ((lane & 15) == 0) sCs[wave * 64 + dt * 16 + 4 * g + r] = vq;
        }
      __syncthreads();
      if (tid < 64)
        colsum_ws[((long)b * nqb + qblk) * 3 * D + h * 64 + tid] = ((sCs[tid] + sCs[64 + tid]) + sCs[128 + tid]) + sCs[192 + tid];
    }
  } else {
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
}

// colsum[b][c] = sum_n dqkv[b, n, c] (c < C = 3 H DH) in fp32, in a fixed order: thread (phase = tid >> 5, 8 columns from
// 8 (tid & 31)) adds rows phase, phase + 8, ...; the eight phase sums are added in order.  One workgroup per (256 columns, image).
__global__ __launch_bounds__(256) void attn_colsum_kernel(const bf16_t* __restrict__ dqkv, float* __restrict__ colsum, int N, int C) {
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

// colsum[b][c] = sum_k ws[b][k][c] over the nblk row-block partials of the F16 backward, k = 0, 1, ... in order
__global__ __launch_bounds__(256) void attn_colsum_ws_kernel(const float* __restrict__ ws, float* __restrict__ colsum, int nblk, int C,
                                                             long total) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;     // = b C + c
  if (idx >= total) return;
  const long b = idx / C, c = idx % C;
  const float* p = ws + b * nblk * C + c;
  float s = 0.f;
  for (int k = 0; k < nblk; ++k) s += p[(long)k * C];
  colsum[idx] = s;
}

// The launchers repeat the grid-size checks of the entry points that have their own (the *_long* ones, ahead of their alignment
// check): one place knows the workgroup shape.
template <int DH, bool F16>
int launch_fwd(const void* qkv, void* out, float* lse, int B, int N, int H, float scale, hipStream_t s) {
  using C = DhCfg<DH>;
  const long nqb = (N + C::WGROWS - 1) / C::WGROWS;
  MV_REQUIRE(nqb * B * H < (1L << 31), MV_ERR_SHAPE);
  return mv_launch<attn_fwd_kernel<DH, F16>>(MV_HERE, (unsigned)(nqb * B * H), 256, 0, s, (const bf16_t*)qkv, (bf16_t*)out, lse, N,
                                             H, (int)nqb, scale * LOG2E);
}

template <int DH>
int launch_bwd(const void* qkv, const void* out, const void* dout, const float* lse, float* delta_ws, void* dqkv, float* colsum,
               int B, int N, int H, float scale, hipStream_t s) {
  using C = DhCfg<DH>;
  const long nb = (N + C::WGROWS - 1) / C::WGROWS, chunks = (long)B * N * H * C::CPR;
  MV_REQUIRE(nb * B * H < (1L << 31) && (chunks + 255) / 256 < (1L << 31) && B < 65536, MV_ERR_SHAPE);
  const unsigned grid = (unsigned)(nb * B * H);
  if (int rc = mv_launch<attn_delta_kernel<C::CPR>>(MV_HERE, (unsigned)((chunks + 255) / 256), 256, 0, s, (const bf16_t*)out,
                                                    (const bf16_t*)dout, delta_ws, (long)B * N * H, N, H))
    return rc;
  if (int rc = mv_launch<attn_bwd_dkdv_kernel<DH>>(MV_HERE, grid, 256, 0, s, (const bf16_t*)qkv, (const bf16_t*)dout, lse, delta_ws,
                                                   (bf16_t*)dqkv, N, H, (int)nb, scale, nullptr, nullptr))
    return rc;
  const int rc = mv_launch<attn_bwd_dq_kernel<DH>>(MV_HERE, grid, 256, 0, s, (const bf16_t*)qkv, (const bf16_t*)dout, lse, delta_ws,
                                                   (bf16_t*)dqkv, N, H, (int)nb, scale, nullptr, nullptr);
  if (rc != MV_OK || !colsum) return rc;
  const int Cc = 3 * H * DH;
  return mv_launch<attn_colsum_kernel>(MV_HERE, dim3((Cc + 255) / 256, B), 256, 0, s, (const bf16_t*)dqkv, colsum, N, Cc);
}

// the two F16 backward kernels (delta and gscale come from mv_attention_bwd_prep_f16); ws: the column-sum workspace or nullptr
template <int SPLIT>
int launch_bwd_f16(const void* qkv16, const void* dout16, const float* delta, const float* lse, const float* gscale, void* dqkv,
                   float* ws, int B, int N, int H, int nb, float scale, hipStream_t s) {
  if (int rc = mv_launch<attn_bwd_dkdv_kernel<64, true, SPLIT>>(MV_HERE, (unsigned)(nb * B * H), 256, 0, s, (const bf16_t*)qkv16,
                                                                (const bf16_t*)dout16, lse, delta, (bf16_t*)dqkv, N, H, nb, scale, gscale, ws))
    return rc;
  return mv_launch<attn_bwd_dq_kernel<64, true, SPLIT>>(MV_HERE, (unsigned)(nb * B * H), 256, 0, s, (const bf16_t*)qkv16,
                                                        (const bf16_t*)dout16, lse, delta, (bf16_t*)dqkv, N, H, nb, scale, gscale, ws);
}

constexpr int LROWS = DhCfg<64>::WGROWS;   // rows per workgroup of the 64-wide kernels: forward / dQ queries, dK / dV keys
static_assert(LROWS == 128, "the F16 column-sum workspace has one [3 D] row per 128-row block of queries and of keys");

}  // namespace

// ------------------------------------------------------------------------------------------------
// 64-wide bf16, any N up to ATTN_TILED_MAX_N (ops.attention_fwd / _bwd route N > 320 here)
// ------------------------------------------------------------------------------------------------
extern "C" int mv_attention_fwd_long(const void* qkv, void* out, float* lse, int B, int N, int H, float scale,
                                     mv_stream_t stream) {
  MV_REQUIRE(B >= 0 && N > 0 && H > 0 && N <= ATTN_TILED_MAX_N, MV_ERR_SHAPE);
  const long nqb = (N + LROWS - 1) / LROWS;
  MV_REQUIRE(nqb * B * H < (1L << 31), MV_ERR_SHAPE);
  MV_REQUIRE(mv_aligned16(qkv) && mv_aligned16(out) && lse, MV_ERR_ALIGN);
  if (B == 0) return MV_OK;
  return launch_fwd<64, false>(qkv, out, lse, B, N, H, scale, (hipStream_t)stream);
}

extern "C" int mv_attention_bwd_long(const void* qkv, const void* out, const void* dout, const float* lse, float* delta_ws,
                                     void* dqkv, float* colsum, int B, int N, int H, float scale, mv_stream_t stream) {
  MV_REQUIRE(B >= 0 && N > 0 && H > 0 && N <= ATTN_TILED_MAX_N, MV_ERR_SHAPE);
  const long nqb = (N + LROWS - 1) / LROWS, nkb = nqb, rows8 = (long)B * N * H * 8;
  MV_REQUIRE(nqb * B * H < (1L << 31) && nkb * B * H < (1L << 31) && (rows8 + 255) / 256 < (1L << 31) && B < 65536,
             MV_ERR_SHAPE);
  MV_REQUIRE(mv_aligned16(qkv) && mv_aligned16(out) && mv_aligned16(dout) && mv_aligned16(dqkv) && lse && delta_ws, MV_ERR_ALIGN);
  if (B == 0) return MV_OK;
  return launch_bwd<64>(qkv, out, dout, lse, delta_ws, dqkv, colsum, B, N, H, scale, (hipStream_t)stream);
}

// ------------------------------------------------------------------------------------------------
// precision "bf16x3h" past 288 tokens: the same kernels on IEEE-half operands (ops.attention_fwd_f16 / _bwd_f16 route N > 288
// here); any 1 <= N <= ATTN_TILED_MAX_N
// ------------------------------------------------------------------------------------------------
extern "C" int mv_attention_fwd_long_f16(const void* qkv16, float* out, float* lse, int B, int N, int H, float scale,
                                         mv_stream_t stream) {
  MV_REQUIRE(B >= 0 && N > 0 && H > 0 && N <= ATTN_TILED_MAX_N, MV_ERR_SHAPE);
  const long nqb = (N + LROWS - 1) / LROWS;
  MV_REQUIRE(nqb * B * H < (1L << 31), MV_ERR_SHAPE);
  MV_REQUIRE(mv_aligned16(qkv16) && mv_aligned16(out) && lse, MV_ERR_ALIGN);
  if (B == 0) return MV_OK;
  return launch_fwd<64, true>(qkv16, out, lse, B, N, H, scale, (hipStream_t)stream);
}

extern "C" int mv_attention_bwd_long_f16(const void* qkv16, const void* dout16, const float* delta, const float* lse,
                                         const float* gscale, void* dqkv, int nseg, float* colsum, float* colsum_ws, int B, int N,
                                         int H, float scale, mv_stream_t stream) {
  MV_REQUIRE(B >= 0 && N > 0 && H > 0 && N <= ATTN_TILED_MAX_N, MV_ERR_SHAPE);
  MV_REQUIRE(nseg == 0 || nseg == 3 || nseg == 6, MV_ERR_UNSUPPORTED);
  const long nb = (N + LROWS - 1) / LROWS, C = 3L * H * 64;
  MV_REQUIRE(nb * B * H < (1L << 31) && ((long)B * C + 255) / 256 < (1L << 31), MV_ERR_SHAPE);
  MV_REQUIRE(mv_aligned16(qkv16) && mv_aligned16(dout16) && mv_aligned16(dqkv) && delta && lse && gscale && (!colsum || colsum_ws),
             MV_ERR_ALIGN);
  if (B == 0) return MV_OK;
  hipStream_t s = (hipStream_t)stream;
  float* ws = colsum ? colsum_ws : nullptr;
  const int rc = mv_pick<0, 3, 6>(nseg, [&](auto NSEG) {
    return launch_bwd_f16<NSEG()>(qkv16, dout16, delta, lse, gscale, dqkv, ws, B, N, H, (int)nb, scale, s);
  });
  if (rc != MV_OK || !colsum) return rc;
  return mv_launch<attn_colsum_ws_kernel>(MV_HERE, (unsigned)(((long)B * C + 255) / 256), 256, 0, s, ws, colsum, (int)nb, (int)C,
                                          (long)B * C);
}

// ------------------------------------------------------------------------------------------------
// bf16 at widths 32 and 128 (64 has the entry points above)
// ------------------------------------------------------------------------------------------------
extern "C" int mv_attention_fwd_dh(const void* qkv, void* out, float* lse, int B, int N, int H, int dim_head, float scale,
                                   mv_stream_t stream) {
  MV_REQUIRE(B >= 0 && N > 0 && H > 0 && N <= ATTN_TILED_MAX_N, MV_ERR_SHAPE);
  MV_REQUIRE(dim_head == 32 || dim_head == 128, MV_ERR_UNSUPPORTED);
  MV_REQUIRE(mv_aligned16(qkv) && mv_aligned16(out) && lse, MV_ERR_ALIGN);
  if (B == 0) return MV_OK;
  return mv_pick<32, 128>(dim_head, [&](auto DH) { return launch_fwd<DH(), false>(qkv, out, lse, B, N, H, scale, (hipStream_t)stream); });
}

extern "C" int mv_attention_bwd_dh(const void* qkv, const void* out, const void* dout, const float* lse, float* delta_ws,
                                   void* dqkv, float* colsum, int B, int N, int H, int dim_head, float scale, mv_stream_t stream) {
  MV_REQUIRE(B >= 0 && N > 0 && H > 0 && N <= ATTN_TILED_MAX_N, MV_ERR_SHAPE);
  MV_REQUIRE(dim_head == 32 || dim_head == 128, MV_ERR_UNSUPPORTED);
  MV_REQUIRE(mv_aligned16(qkv) && mv_aligned16(out) && mv_aligned16(dout) && mv_aligned16(dqkv) && lse && delta_ws, MV_ERR_ALIGN);
  if (B == 0) return MV_OK;
  return mv_pick<32, 128>(dim_head, [&](auto DH) {
    return launch_bwd<DH()>(qkv, out, dout, lse, delta_ws, dqkv, colsum, B, N, H, scale, (hipStream_t)stream);
  });
}
