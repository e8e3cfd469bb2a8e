// Stochastic depth ("drop path", timm's DropPath with scale_by_keep) for the fused transformer blocks (gfx950): the device-side
// draw of the per-(branch, sample) factors and the two HBM-bound kernels that apply one factor per sample.
#include "mv_common.h"
#include "philox.h"

namespace {

// ---- the draw: table[r, b] = (Philox word >= thr[r]) ? scale[r] : 0, counter offset = state[1], key = state[0] ----
// ONE workgroup draws the whole table (at most 2 * depth * B elements) and then bumps the step: no other workgroup exists that
// could read the step after the bump, and the barrier puts every thread's read in front of it.
__global__ __launch_bounds__(256) void drop_path_draw_kernel(uint64_t* state, const unsigned* __restrict__ thr,
                                                             const float* __restrict__ scale, float* __restrict__ table, int R,
                                                             int B) {
  const uint64_t seed = state[0], step = state[1];
  const long n = (long)R * B, n4 = (n + 3) >> 2;
  for (long i = threadIdx.x; i < n4; i += 256) {
    unsigned w[4];
    philox4x32_10((unsigned)i, (unsigned)((uint64_t)i >> 32), (unsigned)step, (unsigned)(step >> 32), (unsigned)seed,
                  (unsigned)(seed >> 32), w);
    const long e0 = i << 2;
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (e0 + e < n) {
        const int r = (int)((e0 + e) / B);
        table[e0 + e] = w[e] >= thr[r] ? scale[r] : 0.f;
      }
  }
  __syncthreads();
  if (threadIdx.x == 0) state[1] = step + 1;
}

// ---- one factor per sample over [B, per_sample] -------------------------------------------------------------------------------
// The walk both streaming kernels share.  The array is walked FLAT in vectors of V elements (16-byte accesses from a 16-byte aligned
// base, whatever per_sample is), grid-stride; a thread keeps (sample, offset in the sample) of its vector and advances both by the
// stride's quotient and remainder, so it divides once.  A vector inside one sample takes that sample's factor; one that straddles
// samples (per_sample % V != 0, or per_sample < V) picks a factor per element.  The n % V elements after the last whole vector are
// the scalar tail, one thread each.  body(i, cv) handles vector i with its V factors, tail(j, c) element j.
template <int V, typename Body, typename Tail>
__device__ __forceinline__ void sample_walk(const float* __restrict__ c, long n, long per_sample, Body body, Tail tail) {
  const long nv = n / V;
  const long stride = (long)gridDim.x * 256;
  long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < nv) {
    const long q = stride * V / per_sample, r = stride * V - q * per_sample;
    long b = i * V / per_sample, rem = i * V - b * per_sample;
    for (; i < nv; i += stride) {
      float cv[V];
      if (rem + V <= per_sample) {
        const float cc = c[b];
#pragma unroll
        for (int e = 0; e < V; ++e) cv[e] = cc;
      } else {
        long be = b, re = rem;
#pragma unroll
        for (int e = 0; e < V; ++e) {
          while (re >= per_sample) { re -= per_sample; ++be; }
          cv[e] = c[be];
          ++re;
        }
      }
      body(i, cv);
      b += q;
      rem += r;
      if (rem >= per_sample) { rem -= per_sample; ++b; }
    }
  }
  const long j = nv * V + threadIdx.x;
  if (blockIdx.x == 0 && j < n) tail(j, c[j / per_sample]);
}

// f <- x + c[b] * f where c[b] != 0 (one fused multiply-add), exactly x where c[b] == 0 (f is not even read when the whole vector is dropped)
__global__ __launch_bounds__(256) void drop_path_add_kernel(const float* __restrict__ x, float* __restrict__ f,
                                                            const float* __restrict__ c, long n, long per_sample) {
  sample_walk<4>(
      c, n, per_sample,
      [&](long i, const float(&cv)[4]) {
        const float4 X = reinterpret_cast<const float4*>(x)[i];
        float4 F = X;
        if (cv[0] != 0.f || cv[1] != 0.f || cv[2] != 0.f || cv[3] != 0.f) {
          F = reinterpret_cast<const float4*>(f)[i];
          const float* xx = &X.x;
          float* ff = &F.x;
#pragma unroll
          for (int e = 0; e < 4; ++e) ff[e] = cv[e] != 0.f ? __builtin_fmaf(cv[e], ff[e], xx[e]) : xx[e];
        }
        reinterpret_cast<float4*>(f)[i] = F;
      },
      [&](long j, float cc) { f[j] = cc != 0.f ? __builtin_fmaf(cc, f[j], x[j]) : x[j]; });
}

// V consecutive elements as floats <- / -> memory in 16-byte pieces (V * sizeof(T) is 16 or 32)
template <int V, typename T>
__device__ __forceinline__ void ld_vec(const T* __restrict__ p, long i, float (&v)[V]) {
  constexpr int PER = 16 / sizeof(T);
#pragma unroll
  for (int k = 0; k < V / PER; ++k) {
    const u32x4 raw = reinterpret_cast<const u32x4*>(p)[i * (V / PER) + k];
    const T* t = reinterpret_cast<const T*>(&raw);
#pragma unroll
    for (int e = 0; e < PER; ++e) v[k * PER + e] = (float)t[e];
  }
}
template <int V, typename T>
__device__ __forceinline__ void st_vec(T* __restrict__ p, long i, const float (&v)[V]) {
  constexpr int PER = 16 / sizeof(T);
#pragma unroll
  for (int k = 0; k < V / PER; ++k) {
    u32x4 raw;
    T* t = reinterpret_cast<T*>(&raw);
#pragma unroll
    for (int e = 0; e < PER; ++e) t[e] = (T)v[k * PER + e];
    reinterpret_cast<u32x4*>(p)[i * (V / PER) + k] = raw;
  }
}

// out <- round(c[b] * float(in)): one rounding of the fp32 product.  A dropped row is still multiplied (0 * x keeps x's sign, as the
// reference product does).
template <typename TI, typename TO>
__global__ __launch_bounds__(256) void row_scale_kernel(const TI* __restrict__ in, TO* __restrict__ out, const float* __restrict__ c,
                                                        long n, long per_sample) {
  constexpr int V = (sizeof(TI) == 4 && sizeof(TO) == 4) ? 4 : 8;
  sample_walk<V>(
      c, n, per_sample,
      [&](long i, const float(&cv)[V]) {
        float v[V];
        ld_vec<V>(in, i, v);
#pragma unroll
        for (int e = 0; e < V; ++e) v[e] = cv[e] * v[e];
        st_vec<V>(out, i, v);
      },
      [&](long j, float cc) { out[j] = (TO)(cc * (float)in[j]); });
}

// Workgroups of 256 threads for nv vectors: one vector per thread, at most the resident workgroups (at most DP_MAX_BLOCKS_PER_CU per
// compute unit: 2 048 threads), grid-stride beyond.
constexpr int DP_MAX_BLOCKS_PER_CU = 8;
template <auto K>
int sample_grid(long nv) {
  long resident = mv_resident_blocks<K>(256, 0);
  const long cap = (long)DP_MAX_BLOCKS_PER_CU * mv_cu_count();
  if (resident > cap) resident = cap;
  const long need = (nv + 255) / 256;
  return (int)(need < 1 ? 1 : need < resident ? need : resident);
}

}  // namespace

extern "C" int mv_drop_path_draw(uint64_t* state, const uint32_t* thr, const float* scale, float* table, int R, int B,
                                 mv_stream_t stream) {
  MV_REQUIRE(R >= 0 && B >= 0 && (long)R * B <= (1L << 24), MV_ERR_SHAPE);
  if ((long)R * B == 0) return MV_OK;
  MV_REQUIRE(state && thr && scale && table && mv_aligned16(state), MV_ERR_ALIGN);
  return mv_launch<drop_path_draw_kernel>(MV_HERE, 1, 256, 0, (hipStream_t)stream, state, thr, scale, table, R, B);
}

extern "C" int mv_drop_path_add(const float* x, float* f, const float* c, int B, long per_sample, mv_stream_t stream) {
  MV_REQUIRE(B >= 0 && per_sample >= 0, MV_ERR_SHAPE);
  const long n = (long)B * per_sample;
  if (n == 0) return MV_OK;
  MV_REQUIRE(x && f && c && mv_aligned16(x) && mv_aligned16(f), MV_ERR_ALIGN);
  return mv_launch<drop_path_add_kernel>(MV_HERE, sample_grid<drop_path_add_kernel>(n / 4), 256, 0, (hipStream_t)stream, x, f, c, n,
                                         per_sample);
}

extern "C" int mv_row_scale(const void* in, int in_dtype, void* out, int out_dtype, const float* c, int B, long per_sample,
                            mv_stream_t stream) {
  MV_REQUIRE(B >= 0 && per_sample >= 0, MV_ERR_SHAPE);
  MV_REQUIRE((in_dtype == MV_F32 || in_dtype == MV_BF16) && (out_dtype == MV_F32 || out_dtype == MV_BF16), MV_ERR_UNSUPPORTED);
  const long n = (long)B * per_sample;
  if (n == 0) return MV_OK;
  MV_REQUIRE(in && out && c && mv_aligned16(in) && mv_aligned16(out), MV_ERR_ALIGN);
  return mv_pick<MV_F32, MV_BF16>(in_dtype, [&](auto DI) {
    return mv_pick<MV_F32, MV_BF16>(out_dtype, [&](auto DO) {
      using TI = mv_elem_t<DI()>;
      using TO = mv_elem_t<DO()>;
      constexpr int V = (sizeof(TI) == 4 && sizeof(TO) == 4) ? 4 : 8;
      return mv_launch<row_scale_kernel<TI, TO>>(MV_HERE, sample_grid<row_scale_kernel<TI, TO>>(n / V), 256, 0, (hipStream_t)stream,
                                                 (const TI*)in, (TO*)out, c, n, per_sample);
    });
  });
}
