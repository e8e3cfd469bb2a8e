// What the whole-head kernels (attention.hip) and the key-tiled kernels (attention_tiled.hip) of the 2-byte attention core share:
// the constants, the fragment helpers, the matrix instruction with its half form, the 16-byte output stores.  Each is defined once;
// a helper with one user stays in that user's file.
#pragma once
#include "mv_common.h"

namespace {

constexpr float LOG2E = 1.4426950408889634f;
constexpr float LN2 = 0.6931471805599453f;

__device__ __forceinline__ bf16x8 cat8(bf16x4 a, bf16x4 b) { return __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7); }
__device__ __forceinline__ bf16x4 tr_read(const char* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4bf16(LDS_PTR(bf16x4, p));
}
__device__ __forceinline__ bf16x8 pack8(f32x4 a, f32x4 b) {
  bf16x8 r = {(bf16_t)a[0], (bf16_t)a[1], (bf16_t)a[2], (bf16_t)a[3], (bf16_t)b[0], (bf16_t)b[1], (bf16_t)b[2], (bf16_t)b[3]};
  return r;
}
__device__ __forceinline__ bf16x4 pack4(f32x4 a) {
  bf16x4 r = {(bf16_t)a[0], (bf16_t)a[1], (bf16_t)a[2], (bf16_t)a[3]};
  return r;
}
// F16 forms (round 4, precision "bf16x3"): the SAME kernels on IEEE-half operands -- 11 significand bits instead of 8, the same
// 2-byte geometry, LDS images, fragment maps and MFMA rate (v_mfma_f32_16x16x32_f16).  Fragments stay in their bf16x8 / bf16x4
// containers (they are only moved); what changes is the matrix instruction and every float -> element conversion.
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8_t;
typedef __attribute__((ext_vector_type(4))) _Float16 f16x4_t;
template <bool F16>
__device__ __forceinline__ f32x4 mma32(bf16x8 a, bf16x8 b, f32x4 c, int, int, int) {
  if constexpr (F16)
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8_t, a), __builtin_bit_cast(f16x8_t, b), c, 0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}
template <bool F16>
__device__ __forceinline__ bf16x8 pack8t(f32x4 a, f32x4 b) {
  if constexpr (F16) {
    const f16x8_t r = {(_Float16)a[0], (_Float16)a[1], (_Float16)a[2], (_Float16)a[3],
                       (_Float16)b[0], (_Float16)b[1], (_Float16)b[2], (_Float16)b[3]};
    return __builtin_bit_cast(bf16x8, r);
  } else {
    return pack8(a, b);
  }
}
template <bool F16>
__device__ __forceinline__ bf16x4 pack4t(f32x4 a) {
  if constexpr (F16) {
    const f16x4_t r = {(_Float16)a[0], (_Float16)a[1], (_Float16)a[2], (_Float16)a[3]};
    return __builtin_bit_cast(bf16x4, r);
  } else {
    return pack4(a);
  }
}
// Outputs leave as 16-byte stores: a lane holds 4 consecutive features (8 bytes) of each 16-feature tile; for an adjacent
// tile pair v_permlane16_swap (lanes l <-> l ^ 16, same row) leaves lane group g with 8 consecutive features of tile
// (g & 1), starting at feature 8 (g >> 1) -- a row's four lanes then cover 64 contiguous bytes per instruction instead of
// two 32-byte pieces in two instructions (the NT epilogue's trick; partial-sector accesses are what hurt, DESIGN finding 23).
// Must be executed by every lane of the wave.
__device__ __forceinline__ u32x4 pair16(f32x4 a, f32x4 b) {
  typedef unsigned u32x2_t __attribute__((ext_vector_type(2)));
  const u32x2_t pa = __builtin_bit_cast(u32x2_t, pack4(a)), pb = __builtin_bit_cast(u32x2_t, pack4(b));
  const u32x2_t r0 = __builtin_amdgcn_permlane16_swap(pa[0], pb[0], false, false);
  const u32x2_t r1 = __builtin_amdgcn_permlane16_swap(pa[1], pb[1], false, false);
  return (u32x4){r0[0], r1[0], r0[1], r1[1]};
}
// feature offset of that vector inside the tile pair starting at tile j0: 16 (j0 + (g & 1)) + 8 (g >> 1)
__device__ __forceinline__ int pair16_off(int j0, int g) { return 16 * (j0 + (g & 1)) + 8 * (g >> 1); }

// sum over the 16 lanes with equal lane >> 4 (the 16 rows of a tile), a fixed shuffle tree
__device__ __forceinline__ float rowsum16(float v) {
  v += __shfl_xor(v, 1, 64);
  v += __shfl_xor(v, 2, 64);
  v += __shfl_xor(v, 4, 64);
  v += __shfl_xor(v, 8, 64);
  return v;
}

}  // namespace
