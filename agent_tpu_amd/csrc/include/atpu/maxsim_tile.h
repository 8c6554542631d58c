// The on-chip passage tile of the resident-index MaxSim kernels (maxsim_index.hip, maxsim_residual.hip):
// its LDS geometry, the clamps of device data and the MFMA walk over the tile's rows. The kernels differ
// only in how they fill the LDS image; what reads it is this file, so their scores share one arithmetic.
#pragma once

#include "atpu/common.h"

namespace atpu {
namespace {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef const __attribute__((address_space(1))) float* mi_gfloat;  // a global pointer across a call: global_load, not flat
typedef const __attribute__((address_space(1))) f32x4* mi_gf32x4;

constexpr int kMiThreads = 256;
constexpr int kMiMaxTiles = 8;            // 16-row tiles of one on-chip passage tile
constexpr int kMiQChunk = 32;             // queries of one workgroup in the all form
constexpr int kMiLdsBudget = 96 * 1024;   // bytes of passage rows on chip

__host__ __device__ inline int mi_row_bytes(int P, bool f16) { return P * (f16 ? 2 : 4) + 16; }

inline int mi_tile_rows(int P, bool f16) {
  const int rows = (kMiLdsBudget / mi_row_bytes(P, f16)) & ~15;
  return rows < 16 ? 16 : (rows > 16 * kMiMaxTiles ? 16 * kMiMaxTiles : rows);
}

__device__ __forceinline__ int mi_clamp(int x, int lo, int hi) { return min(max(x, lo), hi); }
__device__ __forceinline__ long long mi_clampl(long long x, long long lo, long long hi) {
  return x < lo ? lo : (x > hi ? hi : x);
}

// The lane's max over the live rows of NT on-chip row tiles for query token (lane & 15) of the tile at
// qrow (the lane's own query row, + 4 g floats for fp32, + 8 g for fp16). A call, not inlined: with the
// eight forms inlined into one kernel the scalar registers spill (65 of them); as calls nothing does.
template <bool F16, int NT>
__device__ __noinline__ float mi_tile_max(const unsigned char* __restrict__ lds, int rb, mi_gfloat qrow, int P, int rows,
                                          int r, int g) {
  f32x4 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  if (F16) {
    const unsigned char* a0 = lds + r * rb + 16 * g;
    for (int cp = 0; cp < (P >> 5); ++cp) {
      const f32x4 b0 = *(mi_gf32x4)(qrow + 32 * cp);
      const f32x4 b1 = *(mi_gf32x4)(qrow + 32 * cp + 4);
      f16x8 a[NT];
#pragma unroll
      for (int t = 0; t < NT; ++t) a[t] = *reinterpret_cast<const f16x8*>(a0 + t * 16 * rb + 64 * cp);
#pragma unroll
      for (int j = 0; j < 8; ++j)
#pragma unroll
        for (int t = 0; t < NT; ++t)
          acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32((float)a[t][j], j < 4 ? b0[j & 3] : b1[j & 3], acc[t], 0, 0, 0);
    }
  } else {
    const unsigned char* a0 = lds + r * rb + 16 * g;
    for (int ch = 0; ch < (P >> 4); ++ch) {
      const f32x4 b = *(mi_gf32x4)(qrow + 16 * ch);
      f32x4 a[NT];
#pragma unroll
      for (int t = 0; t < NT; ++t) a[t] = *reinterpret_cast<const f32x4*>(a0 + t * 16 * rb + 64 * ch);
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t][j], b[j], acc[t], 0, 0, 0);
    }
  }
  float m = -__builtin_inff();
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int e = 0; e < 4; ++e) m = fmaxf(m, t * 16 + g * 4 + e < rows ? acc[t][e] : -__builtin_inff());
  return m;
}

// mi_tile_max for the tile's nt = 1 .. 8 row tiles
template <bool F16>
__device__ __forceinline__ float mi_tiles_max(int nt, const unsigned char* lds, int rb, mi_gfloat qrow, int P, int rows,
                                              int r, int g) {
  switch (nt) {
    case 1: return mi_tile_max<F16, 1>(lds, rb, qrow, P, rows, r, g);
    case 2: return mi_tile_max<F16, 2>(lds, rb, qrow, P, rows, r, g);
    case 3: return mi_tile_max<F16, 3>(lds, rb, qrow, P, rows, r, g);
    case 4: return mi_tile_max<F16, 4>(lds, rb, qrow, P, rows, r, g);
    case 5: return mi_tile_max<F16, 5>(lds, rb, qrow, P, rows, r, g);
    case 6: return mi_tile_max<F16, 6>(lds, rb, qrow, P, rows, r, g);
    case 7: return mi_tile_max<F16, 7>(lds, rb, qrow, P, rows, r, g);
    default: return mi_tile_max<F16, 8>(lds, rb, qrow, P, rows, r, g);
  }
}

}  // namespace
}  // namespace atpu
