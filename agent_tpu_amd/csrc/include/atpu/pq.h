// Constants and the fixed-order fp32 arithmetic shared by the product-quantization kernels (pq.hip, pq_ivf.hip).
#pragma once

#include "atpu/common.h"

namespace atpu {

constexpr int kPqCodewords = 256;
constexpr int kPqThreads = 256;  // encode and table kernels
constexpr int kPqScanWaves = 8;
constexpr int kPqScanThreads = kPqScanWaves * kWave;
constexpr int kPqBlock = 64;   // rows of one interleaved block: one per lane
constexpr int kPqChains = 4;   // blocks (rows per lane) of one wave step

// The chain p_0, + p_1, ..., + p_{DSUB-1} of separately rounded products.
template <int DSUB>
__device__ __forceinline__ float pq_dot(const float (&x)[DSUB], const float* __restrict__ c) {
  // Plain operators under the pragma, not __fmul_rn / __fadd_rn: those are header functions compiled under the
  // default contraction mode, and once inlined their multiply and add were fused into v_fmac_f32.
#pragma clang fp contract(off)
  float acc = x[0] * c[0];
#pragma unroll
  for (int d = 1; d < DSUB; ++d) {
    const float p = x[d] * c[d];
    acc = acc + p;
  }
  return acc;
}

__device__ __forceinline__ float pq_add(float a, float b) {
#pragma clang fp contract(off)
  return a + b;
}

}  // namespace atpu
