// Symmetric 127-level row quantisation shared by quantize_rows_i8 and layernorm_quant_i8
// (gemm_i8.hip): every step is one IEEE fp32 operation, so all users agree bit for bit
// with each other and with the PyTorch twin (ops/linear_i8.py).
#pragma once

#include "atpu/common.h"

namespace atpu {

typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ float absmax_bf16x8(bf16x8 v, float amax) {
#pragma unroll
  for (int e = 0; e < 8; ++e) amax = fmaxf(amax, fabsf(bf2f(v[e])));
  return amax;
}

// scale = amax / 127 and inv = 127 / amax of a row (1 and 0 for an all-zero row)
__device__ __forceinline__ float2 quant_scale_inv(float amax) {
  const bool any = amax > 0.f;
  return float2{any ? amax / 127.0f : 1.0f, any ? 127.0f / amax : 0.f};
}

// 8 bf16 -> 8 int8 (two dwords, element e in byte e): clamp(rint(x * inv), -127, 127), rint
// rounding half to even (v_rndne_f32)
__device__ __forceinline__ u32x2 quant_pack8(bf16x8 t, float inv) {
  unsigned w[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    unsigned p = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float r = fminf(fmaxf(rintf(bf2f(t[h * 4 + e]) * inv), -127.f), 127.f);
      p |= (static_cast<unsigned>(static_cast<int>(r)) & 0xffu) << (8 * e);
    }
    w[h] = p;
  }
  return u32x2{w[0], w[1]};
}

}  // namespace atpu
