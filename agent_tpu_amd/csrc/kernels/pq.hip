// Product quantization (PQ): a row of D floats is stored as M bytes, byte m the nearest of 256 codewords
// of the sub-space m (columns m * dsub .. + dsub - 1, dsub = D / M in {4, 8, 16}). A query is scored
// against the codes by asymmetric distance computation (ADC): a table lut [M, 256] of the query's
// sub-vector dot products with every codeword, summed per row over the row's M codes. No MFMA: the
// encoder and the table are short fp32 chains on the VALU, the scan is LDS gathers and adds.
//
// Arithmetic, the same in all three kernels and in their PyTorch twins (ops/pq.py): a dot product over
// a sub-space is the chain p_0, + p_1, ..., + p_{dsub-1} of separately rounded products p_d = x_d * c_d
// (no FMA contraction), and a row's ADC score is the chain lut[0][code_0], + lut[1][code_1], ... in
// ascending m. A value therefore depends on its own operands only: not on the launch shape, the batch,
// the split or the row's position.
//
// pq_encode_kernel<DSUB>: one workgroup per (256 rows, sub-space); the sub-space's codebook (at most
// 16 KiB) and bias sit in LDS, every lane owns one row, keeps its DSUB values in registers and walks the
// 256 codewords (all lanes read the same LDS address: a broadcast). Sub-space is the fast grid index,
// so the workgroups that share a row block run together and share its lines in L2.
//
// pq_lut_kernel<DSUB>: one thread per table entry.
//
// pq_scan_kernel<KM>: one workgroup of 8 waves per split of the rows. It loops over the queries: the
// query's table (M KiB) is copied to LDS, the split's codes are scanned, and the workgroup's top-k goes
// to ws[query][split]; the codes of a split (rows * M bytes) are re-read per query from L2 / Infinity
// Cache. The codes come in the index's interleaved layout [block of 64 rows][M / 4][lane][4 bytes]: the
// wave's load of 4 sub-spaces of 64 rows is one contiguous 256 B. A lane runs kPqChains = 4 rows (of
// four 64-row blocks) at once, so four independent add chains cover the latency of the dependent
// LDS gathers; 64 lanes gather from one 256-entry table, which conflicts on banks a few ways. Each
// lane keeps one sorted register list per query (list_insert behind a wave ballot, as sim_topk);
// wave_topk reduces the 64 lists of a wave in registers, and 8 lanes of wave 0 merge the 8 wave lists
// through LDS. Eight waves because the table of M = 128 (128 KiB) leaves one workgroup per CU: two
// waves per SIMD keep gathers in flight while the other wave adds.
//
// Rows past N in the last block are padding of the interleaved layout (zero codes, inside the buffer):
// their scores are discarded by select. Nothing outside lut, the blocks [0, ceil(N / 64)) and ws is touched.
#include "atpu/common.h"
#include "atpu/kernels.h"
#include "atpu/topk.h"

namespace atpu {
namespace {

constexpr int kPqCodewords = 256;
constexpr int kPqThreads = 256;  // encode and table kernels
constexpr int kPqScanWaves = 8;
constexpr int kPqScanThreads = kPqScanWaves * kWave;
constexpr int kPqBlock = 64;   // rows of one interleaved block: one per lane
constexpr int kPqChains = 4;   // blocks (rows per lane) of one wave step
constexpr int kNoRow = 0x7fffffff;

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

template <int DSUB>
__global__ __launch_bounds__(kPqThreads) void pq_encode_kernel(const float* __restrict__ x,
                                                               const float* __restrict__ cb,
                                                               const float* __restrict__ bias,
                                                               uint8_t* __restrict__ codes, int n, int D, int M) {
#pragma clang fp contract(off)
  __shared__ __attribute__((aligned(16))) float scb[kPqCodewords * DSUB];
  __shared__ __attribute__((aligned(16))) float sb[kPqCodewords];
  const int tid = threadIdx.x;
  const int m = blockIdx.x % M, rb = blockIdx.x / M;
  const f32x4* src = reinterpret_cast<const f32x4*>(cb + (size_t)m * kPqCodewords * DSUB);
  for (int i = tid; i < kPqCodewords * DSUB / 4; i += kPqThreads) reinterpret_cast<f32x4*>(scb)[i] = src[i];
  sb[tid] = bias[m * kPqCodewords + tid];
  __syncthreads();
  const int row = rb * kPqThreads + tid;
  if (row >= n) return;
  float xv[DSUB];
  const f32x4* xp = reinterpret_cast<const f32x4*>(x + (size_t)row * D + m * DSUB);
#pragma unroll
  for (int e = 0; e < DSUB / 4; ++e) {
    const f32x4 v = xp[e];
#pragma unroll
    for (int j = 0; j < 4; ++j) xv[4 * e + j] = v[j];
  }
  float best = pq_add(pq_dot<DSUB>(xv, scb), sb[0]);
  int bi = 0;
  for (int j = 1; j < kPqCodewords; ++j) {
    const float s = pq_add(pq_dot<DSUB>(xv, scb + j * DSUB), sb[j]);
    if (s > best) {  // ascending j: a tie (+0.0 == -0.0 too) keeps the lower id
      best = s;
      bi = j;
    }
  }
  codes[(size_t)row * M + m] = (uint8_t)bi;
}

template <int DSUB>
__global__ __launch_bounds__(kPqThreads) void pq_lut_kernel(const float* __restrict__ q, const float* __restrict__ cb,
                                                            float* __restrict__ lut, int D, int M) {
  // one workgroup per (query, sub-space), one thread per codeword
  const int m = blockIdx.x % M, qi = blockIdx.x / M, j = threadIdx.x;
  float xv[DSUB], cv[DSUB];
  const f32x4* xp = reinterpret_cast<const f32x4*>(q + (size_t)qi * D + m * DSUB);
  const f32x4* cp = reinterpret_cast<const f32x4*>(cb + ((size_t)m * kPqCodewords + j) * DSUB);
#pragma unroll
  for (int e = 0; e < DSUB / 4; ++e) {
    const f32x4 v = xp[e], c = cp[e];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      xv[4 * e + i] = v[i];
      cv[4 * e + i] = c[i];
    }
  }
  lut[((size_t)qi * M + m) * kPqCodewords + j] = pq_dot<DSUB>(xv, cv);
}

template <int KM>
__global__ __launch_bounds__(kPqScanThreads) void pq_scan_kernel(const float* __restrict__ lut,
                                                                 const uint32_t* __restrict__ codes,
                                                                 float2* __restrict__ ws, int nq, int N, int M, int k,
                                                                 int P, int blocks_per_split) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float2* wl = reinterpret_cast<float2*>(smem + M * kPqCodewords);  // [kPqScanWaves][KM] wave lists
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int split = blockIdx.x;
  const int M4 = M >> 2;
  const int nblocks = (N + kPqBlock - 1) / kPqBlock;
  const int b_lo = split * blocks_per_split, b_hi = min(b_lo + blocks_per_split, nblocks);

  for (int qi = 0; qi < nq; ++qi) {
    // the query's table -> LDS (the previous query's scan ended at the barrier before its merge)
    const f32x4* src = reinterpret_cast<const f32x4*>(lut + (size_t)qi * M * kPqCodewords);
    for (int i = tid; i < M * (kPqCodewords / 4); i += kPqScanThreads) reinterpret_cast<f32x4*>(smem)[i] = src[i];
    __syncthreads();

    float tv[KM];
    int ti[KM];
#pragma unroll
    for (int e = 0; e < KM; ++e) {
      tv[e] = -__builtin_inff();
      ti[e] = kNoRow;
    }
    for (int b = b_lo + wave * kPqChains; b < b_hi; b += kPqScanWaves * kPqChains) {
      const uint32_t* cp[kPqChains];
#pragma unroll
      for (int c = 0; c < kPqChains; ++c)  // a block past the split is clamped, its scores discarded
        cp[c] = codes + ((size_t)min(b + c, b_hi - 1) * M4) * kPqBlock + lane;
      float acc[kPqChains];
      uint32_t w[kPqChains], wn[kPqChains];
#pragma unroll
      for (int c = 0; c < kPqChains; ++c) w[c] = cp[c][0];
      // the codes of the next four sub-spaces are loaded before the gathers of these four
      auto four = [&](int m4, bool first) {
#pragma unroll
        for (int c = 0; c < kPqChains; ++c) wn[c] = cp[c][(size_t)min(m4 + 1, M4 - 1) * kPqBlock];
        const float* t = smem + m4 * 4 * kPqCodewords;
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
          for (int c = 0; c < kPqChains; ++c) {
            const float v = t[e * kPqCodewords + ((w[c] >> (8 * e)) & 255u)];
            acc[c] = (first && e == 0) ? v : acc[c] + v;  // the chain starts at lut[0][code_0]
          }
#pragma unroll
        for (int c = 0; c < kPqChains; ++c) w[c] = wn[c];
      };
      four(0, true);
      for (int m4 = 1; m4 < M4; ++m4) four(m4, false);
#pragma unroll
      for (int c = 0; c < kPqChains; ++c) {
        const int row = (b + c) * kPqBlock + lane;
        const bool live = b + c < b_hi && row < N;
        const float v = live ? acc[c] : -__builtin_inff();
        const int id = live ? row : kNoRow;
        if (__ballot(better(v, id, tv[KM - 1], ti[KM - 1])) != 0) list_insert<KM>(tv, ti, v, id);
      }
    }

    // 64 lane lists -> the wave's sorted top-KM in lanes 0 .. KM - 1 -> LDS
    float rv;
    int ri;
    wave_topk<KM>(tv, ti, rv, ri);
    if (lane < KM) wl[wave * KM + lane] = float2{rv, __int_as_float(ri)};
    __syncthreads();
    if (wave == 0) {  // 8 lanes, one wave list each: k rounds of "best head", the owner pops
      const float2* mine = wl + (lane & (kPqScanWaves - 1)) * KM;
      int pos = 0;
      for (int n = 0; n < k; ++n) {
        const float2 hd = mine[min(pos, KM - 1)];
        const float hv = pos < KM ? hd.x : -__builtin_inff();
        const int hi = pos < KM ? __float_as_int(hd.y) : kNoRow;
        float bv = hv;
        int bi = hi;
        auto step = [&](float ov, int oi) {
          if (better(ov, oi, bv, bi)) {
            bv = ov;
            bi = oi;
          }
        };
        step(dppf<kDppHalfMirror>(bv), dppi<kDppHalfMirror>(bi));
        step(dppf<kDppXor2>(bv), dppi<kDppXor2>(bi));
        step(dppf<kDppXor1>(bv), dppi<kDppXor1>(bi));
        if (hi == bi && bi != kNoRow) ++pos;  // rows are distinct: exactly one owner
        if (lane == 0) ws[((size_t)qi * P + split) * k + n] = float2{bv, __int_as_float(bi)};
      }
    }
    // wave 0 reaches the next barrier (after the table copy) only when its merge is done, and the wave
    // lists are written again after that barrier; the table region is not read by the merge
  }
}

size_t pq_scan_lds_bytes(int M, int KM) {
  return (size_t)M * kPqCodewords * sizeof(float) + (size_t)kPqScanWaves * KM * sizeof(float2);
}

template <int KM>
void pq_scan_launch(const float* lut, const uint32_t* codes, float2* ws, int nq, int N, int M, int k, int P, int bps,
                    hipStream_t stream) {
  const size_t lds = pq_scan_lds_bytes(M, KM);  // up to 130 KiB (M = 128, KM = 32); the attribute is per device
  ATPU_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&pq_scan_kernel<KM>),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL((pq_scan_kernel<KM>), dim3(P), dim3(kPqScanThreads), lds, stream, lut, codes, ws, nq, N, M, k, P,
                     bps);
  ATPU_HIP_CHECK(hipGetLastError());
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

bool pq_shape_ok(int D, int M) {
  if (M < 4 || M > kPqMaxSubvectors || M % 4 != 0 || D < M || D % M != 0) return false;
  const int dsub = D / M;
  return dsub == 4 || dsub == 8 || dsub == 16;
}

void pq_encode(const float* x, const float* codebooks, const float* bias, uint8_t* codes, int64_t n, int D, int M,
               hipStream_t stream) {
  ATPU_CHECK(pq_shape_ok(D, M), "pq_encode: D / M must be 4, 8 or 16 and M a multiple of 4 up to 128");
  ATPU_CHECK(n >= 1 && n <= 2147483647LL - 256, "pq_encode: n must be in [1, 2^31 - 256]");
  ATPU_CHECK(x && codebooks && bias && codes, "pq_encode: null tensor");
  ATPU_CHECK(aligned16(x) && aligned16(codebooks), "pq_encode: x and codebooks must be 16-byte aligned");
  const int64_t wgs = ((n + kPqThreads - 1) / kPqThreads) * M;
  ATPU_CHECK(wgs <= 2147483647LL, "pq_encode: too many workgroups");
  const dim3 grid((unsigned)wgs), block(kPqThreads);
  switch (D / M) {
    case 4: hipLaunchKernelGGL(pq_encode_kernel<4>, grid, block, 0, stream, x, codebooks, bias, codes, (int)n, D, M); break;
    case 8: hipLaunchKernelGGL(pq_encode_kernel<8>, grid, block, 0, stream, x, codebooks, bias, codes, (int)n, D, M); break;
    default: hipLaunchKernelGGL(pq_encode_kernel<16>, grid, block, 0, stream, x, codebooks, bias, codes, (int)n, D, M);
  }
  ATPU_HIP_CHECK(hipGetLastError());
}

void pq_lut(const float* q, const float* codebooks, float* lut, int nq, int D, int M, hipStream_t stream) {
  ATPU_CHECK(pq_shape_ok(D, M), "pq_lut: D / M must be 4, 8 or 16 and M a multiple of 4 up to 128");
  ATPU_CHECK(nq >= 1 && (int64_t)nq * M <= 2147483647LL, "pq_lut: nq must be >= 1 and nq * M below 2^31");
  ATPU_CHECK(q && codebooks && lut, "pq_lut: null tensor");
  ATPU_CHECK(aligned16(q) && aligned16(codebooks), "pq_lut: q and codebooks must be 16-byte aligned");
  const dim3 grid((unsigned)(nq * M)), block(kPqThreads);
  switch (D / M) {
    case 4: hipLaunchKernelGGL(pq_lut_kernel<4>, grid, block, 0, stream, q, codebooks, lut, D, M); break;
    case 8: hipLaunchKernelGGL(pq_lut_kernel<8>, grid, block, 0, stream, q, codebooks, lut, D, M); break;
    default: hipLaunchKernelGGL(pq_lut_kernel<16>, grid, block, 0, stream, q, codebooks, lut, D, M);
  }
  ATPU_HIP_CHECK(hipGetLastError());
}

int pq_scan_splits(int N, int want) {
  const int nblocks = (N + kPqBlock - 1) / kPqBlock;
  const int p = want < 1 ? 1 : (want > kSimMaxSplits ? kSimMaxSplits : want);
  const int bps = (nblocks + p - 1) / p;
  return (nblocks + bps - 1) / bps;  // no empty split
}

void pq_scan_partial(const float* lut, const uint8_t* codes, float* ws, int nq, int N, int M, int k, int P,
                     hipStream_t stream) {
  ATPU_CHECK(nq >= 1 && N >= 1 && N <= 2147483647 - 256, "pq_scan: nq >= 1 and N in [1, 2^31 - 256]");
  ATPU_CHECK(M >= 4 && M <= kPqMaxSubvectors && M % 4 == 0, "pq_scan: M must be a multiple of 4 in [4, 128]");
  ATPU_CHECK(k >= 1 && k <= 32, "pq_scan: k must be in [1, 32]");
  ATPU_CHECK(P >= 1 && P == pq_scan_splits(N, P), "pq_scan: P must come from pq_scan_splits");
  ATPU_CHECK(lut && codes && ws, "pq_scan: null tensor");
  ATPU_CHECK(aligned16(lut) && (reinterpret_cast<uintptr_t>(codes) & 3) == 0 &&
                 (reinterpret_cast<uintptr_t>(ws) & 7) == 0,
             "pq_scan: lut must be 16-byte, the codes 4-byte and the workspace 8-byte aligned");
  const int nblocks = (N + kPqBlock - 1) / kPqBlock;
  const int bps = (nblocks + P - 1) / P;
  const uint32_t* c = reinterpret_cast<const uint32_t*>(codes);
  float2* w = reinterpret_cast<float2*>(ws);
  if (k <= 8) pq_scan_launch<8>(lut, c, w, nq, N, M, k, P, bps, stream);
  else if (k <= 16) pq_scan_launch<16>(lut, c, w, nq, N, M, k, P, bps, stream);
  else pq_scan_launch<32>(lut, c, w, nq, N, M, k, P, bps, stream);
}

}  // namespace atpu
