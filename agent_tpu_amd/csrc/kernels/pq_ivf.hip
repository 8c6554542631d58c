// IVF-PQ (IVFADC): coarse k-means clusters and product-quantization codes of the residual x - centroid[label].
// The rows are sorted by cluster (row_ids [N] int32: the original row of a sorted row; offsets [K + 1] int32) and
// their codes are ONE interleaved PqCodes image over the sorted rows (pq.hip's layout: blocks of 64 rows); clusters
// are not padded, so a block at a cluster border belongs to two clusters. A query scores the rows of the nprobe
// clusters it probes only:
//
//     score(q, row) = (lut[0][code_0] + lut[1][code_1] + ... + lut[M-1][code_{M-1}]) + coarse(q, cluster(row))
//
// lut is pq_lut of the query against the residual codebooks: for inner products it depends on the query alone, so
// one table serves every probed cluster. coarse is dot(q, centroid) in a fixed order (pq_coarse below).
//
// pq_encode_residual_kernel<DSUB>: pq_encode_kernel with the subtraction in front. A lane loads its row's
// sub-vector and the same columns of its row's centroid, subtracts in registers (one rounding per column) and walks
// the 256 codewords in LDS; the residual rows never exist in memory. Ties and signed zeros as pq_encode.
//
// pq_coarse_kernel: coarse [nq, nprobe] for the probed clusters, 16 lanes per (query, slot). Lane j runs the chain
// of the separately rounded products of columns 64 s + 4 j + e (s ascending, then e = 0 .. 3); the 16 chains meet in
// a butterfly over the lane bits 1, 2, then the half-mirror and the mirror of the 16-lane row (fp32 adds commute, so
// every lane holds the same bits). The order is a function of D alone and the PyTorch twin repeats it; the probe's
// own MFMA score is not used because no twin has its bits.
//
// pq_scan_ivf_kernel<KM>: the hot path, query-stationary. A query's table is M KiB and an average cluster's codes
// are about as large, so grouping the work by cluster (sim_topk_ivf's items) would load a table per (query,
// cluster) pair and double the traffic; here workgroup (query, split) loads the query's table ONCE and walks that
// query's clusters. Grid (nq, S), 8 waves. LDS: the table [M][256] fp32, the 8 wave lists and a probe table of 32
// slots (about 131 KiB at M = 128, KM = 32: one workgroup per CU, two waves per SIMD).
//
// Prologue: all threads copy the table as f32x4; lanes 0 .. 31 of wave 0 take one probe slot each: cluster id and
// coarse score, lo / hi = offsets[c], offsets[c + 1] clamped into [0, N], the covering 64-row block range
// [lo / 64, ceil(hi / 64)) (no blocks for an empty cluster) and, by a wave scan, the prefix sums of the block counts.
//
// Walk: the query's virtual block sequence is the slots' block ranges back to back in slot order; split s takes the
// contiguous share [s * per, (s + 1) * per), per = ceil(total / S). A wave takes kPqChains = 4 virtual blocks per
// step; each maps to (slot, block) by a binary search of the prefix sums (wave-uniform, broadcast LDS reads), so
// the chains of one step may lie in different clusters. A virtual block past the share is clamped to the share's
// last block and its scores are discarded by select. The gathers, the one-group-ahead code prefetch and the four
// independent add chains are pq_scan_kernel's.
//
// A row enters the lists only if lo_slot <= row < hi_slot (by select): a block shared by two probed clusters is
// visited once per slot and each of its rows is counted once. The id is row_ids[row] (clamped index), so the lists
// rank by the ORIGINAL row: (score desc, original id asc). list_insert behind a ballot, wave_topk, then 8 lanes of
// wave 0 merge the wave lists; the sorted top-k goes to ws[(q * S + split) * k], all (-inf, kNoRow) for an empty
// share, so every slot is written and sim_topk_merge reduces with P = S.
//
// Read bounds: nothing outside lut, probes / coarse [nq, nprobe], offsets[0 : K + 1], row_ids[0 : N] and the code
// blocks [0, ceil(N / 64)); a cluster id outside [0, K) counts as an empty cluster.
#include "atpu/common.h"
#include "atpu/kernels.h"
#include "atpu/pq.h"
#include "atpu/topk.h"

namespace atpu {
namespace {

constexpr int kNoRow = 0x7fffffff;
constexpr int kIvfPqSlots = 32;     // probe slots of the LDS table: nprobe <= 32
constexpr int kCoarseLanes = 16;    // lanes of one (query, slot) pair in pq_coarse_kernel
constexpr int kCoarseStep = 64;     // columns per step: 16 lanes x 4

template <int DSUB>
__global__ __launch_bounds__(kPqThreads) void pq_encode_residual_kernel(
    const float* __restrict__ x, const int* __restrict__ labels, const float* __restrict__ centroids,
    const float* __restrict__ cb, const float* __restrict__ bias, uint8_t* __restrict__ codes, int n, int D, int M,
    int K) {
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
  const int lab = max(0, min(labels[row], K - 1));  // a label outside [0, K) is clamped: nothing outside centroids
  float xv[DSUB];
  const f32x4* xp = reinterpret_cast<const f32x4*>(x + (size_t)row * D + m * DSUB);
  const f32x4* cp = reinterpret_cast<const f32x4*>(centroids + (size_t)lab * D + m * DSUB);
#pragma unroll
  for (int e = 0; e < DSUB / 4; ++e) {
    const f32x4 v = xp[e], c = cp[e];
#pragma unroll
    for (int j = 0; j < 4; ++j) xv[4 * e + j] = v[j] - c[j];  // the residual: one rounding, registers only
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

__global__ __launch_bounds__(kPqThreads) void pq_coarse_kernel(const float* __restrict__ q,
                                                               const float* __restrict__ centroids,
                                                               const int64_t* __restrict__ probes,
                                                               float* __restrict__ coarse, int pairs, int D, int K,
                                                               int nprobe) {
#pragma clang fp contract(off)
  const int tid = threadIdx.x, j = tid & (kCoarseLanes - 1);
  const int pair = blockIdx.x * (kPqThreads / kCoarseLanes) + tid / kCoarseLanes;
  const int p = min(pair, pairs - 1);  // a pair past the end repeats the last one (the DPP rows stay whole)
  const int64_t cl64 = probes[p];
  const int cl = (int)(cl64 < 0 ? 0 : (cl64 >= K ? K - 1 : cl64));
  const float* qp = q + (size_t)(p / nprobe) * D + 4 * j;
  const float* cp = centroids + (size_t)cl * D + 4 * j;
  float acc = 0.f;
  for (int s = 0; s < D / kCoarseStep; ++s) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(qp + s * kCoarseStep);
    const f32x4 b = *reinterpret_cast<const f32x4*>(cp + s * kCoarseStep);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float pr = a[e] * b[e];
      acc = (s == 0 && e == 0) ? pr : acc + pr;  // the chain starts at its first product
    }
  }
  acc = acc + dppf<kDppXor1>(acc);
  acc = acc + dppf<kDppXor2>(acc);
  acc = acc + dppf<kDppHalfMirror>(acc);
  acc = acc + dppf<kDppMirror>(acc);
  if (j == 0 && pair < pairs) coarse[pair] = acc;
}

template <int KM>
__global__ __launch_bounds__(kPqScanThreads) void pq_scan_ivf_kernel(
    const float* __restrict__ lut, const uint32_t* __restrict__ codes, const int* __restrict__ row_ids,
    const int* __restrict__ offsets, const int64_t* __restrict__ probes, const float* __restrict__ coarse,
    float2* __restrict__ ws, int N, int M, int k, int K, int nprobe, int S) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float2* wl = reinterpret_cast<float2*>(smem + M * kPqCodewords);  // [kPqScanWaves][KM] wave lists
  int* p_lo = reinterpret_cast<int*>(wl + kPqScanWaves * KM);       // [32] first row of the slot's cluster
  int* p_hi = p_lo + kIvfPqSlots;                                   // [32] one past its last row
  int* p_b0 = p_hi + kIvfPqSlots;                                   // [32] its first 64-row block
  int* p_pre = p_b0 + kIvfPqSlots;                                  // [33] blocks of the slots before it; [32]: all
  float* p_co = reinterpret_cast<float*>(p_pre + kIvfPqSlots + 1);  // [32] its coarse score
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int qi = blockIdx.x, split = blockIdx.y;
  const int M4 = M >> 2;
  const int nblocks = (N + kPqBlock - 1) / kPqBlock;

  // prologue: the query's table -> LDS, and one probe slot per lane of wave 0
  const f32x4* src = reinterpret_cast<const f32x4*>(lut + (size_t)qi * M * kPqCodewords);
  for (int i = tid; i < M * (kPqCodewords / 4); i += kPqScanThreads) reinterpret_cast<f32x4*>(smem)[i] = src[i];
  if (wave == 0) {
    const bool slot_ok = lane < nprobe;
    const size_t pi = (size_t)qi * nprobe + min(lane, nprobe - 1);
    const int64_t cl = probes[pi];
    const bool has = slot_ok && cl >= 0 && cl < K;
    const int c = has ? (int)cl : 0;
    const int lo = max(0, min(offsets[c], N));
    const int hi = has ? max(lo, min(offsets[c + 1], N)) : lo;
    const int nb = hi > lo ? (hi + kPqBlock - 1) / kPqBlock - lo / kPqBlock : 0;
    int inc = nb;  // inclusive scan over the lanes; lanes at or past nprobe add nothing
#pragma unroll
    for (int d = 1; d < kIvfPqSlots; d <<= 1) {
      const int t = __shfl_up(inc, d);
      if (lane >= d) inc += t;
    }
    if (lane < kIvfPqSlots) {
      p_lo[lane] = lo;
      p_hi[lane] = hi;
      p_b0[lane] = lo / kPqBlock;
      p_pre[lane] = inc - nb;
      p_co[lane] = coarse[pi];
      if (lane == kIvfPqSlots - 1) p_pre[kIvfPqSlots] = inc;
    }
  }
  __syncthreads();

  float tv[KM];
  int ti[KM];
#pragma unroll
  for (int e = 0; e < KM; ++e) {
    tv[e] = -__builtin_inff();
    ti[e] = kNoRow;
  }

  // this split's share of the query's virtual blocks
  const int total = p_pre[kIvfPqSlots];
  const int per = (total + S - 1) / S;
  const int v_lo = min(split * per, total), v_hi = min(v_lo + per, total);
  for (int v = v_lo + wave * kPqChains; v < v_hi; v += kPqScanWaves * kPqChains) {
    const uint32_t* cp[kPqChains];
    int row[kPqChains], rid[kPqChains], slot[kPqChains];
#pragma unroll
    for (int c = 0; c < kPqChains; ++c) {
      const int vb = min(v + c, v_hi - 1);  // past the share: clamped, the scores discarded
      int s_lo = 0, s_hi = nprobe;          // the last slot whose prefix is <= vb: it holds vb, so it is not empty
      while (s_hi - s_lo > 1) {
        const int mid = (s_lo + s_hi) >> 1;
        if (p_pre[mid] <= vb) s_lo = mid;
        else s_hi = mid;
      }
      slot[c] = s_lo;
      const int blk = max(0, min(p_b0[s_lo] + (vb - p_pre[s_lo]), nblocks - 1));
      cp[c] = codes + ((size_t)blk * M4) * kPqBlock + lane;
      row[c] = blk * kPqBlock + lane;
      rid[c] = row_ids[min(row[c], N - 1)];  // the original row, ahead of the gathers
    }
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
          const float x = t[e * kPqCodewords + ((w[c] >> (8 * e)) & 255u)];
          acc[c] = (first && e == 0) ? x : pq_add(acc[c], x);  // the chain starts at lut[0][code_0]
        }
#pragma unroll
      for (int c = 0; c < kPqChains; ++c) w[c] = wn[c];
    };
    four(0, true);
    for (int m4 = 1; m4 < M4; ++m4) four(m4, false);
#pragma unroll
    for (int c = 0; c < kPqChains; ++c) {
      const bool live = v + c < v_hi && row[c] >= p_lo[slot[c]] && row[c] < p_hi[slot[c]];
      const float x = live ? pq_add(acc[c], p_co[slot[c]]) : -__builtin_inff();
      const int id = live ? rid[c] : kNoRow;
      if (__ballot(better(x, id, tv[KM - 1], ti[KM - 1])) != 0) list_insert<KM>(tv, ti, x, id);
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
    float2* out = ws + ((size_t)qi * S + split) * k;
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
      if (hi == bi && bi != kNoRow) ++pos;  // original rows are distinct: exactly one owner
      if (lane == 0) out[n] = float2{bv, __int_as_float(bi)};
    }
  }
}

size_t pq_scan_ivf_lds_bytes(int M, int KM) {
  return (size_t)M * kPqCodewords * sizeof(float) + (size_t)kPqScanWaves * KM * sizeof(float2) +
         (size_t)(5 * kIvfPqSlots + 1) * sizeof(int);
}

template <int KM, typename... Args>
void pq_scan_ivf_launch(int nq, int S, int M, hipStream_t stream, Args... args) {
  const size_t lds = pq_scan_ivf_lds_bytes(M, KM);  // up to 131 KiB (M = 128, KM = 32); the attribute is per device
  ATPU_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&pq_scan_ivf_kernel<KM>),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL((pq_scan_ivf_kernel<KM>), dim3(nq, S), dim3(kPqScanThreads), lds, stream, args...);
  ATPU_HIP_CHECK(hipGetLastError());
}

bool aligned(const void* p, uintptr_t bytes) { return (reinterpret_cast<uintptr_t>(p) & (bytes - 1)) == 0; }

}  // namespace

void pq_encode_residual(const float* x, const int32_t* labels, const float* centroids, const float* codebooks,
                        const float* bias, uint8_t* codes, int64_t n, int D, int M, int K, hipStream_t stream) {
  ATPU_CHECK(pq_shape_ok(D, M), "pq_encode_residual: D / M must be 4, 8 or 16 and M a multiple of 4 up to 128");
  ATPU_CHECK(n >= 1 && n <= 2147483647LL - 256, "pq_encode_residual: n must be in [1, 2^31 - 256]");
  ATPU_CHECK(K >= 1 && K <= kKmeansMaxK, "pq_encode_residual: K must be in [1, 4096]");
  ATPU_CHECK(x && labels && centroids && codebooks && bias && codes, "pq_encode_residual: null tensor");
  ATPU_CHECK(aligned(x, 16) && aligned(centroids, 16) && aligned(codebooks, 16) && aligned(labels, 4),
             "pq_encode_residual: x, centroids and codebooks must be 16-byte, labels 4-byte aligned");
  const int64_t wgs = ((n + kPqThreads - 1) / kPqThreads) * M;
  ATPU_CHECK(wgs <= 2147483647LL, "pq_encode_residual: too many workgroups");
  const dim3 grid((unsigned)wgs), block(kPqThreads);
  switch (D / M) {
    case 4:
      hipLaunchKernelGGL(pq_encode_residual_kernel<4>, grid, block, 0, stream, x, labels, centroids, codebooks, bias,
                         codes, (int)n, D, M, K);
      break;
    case 8:
      hipLaunchKernelGGL(pq_encode_residual_kernel<8>, grid, block, 0, stream, x, labels, centroids, codebooks, bias,
                         codes, (int)n, D, M, K);
      break;
    default:
      hipLaunchKernelGGL(pq_encode_residual_kernel<16>, grid, block, 0, stream, x, labels, centroids, codebooks, bias,
                         codes, (int)n, D, M, K);
  }
  ATPU_HIP_CHECK(hipGetLastError());
}

void pq_coarse(const float* q, const float* centroids, const int64_t* probes, float* coarse, int nq, int D, int K,
               int nprobe, hipStream_t stream) {
  ATPU_CHECK(nq >= 1 && D >= 64 && D <= 1024 && D % kCoarseStep == 0, "pq_coarse: nq >= 1, D a multiple of 64 in [64, 1024]");
  ATPU_CHECK(K >= 1 && K <= kKmeansMaxK && nprobe >= 1 && nprobe <= kIvfPqSlots && nprobe <= K,
             "pq_coarse: K in [1, 4096], nprobe in [1, min(32, K)]");
  ATPU_CHECK((int64_t)nq * nprobe < (1ll << 30), "pq_coarse: nq * nprobe must be below 2^30");
  ATPU_CHECK(q && centroids && probes && coarse, "pq_coarse: null tensor");
  ATPU_CHECK(aligned(q, 16) && aligned(centroids, 16) && aligned(probes, 8) && aligned(coarse, 4),
             "pq_coarse: q and centroids must be 16-byte, probes 8-byte, coarse 4-byte aligned");
  const int pairs = nq * nprobe, per = kPqThreads / kCoarseLanes;
  hipLaunchKernelGGL(pq_coarse_kernel, dim3((pairs + per - 1) / per), dim3(kPqThreads), 0, stream, q, centroids, probes,
                     coarse, pairs, D, K, nprobe);
  ATPU_HIP_CHECK(hipGetLastError());
}

void pq_scan_ivf_partial(const float* lut, const uint8_t* codes, const int32_t* row_ids, const int32_t* offsets,
                         const int64_t* probes, const float* coarse, float* ws, int nq, int N, int M, int k, int K,
                         int nprobe, int S, hipStream_t stream) {
  ATPU_CHECK(nq >= 1 && N >= 1 && N <= 2147483647 - 256, "pq_scan_ivf: nq >= 1 and N in [1, 2^31 - 256]");
  ATPU_CHECK(M >= 4 && M <= kPqMaxSubvectors && M % 4 == 0, "pq_scan_ivf: M must be a multiple of 4 in [4, 128]");
  ATPU_CHECK(k >= 1 && k <= 32, "pq_scan_ivf: k must be in [1, 32]");
  ATPU_CHECK(K >= 1 && K <= kKmeansMaxK && nprobe >= 1 && nprobe <= kIvfPqSlots && nprobe <= K,
             "pq_scan_ivf: K in [1, 4096], nprobe in [1, min(32, K)]");
  ATPU_CHECK(S >= 1 && S <= kSimMaxSplits, "pq_scan_ivf: S must be in [1, 256]");
  ATPU_CHECK(lut && codes && row_ids && offsets && probes && coarse && ws, "pq_scan_ivf: null tensor");
  ATPU_CHECK(aligned(lut, 16) && aligned(codes, 4) && aligned(ws, 8) && aligned(probes, 8) && aligned(coarse, 4) &&
                 aligned(row_ids, 4) && aligned(offsets, 4),
             "pq_scan_ivf: lut must be 16-byte, ws and probes 8-byte, the codes and the int32 arrays 4-byte aligned");
  const uint32_t* c = reinterpret_cast<const uint32_t*>(codes);
  float2* w = reinterpret_cast<float2*>(ws);
  if (k <= 8) pq_scan_ivf_launch<8>(nq, S, M, stream, lut, c, row_ids, offsets, probes, coarse, w, N, M, k, K, nprobe, S);
  else if (k <= 16) pq_scan_ivf_launch<16>(nq, S, M, stream, lut, c, row_ids, offsets, probes, coarse, w, N, M, k, K, nprobe, S);
  else pq_scan_ivf_launch<32>(nq, S, M, stream, lut, c, row_ids, offsets, probes, coarse, w, N, M, k, K, nprobe, S);
}

}  // namespace atpu
