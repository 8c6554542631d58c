// Top-k similarity search: scores = Q [nq, D] . C [N, D]^T in exact fp32 with the top-k taken in
// the epilogue, so the [nq, N] score matrix never exists. The only intermediate in global memory
// is the workspace of per-split partial lists [nq, P, k] (value, row), merged by a second kernel
// in the same total order (value desc, row asc: better() of atpu/topk.h). No atomics.
//
// sim_topk_kernel<KM, QH, NW>: one workgroup (NW waves) per (corpus split, tile of QT = 16 QH queries).
// The query tile sits in LDS (row stride D + 4 floats: the 16 query rows a ds_read_b128 touches
// start 4 banks apart). A wave streams pairs of 16-row corpus tiles through
// v_mfma_f32_16x16x4_f32 with the corpus as the A operand and 16 queries as B: 2 QH independent
// accumulators per wave cover the 40-cycle dependent latency, and each B fragment read from LDS
// serves both corpus tiles. In the C/D layout col = lane & 15 is the query and
// row = (lane >> 4) * 4 + reg the corpus row.
//
// k order of one dot product (a function of D alone): the columns go in chunks of 16; lane
// (r = lane & 15, g = lane >> 4) loads the 16 bytes c[row r][16 ch + 4 g .. + 3] and issues 4 MFMAs
// from them, MFMA j taking element j, so the hardware's k index g stands for column
// 16 ch + 4 g + j. The chain of a chunk is j-major: columns 0, 4, 8, 12, 1, 5, 9, 13, ... The query
// operand is read with the same map (16 bytes of q[col][16 ch + 4 g .. + 3] from LDS). One fp32
// accumulator per (query, row), fed in that order whatever the query's slot, the wave, the
// split, N or P: a pair's score has the same bits in every launch shape.
//
// Four chunks (64 columns: D % 64 == 0) of both corpus tiles are loaded one step ahead of the
// MFMAs that consume them, into two fragment buffers that take turns: 8 x 16 B in flight per lane.
//
// Each lane owns 8 scores of QH queries per step and keeps one sorted register list of KM >= k
// entries per query (list_insert). A wave-uniform ballot skips the insertion when no lane's
// score beats its own list tail, which after the first few tiles is nearly always. At the end of
// the split the 4 NW lists of a query (4 lane groups x NW waves) meet in LDS, where 4 NW lanes pop
// the best head k times (DPP butterfly inside the 16-lane row, one permlane swap before it for 32).
//
// NW: with 32 queries the LDS tile (96.5 KiB at D = 768) allows one workgroup per CU. Four waves
// are then one per SIMD with 8 loads in flight each, which does not cover the HBM latency
// (measured 4.0 TB/s of corpus); eight waves share the tile, two per SIMD (4.6 TB/s). KM = 32
// needs more than the 256 registers a wave has at two per SIMD and stays at four waves; the
// 16-query form fits three workgroups of four waves per CU as it is.
//
// Rows past the corpus (N % 32 != 0, N < 32): the row index is clamped to N - 1 and the score
// discarded by select, never multiplied by 0, so nothing outside c[0:N] is read. Query slots
// past nq are clamped the same way and never written.
#include "atpu/common.h"
#include "atpu/kernels.h"
#include "atpu/topk.h"

namespace atpu {
namespace {

constexpr int kSimThreads = 256;  // the merge kernel, and the search kernel with NW = 4 waves
constexpr int kSimWaves = kSimThreads / kWave;
constexpr int kSimRows = 32;    // corpus rows per wave step: two 16-row MFMA tiles
constexpr int kSimStep = 64;    // columns per load step
constexpr int kSimPad = 4;      // floats of padding per LDS query row
constexpr int kNoRow = 0x7fffffff;

struct SimFrag {
  f32x4 a[2][4];  // [corpus tile][chunk]
};

__device__ __forceinline__ void sim_load(SimFrag& f, const float* __restrict__ c, int D, int N, int row0, int r,
                                         int g, int kb) {
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int row = min(row0 + t * 16 + r, N - 1);  // clamp, the score is discarded by select
    const float* p = c + (size_t)row * D + kb + 4 * g;
#pragma unroll
    for (int ch = 0; ch < 4; ++ch) f.a[t][ch] = *reinterpret_cast<const f32x4*>(p + 16 * ch);
  }
}

template <int KM, int QH, int NW>
__global__ __launch_bounds__(NW * kWave) void sim_topk_kernel(const float* __restrict__ q,
                                                               const float* __restrict__ c,
                                                               float2* __restrict__ ws, int nq, int N, int D, int k,
                                                               int P, int steps_per_split) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int QT = 16 * QH;
  constexpr int L = 4 * NW;  // lists per query at the end of a split: 4 lane groups x NW waves
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int split = blockIdx.x, q0 = blockIdx.y * QT;
  const int ldq = D + kSimPad;

  // query tile -> LDS (slots past nq repeat the last query)
  const int c4 = D >> 2;
  for (int i = tid; i < QT * c4; i += NW * kWave) {
    const int qi = i / c4, cc = i - qi * c4;
    const int qr = min(q0 + qi, nq - 1);
    *reinterpret_cast<f32x4*>(smem + qi * ldq + cc * 4) = *reinterpret_cast<const f32x4*>(q + (size_t)qr * D + cc * 4);
  }
  __syncthreads();

  float tv[QH][KM];
  int ti[QH][KM];
#pragma unroll
  for (int h = 0; h < QH; ++h)
#pragma unroll
    for (int e = 0; e < KM; ++e) {
      tv[h][e] = -__builtin_inff();
      ti[h][e] = kNoRow;
    }

  const int nsteps = (N + kSimRows - 1) / kSimRows;
  const int s_lo = split * steps_per_split, s_hi = min(s_lo + steps_per_split, nsteps);
  const int KS = D / kSimStep;
  const float* qb = smem + r * ldq + 4 * g;

  // The wave's (rows, columns) steps form one stream; two fragment buffers take turns, and the
  // loads of step i + 1 are issued before the MFMAs of step i (the scheduling barrier keeps them
  // there): the next 64 columns, or the first 64 of this wave's next rows (clamped into c[0:N]).
  SimFrag f0, f1;
  int s = s_lo + wave, ks = 0;
  f32x4 acc[2][QH];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int h = 0; h < QH; ++h) acc[t][h] = f32x4{0.f, 0.f, 0.f, 0.f};
  if (s < s_hi) sim_load(f0, c, D, N, s * kSimRows, r, g, 0);
  auto stage = [&](const SimFrag& cur, SimFrag& nxt) {
    const bool last = ks + 1 == KS;
    const int ns = last ? s + NW : s, nks = last ? 0 : ks + 1;
    sim_load(nxt, c, D, N, ns * kSimRows, r, g, nks * kSimStep);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int ch = 0; ch < 4; ++ch) {
      f32x4 b[QH];
#pragma unroll
      for (int h = 0; h < QH; ++h)
        b[h] = *reinterpret_cast<const f32x4*>(qb + h * 16 * ldq + ks * kSimStep + 16 * ch);
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int h = 0; h < QH; ++h)
            acc[t][h] = __builtin_amdgcn_mfma_f32_16x16x4f32(cur.a[t][ch][j], b[h][j], acc[t][h], 0, 0, 0);
    }
    if (last) {  // the rows' scores are complete: into the lists
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int row = s * kSimRows + t * 16 + g * 4 + e;
          const bool live = row < N;
#pragma unroll
          for (int h = 0; h < QH; ++h) {
            const float v = live ? acc[t][h][e] : -__builtin_inff();
            const int id = live ? row : kNoRow;
            if (__ballot(better(v, id, tv[h][KM - 1], ti[h][KM - 1])) != 0) list_insert<KM>(tv[h], ti[h], v, id);
          }
        }
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int h = 0; h < QH; ++h) acc[t][h] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    s = ns;
    ks = nks;
  };
  while (s < s_hi) {
    stage(f0, f1);
    if (s < s_hi) stage(f1, f0);
  }

  // the L lists of every query -> LDS (over the query tile, which is no longer read)
  __syncthreads();
  float2* ml = reinterpret_cast<float2*>(smem);
#pragma unroll
  for (int h = 0; h < QH; ++h) {
    float2* dst = ml + ((h * 16 + r) * L + wave * 4 + g) * KM;
#pragma unroll
    for (int e = 0; e < KM; ++e) dst[e] = float2{tv[h][e], __int_as_float(ti[h][e])};
  }
  __syncthreads();
  // L lanes per query (64 / L queries per wave), one list each: k rounds of "best head", the owner pops
  const int li = lane & (L - 1);
#pragma unroll
  for (int h = 0; h < QH; ++h) {
    const int qi = h * 16 + wave * (kWave / L) + lane / L;
    const float2* src = ml + (qi * L + li) * KM;
    int pos = 0;
    for (int n = 0; n < k; ++n) {
      const float2 hd = src[min(pos, KM - 1)];
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
      if constexpr (L == 32) step(xor16f(bv), xor16i(bi));
      step(dppf<kDppMirror>(bv), dppi<kDppMirror>(bi));
      step(dppf<kDppHalfMirror>(bv), dppi<kDppHalfMirror>(bi));
      step(dppf<kDppXor2>(bv), dppi<kDppXor2>(bi));
      step(dppf<kDppXor1>(bv), dppi<kDppXor1>(bi));
      if (hi == bi && bi != kNoRow) ++pos;  // rows are distinct: exactly one owner
      if (li == 0 && q0 + qi < nq) ws[((size_t)(q0 + qi) * P + split) * k + n] = float2{bv, __int_as_float(bi)};
    }
  }
}

// One workgroup per query: thread t owns the sorted partial list of split t (P <= 256); k rounds
// of "best head" over the workgroup (wave butterfly, then the 4 wave results through LDS).
__global__ __launch_bounds__(kSimThreads) void sim_topk_merge_kernel(const float2* __restrict__ ws,
                                                                     float* __restrict__ scores,
                                                                     int64_t* __restrict__ ids, int P, int k, int kk,
                                                                     int64_t id_base) {
  __shared__ float wv[2][kSimWaves];
  __shared__ int wi[2][kSimWaves];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int qi = blockIdx.x;
  const float2* src = ws + ((size_t)qi * P + min(tid, P - 1)) * k;
  int pos = tid < P ? 0 : k;
  for (int n = 0; n < kk; ++n) {
    const float2 hd = src[min(pos, k - 1)];
    const float hv = pos < k ? hd.x : -__builtin_inff();
    const int hi = pos < k ? __float_as_int(hd.y) : kNoRow;
    float bv = hv;
    int bi = hi;
    auto step = [&](float ov, int oi) {
      if (better(ov, oi, bv, bi)) {
        bv = ov;
        bi = oi;
      }
    };
    step(xor32f(bv), xor32i(bi));
    step(xor16f(bv), xor16i(bi));
    step(dppf<kDppMirror>(bv), dppi<kDppMirror>(bi));
    step(dppf<kDppHalfMirror>(bv), dppi<kDppHalfMirror>(bi));
    step(dppf<kDppXor2>(bv), dppi<kDppXor2>(bi));
    step(dppf<kDppXor1>(bv), dppi<kDppXor1>(bi));
    const int buf = n & 1;  // alternating buffers: one barrier per round
    if (lane == 0) {
      wv[buf][wave] = bv;
      wi[buf][wave] = bi;
    }
    __syncthreads();
    bv = wv[buf][0];
    bi = wi[buf][0];
#pragma unroll
    for (int w = 1; w < kSimWaves; ++w) step(wv[buf][w], wi[buf][w]);
    if (hi == bi && bi != kNoRow) ++pos;
    if (tid == 0) {
      scores[(size_t)qi * kk + n] = bv;
      ids[(size_t)qi * kk + n] = id_base + bi;
    }
  }
}

size_t sim_lds_bytes(int D, int KM, int QT, int NW) {
  const size_t qbytes = (size_t)QT * (D + kSimPad) * sizeof(float);
  const size_t mbytes = (size_t)QT * 4 * NW * KM * sizeof(float2);
  return qbytes > mbytes ? qbytes : mbytes;
}

template <int KM, int QH, int NW>
void sim_launch(const float* q, const float* c, float2* ws, int nq, int N, int D, int k, int P, int sps,
                hipStream_t stream) {
  constexpr int QT = 16 * QH;
  const size_t lds = sim_lds_bytes(D, KM, QT, NW);
  // up to 128.5 KiB of dynamic LDS (D = 1024, 32 queries); the attribute is per device
  ATPU_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&sim_topk_kernel<KM, QH, NW>),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL((sim_topk_kernel<KM, QH, NW>), dim3(P, (nq + QT - 1) / QT), dim3(NW * kWave), lds, stream, q, c, ws,
                     nq, N, D, k, P, sps);
  ATPU_HIP_CHECK(hipGetLastError());
}

}  // namespace

int sim_topk_splits(int N, int want) {
  const int nsteps = (N + kSimRows - 1) / kSimRows;
  const int p = want < 1 ? 1 : (want > kSimMaxSplits ? kSimMaxSplits : want);
  const int sps = (nsteps + p - 1) / p;
  return (nsteps + sps - 1) / sps;  // no empty split
}

void sim_topk_partial(const float* q, const float* c, float* ws, int nq, int N, int D, int k, int P,
                      hipStream_t stream) {
  ATPU_CHECK(nq >= 1 && N >= 1, "sim_topk: nq and N must be >= 1");
  ATPU_CHECK(D % 64 == 0 && D >= 64 && D <= 1024, "sim_topk: D must be a multiple of 64 in [64, 1024]");
  ATPU_CHECK(k >= 1 && k <= 32, "sim_topk: k must be in [1, 32]");
  ATPU_CHECK(P >= 1 && P == sim_topk_splits(N, P), "sim_topk: P must come from sim_topk_splits");
  ATPU_CHECK(q && c && ws, "sim_topk: null tensor");
  ATPU_CHECK(((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(c)) & 15) == 0 &&
                 (reinterpret_cast<uintptr_t>(ws) & 7) == 0,
             "sim_topk: q and c must be 16-byte and the workspace 8-byte aligned");
  const int nsteps = (N + kSimRows - 1) / kSimRows;
  const int sps = (nsteps + P - 1) / P;
  float2* w = reinterpret_cast<float2*>(ws);
  const bool wide = nq > 16;  // one or two 16-query halves per workgroup
  // 32 queries: the LDS query tile allows one workgroup per CU, so it has 8 waves (two per SIMD,
  // 16 x 16 B in flight per SIMD lane) where the registers allow it (KM <= 16: 256 per wave)
#define ATPU_SIM_CASE(KM, NWIDE)                                                \
  do {                                                                          \
    if (wide) sim_launch<KM, 2, NWIDE>(q, c, w, nq, N, D, k, P, sps, stream);   \
    else sim_launch<KM, 1, 4>(q, c, w, nq, N, D, k, P, sps, stream);            \
  } while (0)
  if (k <= 8) ATPU_SIM_CASE(8, 8);
  else if (k <= 16) ATPU_SIM_CASE(16, 8);
  else ATPU_SIM_CASE(32, 4);
#undef ATPU_SIM_CASE
}

void sim_topk_merge(const float* ws, float* scores, int64_t* ids, int nq, int P, int k, int kk, int64_t id_base,
                    hipStream_t stream) {
  ATPU_CHECK(nq >= 1 && P >= 1 && P <= kSimMaxSplits, "sim_topk_merge: P must be in [1, 256]");
  ATPU_CHECK(k >= 1 && k <= 32 && kk >= 1 && kk <= k, "sim_topk_merge: 1 <= kk <= k <= 32");
  ATPU_CHECK(ws && scores && ids, "sim_topk_merge: null tensor");
  hipLaunchKernelGGL(sim_topk_merge_kernel, dim3(nq), dim3(kSimThreads), 0, stream,
                     reinterpret_cast<const float2*>(ws), scores, ids, P, k, kk, id_base);
  ATPU_HIP_CHECK(hipGetLastError());
}

}  // namespace atpu
