// IVF top-k similarity search: sim_topk (sim_topk.hip) over the rows of the clusters that each
// query probes, a different row set per query. The index is the corpus sorted by cluster:
// vectors [N, D] fp32, row_ids [N] int32 (the original row of a sorted row, ascending inside a
// cluster) and offsets [K + 1] int32 (cluster c is vectors[offsets[c] : offsets[c + 1]]; an empty
// cluster is legal).
//
// Plan (sim_topk_ivf_plan_kernel below, one launch, no copy back to the host): the nq * nprobe (query, probe slot) pairs
// are grouped by cluster into work items of at most 16 queries of ONE cluster: item_cluster [items]
// (negative: a surplus item of the launch bound, which exits at once), item_query [items, 16] and
// item_slot [items, 16] (negative slot: padding; its query repeats a valid one and is never
// written). Every pair belongs to exactly one item.
//
// sim_topk_ivf_kernel<KM>: one workgroup of four waves per (item, split), the 16-query form of
// sim_topk_kernel (its header holds the tile, the LDS image, the prefetch and the register notes)
// with three differences:
//
// Query tile. The 16 query rows are gathered into LDS through item_query.
//
// Step walk. The steps are the 32-row steps of `vectors` that cover [offsets[c], offsets[c + 1]);
// split `split` of S takes a contiguous share of them, and its waves interleave with the same
// one-step-ahead prefetch, clamped into vectors[0:N].
//
// Epilogue. Row `row` of a step enters the lists only if offsets[c] <= row < offsets[c + 1], by
// select, never by a multiplication: a NaN in a neighbouring cluster's row of the same step cannot
// leak. Its id is row_ids[row] (an int32 load with a clamped index, issued at the head of the
// row step's last stage, before the corpus loads), so the lists rank by the ORIGINAL row and the
// (score desc, id asc) order is that of the exact search.
//
// Score bits: the chunk map, the j-major MFMA chain and the one-accumulator-per-pair rule are those
// of sim_topk_kernel, so a (query, row) score has sim_topk's bits.
//
// The partial list of (query, slot, split) goes to ws[((query * nprobe + slot) * S + split) * k]: for
// one query that is nprobe * S sorted lists, which sim_topk_merge merges as P = nprobe * S splits.
// A split without steps, or an empty cluster, writes an all (-inf, kNoRow) list, so every
// workspace slot is written.
//
// Read bounds: nothing outside q[0:nq], vectors[0:N], row_ids[0:N], offsets[0:K + 1] and the plan
// arrays is read; a cluster, a query, a slot or an offset outside its range is clamped or skipped.
#include "atpu/common.h"
#include "atpu/kernels.h"
#include "atpu/topk.h"

namespace atpu {
namespace {

constexpr int kSimRows = 32;  // corpus rows per wave step: two 16-row MFMA tiles
constexpr int kSimStep = 64;  // columns per load step
constexpr int kSimPad = 4;    // floats of padding per LDS query row
constexpr int kNoRow = 0x7fffffff;
constexpr int kIvfWaves = 4;
constexpr int QT = kIvfItemQueries;

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

template <int KM>
__global__ __launch_bounds__(kIvfWaves * kWave) void sim_topk_ivf_kernel(
    const float* __restrict__ q, const float* __restrict__ c, const int* __restrict__ row_ids,
    const int* __restrict__ offsets, const int* __restrict__ item_cluster, const int* __restrict__ item_query,
    const int* __restrict__ item_slot, float2* __restrict__ ws, int nq, int N, int D, int k, int K, int nprobe, int S) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int NW = kIvfWaves;
  constexpr int L = 4 * NW;  // lists per query at the end of a split: 4 lane groups x NW waves
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 15, g = lane >> 4;
  const int item = blockIdx.x, split = blockIdx.y;
  const int cl = item_cluster[item];
  if (cl < 0 || cl >= K) return;  // a surplus item of the launch bound: the whole workgroup, before any barrier
  const int lo = max(0, min(offsets[cl], N)), hi = max(lo, min(offsets[cl + 1], N));
  const int* iq = item_query + (size_t)item * QT;
  const int* is = item_slot + (size_t)item * QT;
  const int ldq = D + kSimPad;

  // query tile -> LDS, gathered through the item's query list
  const int c4 = D >> 2;
  for (int i = tid; i < QT * c4; i += NW * kWave) {
    const int qi = i / c4, cc = i - qi * c4;
    const int qr = max(0, min(iq[qi], nq - 1));
    *reinterpret_cast<f32x4*>(smem + qi * ldq + cc * 4) = *reinterpret_cast<const f32x4*>(q + (size_t)qr * D + cc * 4);
  }
  __syncthreads();

  float tv[KM];
  int ti[KM];
#pragma unroll
  for (int e = 0; e < KM; ++e) {
    tv[e] = -__builtin_inff();
    ti[e] = kNoRow;
  }

  // the 32-row steps of `vectors` that cover [lo, hi), and this split's contiguous share of them
  const int s_first = lo / kSimRows, s_end = hi > lo ? (hi + kSimRows - 1) / kSimRows : s_first;
  const int per = (s_end - s_first + S - 1) / S;
  const int s_lo = s_first + split * per, s_hi = min(s_lo + per, s_end);
  const int KS = D / kSimStep;
  const float* qb = smem + r * ldq + 4 * g;

  // sim_topk_kernel's stream of (rows, columns) steps: two fragment buffers take turns, the loads
  // of step i + 1 are issued before the MFMAs of step i (clamped into c[0:N])
  SimFrag f0, f1;
  int s = s_lo + wave, ks = 0;
  f32x4 acc[2];
  acc[0] = f32x4{0.f, 0.f, 0.f, 0.f};
  acc[1] = f32x4{0.f, 0.f, 0.f, 0.f};
  if (s < s_hi) sim_load(f0, c, D, N, s * kSimRows, r, g, 0);
  auto stage = [&](const SimFrag& cur, SimFrag& nxt) {
    const bool last = ks + 1 == KS;
    const int ns = last ? s + NW : s, nks = last ? 0 : ks + 1;
    int rid[2][4];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int e = 0; e < 4; ++e) rid[t][e] = kNoRow;
    if (last) {  // the original rows of this step, ahead of the corpus loads
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int e = 0; e < 4; ++e) rid[t][e] = row_ids[min(s * kSimRows + t * 16 + g * 4 + e, N - 1)];
    }
    __builtin_amdgcn_sched_barrier(0);
    sim_load(nxt, c, D, N, ns * kSimRows, r, g, nks * kSimStep);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int ch = 0; ch < 4; ++ch) {
      const f32x4 b = *reinterpret_cast<const f32x4*>(qb + ks * kSimStep + 16 * ch);
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int t = 0; t < 2; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(cur.a[t][ch][j], b[j], acc[t], 0, 0, 0);
    }
    if (last) {  // the rows' scores are complete: the cluster's rows into the lists, under their original ids
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int row = s * kSimRows + t * 16 + g * 4 + e;
          const bool live = row >= lo && row < hi;
          const float v = live ? acc[t][e] : -__builtin_inff();
          const int id = live ? rid[t][e] : kNoRow;
          if (__ballot(better(v, id, tv[KM - 1], ti[KM - 1])) != 0) list_insert<KM>(tv, ti, v, id);
        }
      acc[0] = f32x4{0.f, 0.f, 0.f, 0.f};
      acc[1] = f32x4{0.f, 0.f, 0.f, 0.f};
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
  {
    float2* dst = ml + (r * L + wave * 4 + g) * KM;
#pragma unroll
    for (int e = 0; e < KM; ++e) dst[e] = float2{tv[e], __int_as_float(ti[e])};
  }
  __syncthreads();
  // L lanes per query (four queries per wave), one list each: k rounds of "best head", the owner pops
  const int li = lane & (L - 1);
  const int qi = wave * (kWave / L) + lane / L;
  const int qr = iq[qi], slot = is[qi];
  const bool valid = qr >= 0 && qr < nq && slot >= 0 && slot < nprobe;  // a padding slot never writes
  float2* out = ws + (((size_t)max(qr, 0) * nprobe + max(slot, 0)) * S + split) * k;
  const float2* src = ml + (qi * L + li) * KM;
  int pos = 0;
  for (int n = 0; n < k; ++n) {
    const float2 hd = src[min(pos, KM - 1)];
    const float hv = pos < KM ? hd.x : -__builtin_inff();
    const int hi_ = pos < KM ? __float_as_int(hd.y) : kNoRow;
    float bv = hv;
    int bi = hi_;
    auto step = [&](float ov, int oi) {
      if (better(ov, oi, bv, bi)) {
        bv = ov;
        bi = oi;
      }
    };
    step(dppf<kDppMirror>(bv), dppi<kDppMirror>(bi));
    step(dppf<kDppHalfMirror>(bv), dppi<kDppHalfMirror>(bi));
    step(dppf<kDppXor2>(bv), dppi<kDppXor2>(bi));
    step(dppf<kDppXor1>(bv), dppi<kDppXor1>(bi));
    if (hi_ == bi && bi != kNoRow) ++pos;  // original rows are distinct: exactly one owner
    if (li == 0 && valid) out[n] = float2{bv, __int_as_float(bi)};
  }
}

// The plan in one launch of one workgroup: a histogram of the pairs' clusters in LDS, an exclusive scan of
// ceil(count / 16) over the clusters (a cluster's first item), then every pair takes the next free slot of its
// cluster through an LDS counter. Which slot a pair gets inside its cluster depends on the order of the atomics;
// the search does not: the list of a (query, slot) pair is computed and stored on its own. Surplus items keep
// cluster -1, padding slots -1 and the query of the item's slot 0 (always a real pair).
constexpr int kPlanThreads = 1024;

__global__ __launch_bounds__(kPlanThreads) void sim_topk_ivf_plan_kernel(const int64_t* __restrict__ probes, int M,
                                                                          int nprobe, int K, int items,
                                                                          int* __restrict__ item_cluster,
                                                                          int* __restrict__ item_query,
                                                                          int* __restrict__ item_slot) {
  __shared__ int cnt[kKmeansMaxK];
  __shared__ int first[kKmeansMaxK];
  __shared__ int part[kPlanThreads];
  const int tid = threadIdx.x;
  for (int c = tid; c < K; c += kPlanThreads) cnt[c] = 0;
  for (int i = tid; i < items; i += kPlanThreads) item_cluster[i] = -1;
  for (int i = tid; i < items * QT; i += kPlanThreads) {
    item_query[i] = 0;
    item_slot[i] = -1;
  }
  __syncthreads();
  for (int p = tid; p < M; p += kPlanThreads) {
    const int64_t c = probes[p];
    if (c >= 0 && c < K) atomicAdd(&cnt[(int)c], 1);
  }
  __syncthreads();
  // exclusive scan of the clusters' item counts: a contiguous chunk of clusters per thread, then over the threads
  const int per = (K + kPlanThreads - 1) / kPlanThreads;
  const int c_lo = min(tid * per, K), c_hi = min(c_lo + per, K);
  int mine = 0;
  for (int c = c_lo; c < c_hi; ++c) mine += (cnt[c] + QT - 1) / QT;
  part[tid] = mine;
  __syncthreads();
  for (int d = 1; d < kPlanThreads; d <<= 1) {
    const int v = tid >= d ? part[tid - d] : 0;
    __syncthreads();
    part[tid] += v;
    __syncthreads();
  }
  int run = part[tid] - mine;
  for (int c = c_lo; c < c_hi; ++c) {
    first[c] = run;
    run += (cnt[c] + QT - 1) / QT;
    cnt[c] = 0;  // from here on: the cluster's pairs placed so far (only this thread touched cnt[c] since the barrier)
  }
  __syncthreads();
  for (int p = tid; p < M; p += kPlanThreads) {
    const int64_t c = probes[p];
    if (c < 0 || c >= K) continue;
    const int rank = atomicAdd(&cnt[(int)c], 1);
    const int item = first[(int)c] + rank / QT;
    if (item >= items) continue;  // cannot happen within the launch bound
    item_cluster[item] = (int)c;
    item_query[item * QT + rank % QT] = p / nprobe;
    item_slot[item * QT + rank % QT] = p % nprobe;
  }
  __syncthreads();
  for (int i = tid; i < items * QT; i += kPlanThreads)
    if (item_slot[i] < 0 && item_cluster[i / QT] >= 0) item_query[i] = item_query[i / QT * QT];
}

size_t ivf_lds_bytes(int D, int KM) {
  const size_t qbytes = (size_t)QT * (D + kSimPad) * sizeof(float);
  const size_t mbytes = (size_t)QT * 4 * kIvfWaves * KM * sizeof(float2);
  return qbytes > mbytes ? qbytes : mbytes;
}

template <int KM, typename... Args>
void ivf_launch(int items, int S, int D, hipStream_t stream, Args... args) {
  const size_t lds = ivf_lds_bytes(D, KM);  // at most 65 KiB (D = 1024)
  ATPU_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&sim_topk_ivf_kernel<KM>),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL((sim_topk_ivf_kernel<KM>), dim3(items, S), dim3(kIvfWaves * kWave), lds, stream, args...);
  ATPU_HIP_CHECK(hipGetLastError());
}

}  // namespace

int64_t sim_topk_ivf_items(int64_t nq, int nprobe, int K) {
  const int64_t pairs = nq * nprobe;
  return (pairs < K ? pairs : K) + pairs / kIvfItemQueries;
}

void sim_topk_ivf_plan(const int64_t* probes, int nq, int nprobe, int K, int items, int32_t* item_cluster,
                       int32_t* item_query, int32_t* item_slot, hipStream_t stream) {
  ATPU_CHECK(nq >= 1 && nprobe >= 1 && nprobe <= 32 && K >= 1 && K <= kKmeansMaxK && nprobe <= K,
             "sim_topk_ivf_plan: nq >= 1, K in [1, 4096], nprobe in [1, min(32, K)]");
  ATPU_CHECK((int64_t)nq * nprobe < (1ll << 30) && items == sim_topk_ivf_items(nq, nprobe, K) && items <= (1 << 26),
             "sim_topk_ivf_plan: items must be sim_topk_ivf_items(nq, nprobe, K), at most 2^26");
  ATPU_CHECK(probes && item_cluster && item_query && item_slot, "sim_topk_ivf_plan: null tensor");
  ATPU_CHECK((reinterpret_cast<uintptr_t>(probes) & 7) == 0 &&
                 ((reinterpret_cast<uintptr_t>(item_cluster) | reinterpret_cast<uintptr_t>(item_query) |
                   reinterpret_cast<uintptr_t>(item_slot)) & 3) == 0,
             "sim_topk_ivf_plan: probes must be 8-byte, the int32 arrays 4-byte aligned");
  hipLaunchKernelGGL(sim_topk_ivf_plan_kernel, dim3(1), dim3(kPlanThreads), 0, stream, probes, nq * nprobe, nprobe, K,
                     items, item_cluster, item_query, item_slot);
  ATPU_HIP_CHECK(hipGetLastError());
}

void sim_topk_ivf_partial(const float* q, const float* vectors, const int32_t* row_ids, const int32_t* offsets,
                          const int32_t* item_cluster, const int32_t* item_query, const int32_t* item_slot, float* ws,
                          int nq, int N, int D, int k, int K, int nprobe, int S, int items, hipStream_t stream) {
  ATPU_CHECK(nq >= 1 && N >= 1, "sim_topk_ivf: nq and N must be >= 1");
  ATPU_CHECK(D % 64 == 0 && D >= 64 && D <= 1024, "sim_topk_ivf: D must be a multiple of 64 in [64, 1024]");
  ATPU_CHECK(k >= 1 && k <= 32, "sim_topk_ivf: k must be in [1, 32]");
  ATPU_CHECK(K >= 1 && K <= kKmeansMaxK, "sim_topk_ivf: K must be in [1, 4096]");
  ATPU_CHECK(nprobe >= 1 && nprobe <= 32 && nprobe <= K, "sim_topk_ivf: nprobe must be in [1, min(32, K)]");
  ATPU_CHECK(S >= 1 && nprobe * S <= kSimMaxSplits, "sim_topk_ivf: nprobe * S must be in [1, 256]");
  ATPU_CHECK(items >= 1 && items <= sim_topk_ivf_items(nq, nprobe, K) && sim_topk_ivf_items(nq, nprobe, K) < (1ll << 31),
             "sim_topk_ivf: items must be in [1, sim_topk_ivf_items(nq, nprobe, K)]");
  ATPU_CHECK(q && vectors && row_ids && offsets && item_cluster && item_query && item_slot && ws,
             "sim_topk_ivf: null tensor");
  ATPU_CHECK(((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(vectors)) & 15) == 0 &&
                 (reinterpret_cast<uintptr_t>(ws) & 7) == 0 &&
                 ((reinterpret_cast<uintptr_t>(row_ids) | reinterpret_cast<uintptr_t>(offsets) |
                   reinterpret_cast<uintptr_t>(item_cluster) | reinterpret_cast<uintptr_t>(item_query) |
                   reinterpret_cast<uintptr_t>(item_slot)) & 3) == 0,
             "sim_topk_ivf: q and vectors must be 16-byte, the workspace 8-byte, the int32 arrays 4-byte aligned");
  float2* w = reinterpret_cast<float2*>(ws);
  if (k <= 8)
    ivf_launch<8>(items, S, D, stream, q, vectors, row_ids, offsets, item_cluster, item_query, item_slot, w, nq, N, D, k, K,
                  nprobe, S);
  else if (k <= 16)
    ivf_launch<16>(items, S, D, stream, q, vectors, row_ids, offsets, item_cluster, item_query, item_slot, w, nq, N, D, k,
                   K, nprobe, S);
  else
    ivf_launch<32>(items, S, D, stream, q, vectors, row_ids, offsets, item_cluster, item_query, item_slot, w, nq, N, D, k,
                   K, nprobe, S);
}

}  // namespace atpu
