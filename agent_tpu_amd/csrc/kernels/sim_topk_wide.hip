// Deep top-k similarity search: sim_topk's exact scores with result lists of up to 1024 entries.
// scores = Q [nq, D] . C [N, D]^T (C fp32, or fp16 widened in registers and optionally times an fp32
// row_scale), the [nq, N] matrix never written, the exact top-k in (value desc, row asc) order
// (better() of atpu/topk.h). sim_topk keeps each list in registers (list_insert<KM>, KM <= 32); that
// does not stretch to k = 1024, so the selection here is a threshold filter in front of a buffer
// that is sorted only when it fills.
//
// sim_topk_wide_kernel<HALF, SC>: one workgroup of 4 waves per (corpus split, tile of 16 queries). The
// query tile sits in LDS and a wave streams 32-row steps against it exactly as the 16-query forms
// of sim_topk.hip (fp32: chunks of 16 columns, j-major; row stride D + 4 floats) and sim_topk_f16.hip
// (HALF: chunks of 32 columns, the permuted tile image, row stride D + 8 floats; SC: the finished
// accumulator times row_scale[row]) do: the same loads one step ahead into two fragment buffers,
// the same v_mfma_f32_16x16x4_f32 chain into ONE accumulator per (query, row), so a pair's score
// has the bits sim_topk gives it, whatever the split, the wave or the batch. No barrier in the loop.
//
// Selection, per wave and query (col = lane & 15 is the query in the C/D layout, so the 4 lanes
// r, r + 16, r + 32, r + 48 hold the 32 scores of query r of one step):
//   * a threshold (value, row) and a count, kept in the registers of those 4 lanes (the same values
//     in all four), starting at (-inf, kNoRow) and 0;
//   * a candidate buffer of CAP = 2 K2 (value, row) entries in a global workspace, K2 the power of
//     two >= max(k, 64). It is written once per passing score and read once per prune, by the same
//     wave: it lives in L2.
// Append: after a step's scores are complete a lane tests its 8 scores with better() against the
// threshold. A wave-uniform ballot skips everything when nothing passes, which after the warm-up is
// nearly every step (about k ln(n / k) rows of n pass). Otherwise, score slot by score slot, the
// passing lanes take buffer slots count + (popcount of the ballot among the lower lanes of the same
// query column): no atomics, and the four lanes advance the count alike. Nothing that passed is ever
// dropped: a step appends at most 32 entries per query, and a query whose count exceeds CAP - 32
// is pruned before the next step.
// Prune (the whole wave, one query): fence, copy the buffer into the wave's LDS scratch (CAP x 8 B)
// padded with (-inf, kNoRow), sort it in the total order with a wave-wide bitonic network (LDS ops
// of one wave complete in order: wave barriers only), write the best k back, count = k, threshold =
// the k-th entry. CAP - 32 >= k, so a prune always has k entries to keep. From then on the threshold
// is the k-th best of rows this wave has seen, so a row that fails it is outside the top-k of the
// wave's rows, hence of the corpus: the scheme is exact. The buffer's order of arrival is irrelevant
// (the sort is total and rows are distinct), so the result is a pure function of the operands.
// A radix select would move fewer bytes per prune; the sort was chosen because the last prune of a
// split needs the list sorted anyway, and one network serves both. The sorts are where the time goes
// at k = 1000 (docs/PERF_NOTES.md has the measurements and what they point at).
// End of split: every wave sorts what it holds once more (K2 entries when that is enough) and writes
// k entries to part [nq, 4 P, k], empty ones as (-inf, kNoRow); every slot is written.
//
// LDS: tile 16 (D + 4) x 4 B (HALF: D + 8) + 4 scratches of 16 K2 B: D = 1024, k = 1024 takes 130 KiB
// (one workgroup per CU); k <= 64 adds 4 KiB to the tile, and three workgroups fit at D = 768. The
// launch form is the same for every k: only the dynamic LDS size changes.
//
// sim_topk_wide_merge_kernel: one workgroup of 4 waves per query. Wave w folds the lists w, w + 4, ...
// into a sorted running list of K2 entries in its own LDS: entry t becomes the better of run[t]
// and list[K2 - 1 - t] (the best K2 of the union, a bitonic sequence), then log2 K2 bitonic merge
// passes sort it again: wave barriers only. After one workgroup barrier wave 0 folds the other
// three running lists in the same way and writes kk = min(k, N) scores and id_base + row.
// sim_topk_merge pops heads k times and is sized for k <= 32 and one list per split.
//
// Rows past the corpus and query slots past nq: clamped for the loads and discarded by select
// (never multiplied by 0, never appended, never written), as in sim_topk.hip.
#include "atpu/common.h"
#include "atpu/kernels.h"
#include "atpu/topk.h"

#include <type_traits>

namespace atpu {
namespace {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

constexpr int kWideWaves = 4;
constexpr int kWideThreads = kWideWaves * kWave;
constexpr int kWideRows = 32;     // corpus rows per wave step: two 16-row MFMA tiles
constexpr int kWideQueries = 16;  // queries per workgroup
constexpr int kWideShare = 4;     // the automatic split count leaves a wave at least kWideShare * K2 rows
constexpr int kNoRow = 0x7fffffff;

inline int wide_k2(int k) {
  int p = 64;
  while (p < k) p <<= 1;
  return p;
}

__device__ __forceinline__ float2 wide_pad() { return float2{-__builtin_inff(), __int_as_float(kNoRow)}; }

__device__ __forceinline__ bool ent_better(float2 a, float2 b) {
  return better(a.x, __float_as_int(a.y), b.x, __float_as_int(b.y));
}

// one wave: its LDS writes before, its LDS reads after (LDS ops of a wave complete in order)
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The passes j = kb / 2 .. 1 of a bitonic network over s[0:M] (M a power of two, kb <= M): blocks of
// kb entries end up sorted, best first where (i & kb) == 0 and best last elsewhere; kb == M sorts
// the whole (bitonic) array best first. One wave; entries that compare equal are identical pads.
__device__ __forceinline__ void wave_bitonic_passes(float2* s, int M, int kb, int lane) {
  constexpr int U = 4;  // pairs per lane in flight: the pairs of a pass are disjoint, so all loads go first
  for (int j = kb >> 1; j > 0; j >>= 1) {
    for (int t0 = lane; t0 < (M >> 1); t0 += U * kWave) {
      int i[U];
      float2 a[U], b[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int t = min(t0 + u * kWave, (M >> 1) - 1);  // M / 2 < 256: a clamped slot repeats a pair, never stored
        i[u] = ((t & ~(j - 1)) << 1) | (t & (j - 1));
        a[u] = s[i[u]];
        b[u] = s[i[u] | j];
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const bool desc = (i[u] & kb) == 0;
        if (t0 + u * kWave < (M >> 1) && ent_better(b[u], a[u]) == desc) {
          s[i[u]] = b[u];
          s[i[u] | j] = a[u];
        }
      }
    }
    wave_lds_sync();
  }
}

__device__ __forceinline__ void wave_bitonic_sort(float2* s, int M, int lane) {
  for (int kb = 2; kb <= M; kb <<= 1) wave_bitonic_passes(s, M, kb, lane);
}

// run[0:K2] sorted best first, list(u) for u in [0, K2) sorted best first: run becomes the best K2 of both
template <typename F>
__device__ __forceinline__ void wave_fold(float2* run, int K2, int lane, F list) {
  for (int t = lane; t < K2; t += kWave) {
    const float2 b = list(K2 - 1 - t), a = run[t];
    if (ent_better(b, a)) run[t] = b;
  }
  wave_lds_sync();
  wave_bitonic_passes(run, K2, K2, lane);
}

// The best `keep` of the n buffer entries gb[0:n] to out[0:keep], sorted (pads past n); returns entry
// keep - 1. M >= max(n, keep) is the power of two that is sorted. One wave; sc is its scratch.
__device__ __forceinline__ float2 wide_prune(float2* gb, float2* sc, int n, int M, int keep, float2* out, int lane) {
  // the appends were stores of other lanes of this wave
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  for (int t = lane; t < M; t += kWave) sc[t] = t < n ? gb[t] : wide_pad();
  wave_lds_sync();
  wave_bitonic_sort(sc, M, lane);
  for (int t = lane; t < keep; t += kWave) out[t] = sc[t];
  return sc[keep - 1];
}

template <bool HALF>
struct WideFrag;
template <>
struct WideFrag<false> {
  f32x4 a[2][4];  // [corpus tile][chunk of 16 columns]
};
template <>
struct WideFrag<true> {
  f16x8 a[2][4];  // [corpus tile][chunk of 32 columns]
};

__device__ __forceinline__ void wide_load(WideFrag<false>& f, const float* __restrict__ c, int D, int N, int row0,
                                          int r, int g, int kb) {
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int row = min(row0 + t * 16 + r, N - 1);  // clamp, the score is discarded by select
    const float* p = c + (size_t)row * D + kb + 4 * g;
#pragma unroll
    for (int ch = 0; ch < 4; ++ch) f.a[t][ch] = *reinterpret_cast<const f32x4*>(p + 16 * ch);
  }
}

__device__ __forceinline__ void wide_load(WideFrag<true>& f, const _Float16* __restrict__ c, int D, int N, int row0,
                                          int r, int g, int kb) {
  const int hi = kb + 128 <= D ? 64 : 0;  // a two-chunk tail step loads its chunks twice
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int row = min(row0 + t * 16 + r, N - 1);
    const _Float16* p = c + (size_t)row * D + kb + 8 * g;
    f.a[t][0] = *reinterpret_cast<const f16x8*>(p);
    f.a[t][1] = *reinterpret_cast<const f16x8*>(p + 32);
    f.a[t][2] = *reinterpret_cast<const f16x8*>(p + hi);
    f.a[t][3] = *reinterpret_cast<const f16x8*>(p + hi + 32);
  }
}

template <bool HALF, bool SC>
__global__ __launch_bounds__(kWideThreads) void sim_topk_wide_kernel(
    const float* __restrict__ q, const typename std::conditional<HALF, _Float16, float>::type* __restrict__ c,
    const float* __restrict__ row_scale, float2* buf, float2* part, int nq, int N, int D, int k, int K2, int P,
    int steps_per_split) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int kStep = HALF ? 128 : 64;  // columns per load step
  constexpr int kPad = HALF ? 8 : 4;      // floats of padding per LDS query row
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 15, g = lane >> 4;
  const int split = blockIdx.x, q0 = blockIdx.y * kWideQueries;
  const int ldq = D + kPad, CAP = 2 * K2;

  // query tile -> LDS (HALF: the permuted image of sim_topk_f16.hip); slots past nq repeat the last query
  const int c4 = D >> 2;
  for (int i = tid; i < kWideQueries * c4; i += kWideThreads) {
    const int qi = i / c4, cc = i - qi * c4;
    const int qr = min(q0 + qi, nq - 1);
    const int u = cc & 7, pc = HALF ? (cc & ~7) + 4 * (u & 1) + (u >> 1) : cc;
    *reinterpret_cast<f32x4*>(smem + qi * ldq + pc * 4) = *reinterpret_cast<const f32x4*>(q + (size_t)qr * D + cc * 4);
  }
  __syncthreads();

  float2* sc = reinterpret_cast<float2*>(smem + kWideQueries * ldq) + wave * CAP;  // this wave's sort scratch
  float2* wbuf = buf + (((size_t)blockIdx.y * P + split) * kWideWaves + wave) * kWideQueries * CAP;
  float2* qbuf = wbuf + (size_t)r * CAP;  // the buffer of this lane's query
  const bool qlive = q0 + r < nq;
  const unsigned long long col = 0x0001000100010001ull << r;  // the 4 lanes of this lane's query
  const unsigned long long below = col & ((1ull << lane) - 1);
  float thr_v = -__builtin_inff();
  int thr_i = kNoRow, cnt = 0;

  const int nsteps = (N + kWideRows - 1) / kWideRows;
  const int s_lo = split * steps_per_split, s_hi = min(s_lo + steps_per_split, nsteps);
  const int KS = (D + kStep - 1) / kStep;
  const float* qb = smem + r * ldq + 4 * g;

  // The wave's (rows, columns) steps form one stream, as in sim_topk.hip: the loads of step i + 1 are
  // issued before the MFMAs of step i; rows past this wave's last are clamped into c[0:N].
  WideFrag<HALF> f0, f1;
  int s = s_lo + wave, ks = 0;
  f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
  if (s < s_hi) wide_load(f0, c, D, N, s * kWideRows, r, g, 0);
  auto stage = [&](const WideFrag<HALF>& cur, WideFrag<HALF>& nxt) {
    const bool last = ks + 1 == KS;
    const int ns = last ? s + kWideWaves : s, nks = last ? 0 : ks + 1;
    const int kb = ks * kStep;
    float rs[2][4] = {};
    if constexpr (SC) {
      if (last) {  // wave-uniform; issued before the corpus loads, so the wait for them leaves those in flight
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int e = 0; e < 4; ++e) rs[t][e] = row_scale[min(s * kWideRows + t * 16 + g * 4 + e, N - 1)];
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    wide_load(nxt, c, D, N, ns * kWideRows, r, g, nks * kStep);
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (HALF) {
      auto chunk = [&](int cp) {
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
          const f32x4 b = *reinterpret_cast<const f32x4*>(qb + kb + 32 * cp + 16 * hf);
          float a[2][4];  // converted just in time
#pragma unroll
          for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int j = 0; j < 4; ++j) a[t][j] = (float)cur.a[t][cp][4 * hf + j];
#pragma unroll
          for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int t = 0; t < 2; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t][j], b[j], acc[t], 0, 0, 0);
        }
      };
      chunk(0);
      chunk(1);
      if (kb + kStep <= D) {
        chunk(2);
        chunk(3);
      }
    } else {
#pragma unroll
      for (int ch = 0; ch < 4; ++ch) {
        const f32x4 b = *reinterpret_cast<const f32x4*>(qb + kb + 16 * ch);
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int t = 0; t < 2; ++t)
            acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(cur.a[t][ch][j], b[j], acc[t], 0, 0, 0);
      }
    }
    if (last) {  // the rows' scores are complete: against the threshold, the passing ones into the buffer
      float v[8];
      int id[8];
      bool pass[8], any = false;
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int row = s * kWideRows + t * 16 + g * 4 + e;
          const bool live = row < N;
          float sv = acc[t][e];
          if constexpr (SC) sv *= rs[t][e];
          v[t * 4 + e] = live ? sv : -__builtin_inff();
          id[t * 4 + e] = live ? row : kNoRow;
          pass[t * 4 + e] = qlive && better(v[t * 4 + e], id[t * 4 + e], thr_v, thr_i);  // false for (-inf, kNoRow)
          any |= pass[t * 4 + e];
        }
      acc[0] = f32x4{0.f, 0.f, 0.f, 0.f};
      acc[1] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (__ballot(any) != 0) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const unsigned long long m = __ballot(pass[e]);
          if (pass[e]) qbuf[cnt + __popcll(m & below)] = float2{v[e], __int_as_float(id[e])};
          cnt += __popcll(m & col);  // at most 4 per slot, 32 per step: cnt <= CAP
        }
        unsigned long long full = __ballot(cnt > CAP - 32) & 0xffffull;  // lanes 0 .. 15: one per query
        while (full) {
          const int qx = __builtin_amdgcn_readfirstlane(__ffsll((long long)full) - 1);
          full &= full - 1;
          const int n = __builtin_amdgcn_readlane(cnt, qx);
          float2* gb = wbuf + (size_t)qx * CAP;
          const float2 kth = wide_prune(gb, sc, n, CAP, k, gb, lane);
          if (r == qx) {
            cnt = k;
            thr_v = kth.x;
            thr_i = __float_as_int(kth.y);
          }
        }
      }
    }
    s = ns;
    ks = nks;
  };
  while (s < s_hi) {
    stage(f0, f1);
    if (s < s_hi) stage(f1, f0);
  }

  // end of split: this wave's sorted best k of every live query -> part [nq, 4 P, k]
  for (int qx = 0; qx < kWideQueries && q0 + qx < nq; ++qx) {
    const int n = __builtin_amdgcn_readlane(cnt, qx);
    float2* out = part + (((size_t)(q0 + qx) * P + split) * kWideWaves + wave) * k;
    if (n == 0) {
      for (int t = lane; t < k; t += kWave) out[t] = wide_pad();
    } else {
      wide_prune(wbuf + (size_t)qx * CAP, sc, n, n <= K2 ? K2 : CAP, k, out, lane);
    }
  }
}

__global__ __launch_bounds__(kWideThreads) void sim_topk_wide_merge_kernel(const float2* __restrict__ part,
                                                                            float* __restrict__ scores,
                                                                            int64_t* __restrict__ ids, int L, int k,
                                                                            int K2, int kk, int64_t id_base) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int qi = blockIdx.x;
  float2* run = reinterpret_cast<float2*>(smem) + wave * K2;
  const float2* src = part + (size_t)qi * L * k;
  for (int t = lane; t < K2; t += kWave) run[t] = (wave < L && t < k) ? src[(size_t)wave * k + t] : wide_pad();
  wave_lds_sync();
  for (int l = wave + kWideWaves; l < L; l += kWideWaves) {
    const float2* lp = src + (size_t)l * k;
    wave_fold(run, K2, lane, [&](int u) { return u < k ? lp[u] : wide_pad(); });
  }
  __syncthreads();
  if (wave != 0) return;
  for (int w = 1; w < kWideWaves; ++w) {
    const float2* other = run + w * K2;
    wave_fold(run, K2, lane, [&](int u) { return other[u]; });
  }
  for (int t = lane; t < kk; t += kWave) {
    const float2 e = run[t];
    scores[(size_t)qi * kk + t] = e.x;
    ids[(size_t)qi * kk + t] = id_base + __float_as_int(e.y);
  }
}

size_t wide_lds_bytes(int D, int K2, bool half) {
  return (size_t)kWideQueries * (D + (half ? 8 : 4)) * sizeof(float) + (size_t)kWideWaves * 2 * K2 * sizeof(float2);
}

// bytes of workspace per split: the candidate buffers and the partial lists
int64_t wide_split_bytes(int k, int nq) {
  const int64_t tiles = (nq + kWideQueries - 1) / kWideQueries;
  return (tiles * kWideWaves * kWideQueries * 2 * wide_k2(k) + (int64_t)nq * kWideWaves * k) * (int64_t)sizeof(float2);
}

template <bool HALF, bool SC>
void wide_launch(const float* q, const void* c, const float* row_scale, float2* buf, float2* part, int nq, int N,
                 int D, int k, int P, hipStream_t stream) {
  using T = typename std::conditional<HALF, _Float16, float>::type;
  const int K2 = wide_k2(k);
  const int nsteps = (N + kWideRows - 1) / kWideRows;
  const int sps = (nsteps + P - 1) / P;
  const size_t lds = wide_lds_bytes(D, K2, HALF);
  // up to 130 KiB of dynamic LDS (D = 1024, k = 1024); the attribute is per device and needed above 64 KiB only
  if (lds > 64 * 1024)
    ATPU_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&sim_topk_wide_kernel<HALF, SC>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL((sim_topk_wide_kernel<HALF, SC>), dim3(P, (nq + kWideQueries - 1) / kWideQueries),
                     dim3(kWideThreads), lds, stream, q, static_cast<const T*>(c), row_scale, buf, part, nq, N, D, k, K2,
                     P, sps);
  ATPU_HIP_CHECK(hipGetLastError());
}

void wide_check(const float* q, const void* c, const float* buf, const float* part, int nq, int N, int D, int k,
                int P) {
  ATPU_CHECK(nq >= 1 && N >= 1, "sim_topk_wide: nq and N must be >= 1");
  ATPU_CHECK(D % 64 == 0 && D >= 64 && D <= 1024, "sim_topk_wide: D must be a multiple of 64 in [64, 1024]");
  ATPU_CHECK(k >= 1 && k <= kSimWideMaxK, "sim_topk_wide: k must be in [1, 1024]");
  ATPU_CHECK(P >= 1 && P == sim_topk_wide_splits(N, k, nq, P), "sim_topk_wide: P must come from sim_topk_wide_splits");
  ATPU_CHECK(q && c && buf && part, "sim_topk_wide: null tensor");
  ATPU_CHECK(((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(c)) & 15) == 0 &&
                 ((reinterpret_cast<uintptr_t>(buf) | reinterpret_cast<uintptr_t>(part)) & 7) == 0,
             "sim_topk_wide: q and c must be 16-byte and the workspaces 8-byte aligned");
}

}  // namespace

// The rule. A split count the caller names (want >= 1; tests and benches) is kept up to the hard
// limits: no empty split, at most kSimMaxSplits, and buffers plus partial lists of at most
// kSimWideWsBytes (one split always runs, whatever it takes). want <= 0 asks for the automatic count:
// as many splits as leave every wave at least kWideShare * K2 rows, K2 the power of two >= max(k, 64).
// With fewer rows a wave's threshold never rises far above its warm-up and the wave merely sorts
// its whole share; with more, appends become rare (about k ln(rows / k) of them) while every
// further split adds 4 lists of k entries per query to the merge. The factor kWideShare = 4 was reasoned,
// not measured against other values: it trades workgroups for fewer sorts, and at N = 65536, k = 1000 it
// leaves 4 workgroups per 16-query tile on a 256-CU device, the slowest points measured.
// The bound only lowers the split count: one split of nq queries takes wide_split_bytes(k, nq), which
// grows with nq without limit. The caller keeps it by cutting the query batch (ops.sim_topk_wide does;
// a query's result does not depend on its batch).
int sim_topk_wide_splits(int N, int k, int nq, int want) {
  const int nsteps = (N + kWideRows - 1) / kWideRows;
  int64_t p = want >= 1 ? want : N / (kWideWaves * kWideShare * wide_k2(k));
  const int64_t fit = kSimWideWsBytes / wide_split_bytes(k, nq);
  p = p < fit ? p : fit;
  p = p < 1 ? 1 : (p > kSimMaxSplits ? kSimMaxSplits : p);
  const int sps = (nsteps + (int)p - 1) / (int)p;
  return (nsteps + sps - 1) / sps;  // no empty split
}

void sim_topk_wide_partial(const float* q, const float* c, float* buf, float* part, int nq, int N, int D, int k,
                           int P, hipStream_t stream) {
  wide_check(q, c, buf, part, nq, N, D, k, P);
  wide_launch<false, false>(q, c, nullptr, reinterpret_cast<float2*>(buf), reinterpret_cast<float2*>(part), nq, N, D,
                            k, P, stream);
}

void sim_topk_wide_partial_f16(const float* q, const _Float16* c, const float* row_scale, float* buf, float* part,
                               int nq, int N, int D, int k, int P, hipStream_t stream) {
  wide_check(q, c, buf, part, nq, N, D, k, P);
  ATPU_CHECK((reinterpret_cast<uintptr_t>(row_scale) & 3) == 0, "sim_topk_wide: row_scale must be 4-byte aligned");
  float2* b = reinterpret_cast<float2*>(buf);
  float2* p = reinterpret_cast<float2*>(part);
  if (row_scale) wide_launch<true, true>(q, c, row_scale, b, p, nq, N, D, k, P, stream);
  else wide_launch<true, false>(q, c, nullptr, b, p, nq, N, D, k, P, stream);
}

void sim_topk_wide_merge(const float* part, float* scores, int64_t* ids, int nq, int P, int k, int kk,
                         int64_t id_base, hipStream_t stream) {
  ATPU_CHECK(nq >= 1 && P >= 1 && P <= kSimMaxSplits, "sim_topk_wide_merge: P must be in [1, 256]");
  ATPU_CHECK(k >= 1 && k <= kSimWideMaxK && kk >= 1 && kk <= k, "sim_topk_wide_merge: 1 <= kk <= k <= 1024");
  ATPU_CHECK(part && scores && ids, "sim_topk_wide_merge: null tensor");
  const int K2 = wide_k2(k);
  hipLaunchKernelGGL(sim_topk_wide_merge_kernel, dim3(nq), dim3(kWideThreads),
                     (size_t)kWideWaves * K2 * sizeof(float2), stream, reinterpret_cast<const float2*>(part), scores,
                     ids, P * kWideWaves, k, K2, kk, id_base);
  ATPU_HIP_CHECK(hipGetLastError());
}

}  // namespace atpu
