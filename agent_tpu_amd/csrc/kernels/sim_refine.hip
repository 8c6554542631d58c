// refine_topk: exact re-scoring of a per-query shortlist. Every query brings its own R candidate rows
// (int32 ids into a store c [N, D] of fp32 or fp16 rows, which may be pinned host memory read through
// its device-visible address); the kernel gathers them, scores them with sim_topk's bits and keeps the
// top-k in the total order (value desc, row asc: better() of atpu/topk.h). The only intermediate in
// global memory is the workspace [nq, P, k] of per-chunk lists that sim_topk_merge reduces.
//
// Bits. A (query, row) score is one fp32 accumulator of v_mfma_f32_16x16x4_f32 fed in the k order of
// sim_topk.hip (fp32 store: chunks of 16 columns, lane (r, g) holds c[row r][16 ch + 4 g .. + 3], MFMA j
// takes element j) or of sim_topk_f16.hip (fp16 store: chunks of 32 columns, lane (r, g) holds
// c[row r][32 cp + 8 g .. + 7] widened just before use, MFMA j takes element j, j = 0 .. 7; the query
// image in LDS permuted as in that file), times row_scale[row] once before the ranking when one is
// given. Every output element of the MFMA is an independent chain along k, so it does not matter which
// rows share a tile: a candidate's score is the score sim_topk gives the same (query, row).
//
// Work split: refine_kernel<T, KM, SC>, one workgroup of 4 waves per (query, chunk of its candidates).
// Rows are scattered and differ per query, so there is no corpus tile to share: the query sits once in
// LDS (D floats) and fills all 16 columns of the B operand by broadcast reads; one column's worth of
// the MFMA is useful work. That waste is accepted: the kernel waits for gathered rows, not for the
// matrix unit. A wave step is 32 candidates (two 16-row A tiles): lane (r, g) reads 16 bytes of row r,
// a row's bytes of one step are contiguous (256 B), and a step is 8 x 16 B in flight per lane. The
// wave's (candidates, columns) steps form one stream, as in sim_topk.hip: the loads of step i + 1 (the
// next columns, or the first columns of the wave's next 32 candidates) are issued before the MFMAs of
// step i. Over a host link one step ahead hides little of the latency; the rest comes from occupancy
// (the workgroup needs D * 4 + 1 KiB of LDS, so the registers decide how many share a CU) and from the
// grid (refine_chunks: small chunks, many workgroups).
//
// Candidate ids: lane r of tile t holds the id of slot 16 t + r. An id outside [0, N) (an empty slot
// carries kNoRow) is never dereferenced: its lane reads the row of the tile's first valid id instead
// (no extra lines), or row 0 when the tile has none, and its score is discarded by select. The ids of
// the wave's next step are loaded one step early, after the step's row loads.
//
// Selection: after a step's last columns lane (r, g), r < 8, owns one of the wave's 32 scores (tile
// (r >> 2) & 1, row 4 g + (r & 3)) and keeps a sorted register list of KM >= k entries (list_insert
// behind a wave ballot). At the end the 64 lists of a wave are reduced in registers (k rounds of best
// head), the 4 wave lists meet in LDS, and 4 lanes pop the best head k times into ws[query][chunk].
// The live ids of one query must be distinct (a shortlist of disjoint segments is): a head has one owner.
#include "atpu/common.h"
#include "atpu/kernels.h"
#include "atpu/topk.h"

namespace atpu {
namespace {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

constexpr int kRefWaves = 4;
constexpr int kRefThreads = kRefWaves * kWave;
constexpr int kRefRows = 32;  // candidates per wave step: two 16-row MFMA tiles
constexpr int kNoRow = 0x7fffffff;

template <typename T>
struct RefStore;
template <>
struct RefStore<float> {
  typedef f32x4 Vec;
  static constexpr int kLane = 4, kChunk = 16, kStep = 64;  // elements per 16 B, columns per chunk and per step
};
template <>
struct RefStore<_Float16> {
  typedef f16x8 Vec;
  static constexpr int kLane = 8, kChunk = 32, kStep = 128;
};

template <typename T>
struct RefFrag {
  typename RefStore<T>::Vec a[2][4];  // [tile][chunk]
};

// the four chunks of columns kb .. of the two tiles' rows; a two-chunk tail step (fp16, D an odd
// multiple of 64) loads its chunks twice, as sim_topk_f16.hip
template <typename T>
__device__ __forceinline__ void ref_load(RefFrag<T>& f, const T* __restrict__ c, int D, const int (&row)[2], int g,
                                         int kb) {
  typedef typename RefStore<T>::Vec V;
  constexpr int CH = RefStore<T>::kChunk;
  const int hi = kb + RefStore<T>::kStep <= D ? 2 * CH : 0;
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const T* p = c + (size_t)row[t] * D + kb + RefStore<T>::kLane * g;
    f.a[t][0] = *reinterpret_cast<const V*>(p);
    f.a[t][1] = *reinterpret_cast<const V*>(p + CH);
    f.a[t][2] = *reinterpret_cast<const V*>(p + hi);
    f.a[t][3] = *reinterpret_cast<const V*>(p + hi + CH);
  }
}

// one chunk of both tiles into the accumulators; qk = the query image at this chunk for lane group g
__device__ __forceinline__ void ref_chunk(f32x4 (&acc)[2], const RefFrag<float>& cur, int ch, const float* qk) {
  const f32x4 b = *reinterpret_cast<const f32x4*>(qk);
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int t = 0; t < 2; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(cur.a[t][ch][j], b[j], acc[t], 0, 0, 0);
}

__device__ __forceinline__ void ref_chunk(f32x4 (&acc)[2], const RefFrag<_Float16>& cur, int cp, const float* qk) {
#pragma unroll
  for (int hf = 0; hf < 2; ++hf) {
    const f32x4 b = *reinterpret_cast<const f32x4*>(qk + 16 * hf);
    float a[2][4];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int j = 0; j < 4; ++j) a[t][j] = (float)cur.a[t][cp][4 * hf + j];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int t = 0; t < 2; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t][j], b[j], acc[t], 0, 0, 0);
  }
}

template <typename T, int KM, bool SC>
__global__ __launch_bounds__(kRefThreads) void refine_kernel(const float* __restrict__ q, const T* __restrict__ c,
                                                             const float* __restrict__ row_scale,
                                                             const int32_t* __restrict__ cand, int cand_stride,
                                                             float2* __restrict__ ws, int N, int D, int R, int k, int P,
                                                             int steps_per_chunk) {
  extern __shared__ __attribute__((aligned(16))) float smem[];  // the query image [D], then the wave lists
  constexpr bool kHalf = sizeof(T) == 2;
  constexpr int ST = RefStore<T>::kStep, CH = RefStore<T>::kChunk;
  float2* wl = reinterpret_cast<float2*>(smem + D);  // [kRefWaves][KM]
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 15, g = lane >> 4;
  const int qi = blockIdx.x / P, chunk = blockIdx.x - qi * P;
  const int32_t* cq = cand + (size_t)qi * R * cand_stride;

  // query -> LDS; for an fp16 store in sim_topk_f16.hip's permuted image (inside every 32 columns the
  // 16-byte piece 2 g + hf sits at piece 4 hf + g)
  for (int cc = tid; cc < (D >> 2); cc += kRefThreads) {
    int pc = cc;
    if constexpr (kHalf) {
      const int u = cc & 7;
      pc = (cc & ~7) + 4 * (u & 1) + (u >> 1);
    }
    *reinterpret_cast<f32x4*>(smem + pc * 4) = *reinterpret_cast<const f32x4*>(q + (size_t)qi * D + cc * 4);
  }
  __syncthreads();

  float tv[KM];
  int ti[KM];
#pragma unroll
  for (int e = 0; e < KM; ++e) {
    tv[e] = -__builtin_inff();
    ti[e] = kNoRow;
  }

  const int nsteps = R / kRefRows;
  const int s_lo = chunk * steps_per_chunk, s_hi = min(s_lo + steps_per_chunk, nsteps);  // s_lo < s_hi
  const int KS = (D + ST - 1) / ST;
  const float* qb = smem + 4 * g;

  // ids of the two tiles of a step (clamped to the chunk's last step: slots below R)
  auto load_ids = [&](int (&ids)[2], int step) {
    const int base = min(step, s_hi - 1) * kRefRows + r;
#pragma unroll
    for (int t = 0; t < 2; ++t) ids[t] = cq[(size_t)(base + 16 * t) * cand_stride];
  };
  // the rows to read: an id outside [0, N) reads the tile's first valid row, or row 0
  auto clamp_rows = [&](const int (&ids)[2], int (&rows)[2]) {
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const bool ok = (unsigned)ids[t] < (unsigned)N;
      const unsigned long long m = __ballot(ok);
      const int first = m ? __ffsll(m) - 1 : 0;  // a lane below 16: all four lane groups hold the same ids
      const int fid = __builtin_amdgcn_readlane(ids[t], first);
      rows[t] = ok ? ids[t] : (m ? fid : 0);
    }
  };
  // the id of the score this lane owns after a step: slot 16 t + 4 g + e, t = (r >> 2) & 1, e = r & 3
  auto own_id = [&](const int (&ids)[2]) {
    const int src = (4 * g + (r & 3)) * 4;
    const int a = __builtin_amdgcn_ds_bpermute(src, ids[0]), b = __builtin_amdgcn_ds_bpermute(src, ids[1]);
    return (r & 4) ? b : a;
  };

  RefFrag<T> f0, f1;
  int s = s_lo + wave, ks = 0;
  int row[2] = {0, 0}, nids[2] = {kNoRow, kNoRow}, myid = kNoRow;
  f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
  if (s < s_hi) {
    int ids[2];
    load_ids(ids, s);
    clamp_rows(ids, row);
    myid = own_id(ids);
    ref_load(f0, c, D, row, g, 0);
    load_ids(nids, s + kRefWaves);
  }
  auto stage = [&](const RefFrag<T>& cur, RefFrag<T>& nxt) {
    const bool last = ks + 1 == KS;
    const int ns = last ? s + kRefWaves : s, nks = last ? 0 : ks + 1;
    const int kb = ks * ST;
    int ids[2] = {nids[0], nids[1]}, nrow[2] = {row[0], row[1]};
    if (last) clamp_rows(ids, nrow);  // a step past the chunk repeats its last step's rows: inside c
    float rs = 1.f;
    if constexpr (SC) {
      rs = row_scale[(unsigned)myid < (unsigned)N ? myid : 0];
      __builtin_amdgcn_sched_barrier(0);
    }
    ref_load(nxt, c, D, nrow, g, nks * ST);
    load_ids(nids, ns + kRefWaves);  // every step, the same ids until s moves: no load under a branch
    __builtin_amdgcn_sched_barrier(0);
    ref_chunk(acc, cur, 0, qb + kb);
    ref_chunk(acc, cur, 1, qb + kb + CH);
    if (kb + ST <= D) {
      ref_chunk(acc, cur, 2, qb + kb + 2 * CH);
      ref_chunk(acc, cur, 3, qb + kb + 3 * CH);
    }
    if (last) {  // the candidates' scores are complete: scaled, then one per lane into the lists
      const f32x4 x = (r & 4) ? acc[1] : acc[0];
      const int e = r & 3;
      float sv = e == 0 ? x[0] : (e == 1 ? x[1] : (e == 2 ? x[2] : x[3]));
      if constexpr (SC) sv *= rs;
      const bool live = r < 8 && (unsigned)myid < (unsigned)N;
      const float v = live ? sv : -__builtin_inff();
      const int id = live ? myid : kNoRow;
      if (__ballot(better(v, id, tv[KM - 1], ti[KM - 1])) != 0) list_insert<KM>(tv, ti, v, id);
      acc[0] = acc[1] = f32x4{0.f, 0.f, 0.f, 0.f};
      row[0] = nrow[0];
      row[1] = nrow[1];
      myid = own_id(ids);
    }
    s = ns;
    ks = nks;
  };
  while (s < s_hi) {
    stage(f0, f1);
    if (s < s_hi) stage(f1, f0);
  }

  // the wave's 64 lists -> its sorted top-k in lanes 0 .. k - 1: k rounds of best head, the owner pops
  float rv = -__builtin_inff();
  int ri = kNoRow;
  for (int n = 0; n < k; ++n) {
    float bv = tv[0];
    int bi = ti[0];
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
    if (lane == n) {
      rv = bv;
      ri = bi;
    }
    if (ti[0] == bi && bi != kNoRow) {  // ids are distinct: exactly one owner
#pragma unroll
      for (int x = 0; x + 1 < KM; ++x) {
        tv[x] = tv[x + 1];
        ti[x] = ti[x + 1];
      }
      tv[KM - 1] = -__builtin_inff();
      ti[KM - 1] = kNoRow;
    }
  }
  if (lane < KM) wl[wave * KM + lane] = float2{rv, __int_as_float(ri)};
  __syncthreads();
  if (wave == 0) {  // 4 lanes, one wave list each
    const float2* mine = wl + (lane & (kRefWaves - 1)) * KM;
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
      step(dppf<kDppXor2>(bv), dppi<kDppXor2>(bi));
      step(dppf<kDppXor1>(bv), dppi<kDppXor1>(bi));
      if (hi == bi && bi != kNoRow) ++pos;
      if (lane == 0) ws[((size_t)qi * P + chunk) * k + n] = float2{bv, __int_as_float(bi)};
    }
  }
}

template <typename T, int KM, bool SC>
void refine_launch(const float* q, const T* c, const float* row_scale, const int32_t* cand, int cand_stride, float2* ws,
                   int nq, int N, int D, int R, int k, int P, int spc, hipStream_t stream) {
  const size_t lds = (size_t)D * sizeof(float) + (size_t)kRefWaves * KM * sizeof(float2);  // at most 5 KiB
  hipLaunchKernelGGL((refine_kernel<T, KM, SC>), dim3((unsigned)((int64_t)nq * P)), dim3(kRefThreads), lds, stream, q, c,
                     row_scale, cand, cand_stride, ws, N, D, R, k, P, spc);
  ATPU_HIP_CHECK(hipGetLastError());
}

template <typename T>
void refine_dispatch(const float* q, const T* c, const float* row_scale, const int32_t* cand, int cand_stride,
                     float2* ws, int nq, int N, int D, int R, int k, int P, int spc, hipStream_t stream) {
#define ATPU_REFINE_CASE(KM)                                                                                      \
  do {                                                                                                            \
    if (row_scale) refine_launch<T, KM, true>(q, c, row_scale, cand, cand_stride, ws, nq, N, D, R, k, P, spc, stream); \
    else refine_launch<T, KM, false>(q, c, nullptr, cand, cand_stride, ws, nq, N, D, R, k, P, spc, stream);       \
  } while (0)
  if (k <= 8) ATPU_REFINE_CASE(8);
  else if (k <= 16) ATPU_REFINE_CASE(16);
  else ATPU_REFINE_CASE(32);
#undef ATPU_REFINE_CASE
}

}  // namespace

int refine_chunks(int R, int want) {
  const int nsteps = R / kRefRows;
  const int p = want < 1 ? 1 : (want > kSimMaxSplits ? kSimMaxSplits : want);
  const int spc = (nsteps + p - 1) / p;
  return (nsteps + spc - 1) / spc;  // no empty chunk
}

void refine_topk_partial(const float* q, const void* store, bool half, const float* row_scale, const int32_t* cand,
                         int cand_stride, float* ws, int nq, int N, int D, int R, int k, int P, hipStream_t stream) {
  ATPU_CHECK(nq >= 1 && N >= 1 && N <= 2147483647 - 256, "refine_topk: nq >= 1 and N in [1, 2^31 - 256]");
  ATPU_CHECK(D % 64 == 0 && D >= 64 && D <= 1024, "refine_topk: D must be a multiple of 64 in [64, 1024]");
  ATPU_CHECK(k >= 1 && k <= 32, "refine_topk: k must be in [1, 32]");
  ATPU_CHECK(R % kRefRows == 0 && R >= kRefRows && R <= kRefRows * kSimMaxSplits,
             "refine_topk: R must be a multiple of 32 in [32, 8192]");
  ATPU_CHECK(cand_stride >= 1 && cand_stride <= 2, "refine_topk: the candidate stride must be 1 or 2");
  ATPU_CHECK(P >= 1 && P == refine_chunks(R, P), "refine_topk: P must come from refine_chunks");
  ATPU_CHECK((int64_t)nq * P <= 2147483647LL, "refine_topk: too many workgroups");
  ATPU_CHECK(q && store && cand && ws, "refine_topk: null tensor");
  ATPU_CHECK(half || !row_scale, "refine_topk: row_scale goes with an fp16 store");
  ATPU_CHECK(((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(store)) & 15) == 0 &&
                 (reinterpret_cast<uintptr_t>(ws) & 7) == 0 &&
                 ((reinterpret_cast<uintptr_t>(cand) | reinterpret_cast<uintptr_t>(row_scale)) & 3) == 0,
             "refine_topk: q and the store must be 16-byte, the workspace 8-byte, the ids and row_scale 4-byte aligned");
  const int nsteps = R / kRefRows;
  const int spc = (nsteps + P - 1) / P;
  float2* w = reinterpret_cast<float2*>(ws);
  if (half)
    refine_dispatch<_Float16>(q, static_cast<const _Float16*>(store), row_scale, cand, cand_stride, w, nq, N, D, R, k, P,
                              spc, stream);
  else
    refine_dispatch<float>(q, static_cast<const float*>(store), nullptr, cand, cand_stride, w, nq, N, D, R, k, P, spc,
                           stream);
}

}  // namespace atpu
