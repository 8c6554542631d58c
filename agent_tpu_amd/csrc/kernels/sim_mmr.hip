// mmr_select: maximal-marginal-relevance selection over a query's candidate rows, fused with the Gram matrix it
// needs. Every query brings R <= 32 candidates (int32 ids into a store c [N, D] of fp32 or fp16 rows, device or
// pinned host memory, in the order sim_topk returned them) and their relevance scores; the kernel forms
// G = C C^T over the candidates and picks k of them greedily,
//
//   v_l = rel_l * lam                         while nothing is picked
//   v_l = rel_l * lam - mu * pen_l            afterwards, pen_l = max over the picks j of G[l][j]
//
// three separately rounded fp32 operations (no contraction; the running max is exact), the arg-max of (v, id)
// under better() of atpu/topk.h: a total order, so every pick is unique. Neither G nor a row leaves the GPU.
//
// Work split: one workgroup of 4 waves per query, wave w owns the 16 x 16 tile (w >> 1, w & 1) of G. Both MFMA
// operands come straight from global memory into registers: for v_mfma_f32_16x16x4_f32 the A and the B operand
// have the same lane map (lane (r, g) holds 16 bytes of row r), so one load routine (sim_refine.hip's) serves both
// sides and no operand passes through LDS; a diagonal tile loads its rows once. Loads run one 64-column (fp32) or
// 128-column (fp16) step ahead of the MFMAs, in two fragment buffers that take turns. With R == 16 only wave 0 has
// a tile; the others wait at the barrier.
//
// Bits. Every G[i][j] is ONE fp32 accumulator over the whole of D (no split over D, no cross-wave sum), fed in the
// column order of sim_topk.hip (fp32 store: chunks of 16 columns, lane (r, g) holds c[row r][16 ch + 4 g .. + 3],
// MFMA j takes element j) or of sim_topk_f16.hip (fp16 store: chunks of 32 columns, lane (r, g) holds
// c[row r][32 cp + 8 g .. + 7] widened just before use, MFMA j takes element j, j = 0 .. 7). So
//   - G[i][j] has the bits sim_topk gives the query store[i] against row j;
//   - G[i][j] and G[j][i] are bit-equal: the products commute and the chain order is the same;
//   - computing tile (1, 0) as well as (0, 1) therefore costs no transpose.
// With row_scale (fp16 store): G[i][j] = g * (s_i * s_j), the product of the two scales rounded first (symmetric),
// then one more rounding.
//
// Candidate ids: an id outside [0, N) (a padded slot carries kNoRow) is never dereferenced: its lane reads the
// tile's first valid row instead, or row 0, and the slot is dead in the selection by select.
//
// Selection: the tiles meet in LDS as G [32][33] fp32 (the kernel's only LDS). Wave 0, lane l < R owns candidate
// l. Each of the k rounds takes the wave arg-max by the DPP butterfly; the winner goes to out_ids / out_rel /
// out_mmr [q][t], its lane is retired with (v, id) = (-inf, kNoRow), and every live lane folds G[l][winner] into
// pen_l. Empty and picked slots never win; when the live candidates run out the remaining entries are
// (-inf, id_base + kNoRow). The live ids of one query must be distinct (a top-k list is).
//
// rows_gather: out[i] = store[ids[i] - id_base] (and out_scale[i] = row_scale[..]) in the store's dtype, one wave per
// row, 16-byte loads and stores; an id outside the store writes zeros and scale 1.
#include "atpu/common.h"
#include "atpu/kernels.h"
#include "atpu/topk.h"

namespace atpu {
namespace {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

constexpr int kMmrWaves = 4;
constexpr int kMmrThreads = kMmrWaves * kWave;
constexpr int kMmrSlots = 32;          // candidates per query at most: a 2 x 2 grid of MFMA tiles
constexpr int kMmrLd = kMmrSlots + 1;  // G's row stride in LDS: a column read touches 32 banks
constexpr int kNoRow = 0x7fffffff;

template <typename T>
struct MmrStore;
template <>
struct MmrStore<float> {
  typedef f32x4 Vec;
  static constexpr int kLane = 4, kChunk = 16, kStep = 64;  // elements per 16 B, columns per chunk and per step
};
template <>
struct MmrStore<_Float16> {
  typedef f16x8 Vec;
  static constexpr int kLane = 8, kChunk = 32, kStep = 128;
};

template <typename T, bool DIAG>
struct MmrFrag {
  typename MmrStore<T>::Vec a[4], b[DIAG ? 1 : 4];  // [chunk]; a diagonal tile's B operand is its A operand
};

// the four chunks of columns kb .. of one row; a two-chunk tail step (fp16, D an odd multiple of 64) loads its
// chunks twice, as sim_topk_f16.hip
template <typename T>
__device__ __forceinline__ void mmr_load_row(typename MmrStore<T>::Vec (&v)[4], const T* __restrict__ c, int D, int row,
                                             int g, int kb) {
  typedef typename MmrStore<T>::Vec V;
  constexpr int CH = MmrStore<T>::kChunk;
  const int hi = kb + MmrStore<T>::kStep <= D ? 2 * CH : 0;
  const T* p = c + (size_t)row * D + kb + MmrStore<T>::kLane * g;
  v[0] = *reinterpret_cast<const V*>(p);
  v[1] = *reinterpret_cast<const V*>(p + CH);
  v[2] = *reinterpret_cast<const V*>(p + hi);
  v[3] = *reinterpret_cast<const V*>(p + hi + CH);
}

template <typename T, bool DIAG>
__device__ __forceinline__ void mmr_load(MmrFrag<T, DIAG>& f, const T* __restrict__ c, int D, int row_a, int row_b,
                                         int g, int kb) {
  mmr_load_row<T>(f.a, c, D, row_a, g, kb);
  if constexpr (!DIAG) mmr_load_row<T>(f.b, c, D, row_b, g, kb);
}

// one chunk into the accumulator
__device__ __forceinline__ void mmr_chunk(f32x4& acc, f32x4 a, f32x4 b) {
#pragma unroll
  for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], b[j], acc, 0, 0, 0);
}

__device__ __forceinline__ void mmr_chunk(f32x4& acc, f16x8 a, f16x8 b) {
#pragma unroll
  for (int j = 0; j < 8; ++j) acc = __builtin_amdgcn_mfma_f32_16x16x4f32((float)a[j], (float)b[j], acc, 0, 0, 0);
}

// the 16 x 16 tile (rows row_a of the lanes' r, columns row_b of the lanes' r): lane (r, g) gets
// G[4 g + e][r], e = 0 .. 3
template <typename T, bool DIAG>
__device__ __forceinline__ f32x4 mmr_tile(const T* __restrict__ c, int D, int row_a, int row_b, int g) {
  constexpr int ST = MmrStore<T>::kStep;
  const int KS = (D + ST - 1) / ST;
  MmrFrag<T, DIAG> f0, f1;
  f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
  mmr_load<T, DIAG>(f0, c, D, row_a, row_b, g, 0);
  int ks = 0;
  auto stage = [&](const MmrFrag<T, DIAG>& cur, MmrFrag<T, DIAG>& nxt) {
    const int kb = ks * ST;
    if (ks + 1 < KS) mmr_load<T, DIAG>(nxt, c, D, row_a, row_b, g, kb + ST);  // wave-uniform: nothing past D is read
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int ch = 0; ch < 4; ++ch)
      if (ch < 2 || kb + ST <= D) mmr_chunk(acc, cur.a[ch], DIAG ? cur.a[ch] : cur.b[DIAG ? 0 : ch]);
    ++ks;
  };
  while (ks < KS) {
    stage(f0, f1);
    if (ks < KS) stage(f1, f0);
  }
  return acc;
}

template <typename T, bool SC>
__global__ __launch_bounds__(kMmrThreads) void mmr_kernel(const int32_t* __restrict__ cand,
                                                          const float* __restrict__ rel, const T* __restrict__ c,
                                                          const float* __restrict__ row_scale,
                                                          int64_t* __restrict__ out_ids, float* __restrict__ out_rel,
                                                          float* __restrict__ out_mmr, int N, int D, int R, int k,
                                                          float lam, float mu, int64_t id_base) {
#pragma clang fp contract(off)  // every fp32 operation of the scaling and of the selection rounds once
  __shared__ float G[kMmrSlots * kMmrLd];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 15, g = lane >> 4;
  const int qi = blockIdx.x;
  const int32_t* cq = cand + (size_t)qi * R;
  const int ti = wave >> 1, tj = wave & 1;

  if (16 * max(ti, tj) < R) {  // R == 16: wave 0 alone
    // the row to read for a slot: an id outside [0, N) reads the tile's first valid row, or row 0
    auto tile_row = [&](int t) {
      const int id = cq[16 * t + r];
      const bool ok = (unsigned)id < (unsigned)N;
      const unsigned long long m = __ballot(ok);
      const int first = m ? __ffsll(m) - 1 : 0;  // a lane below 16: all four lane groups hold the same ids
      const int fid = __builtin_amdgcn_readlane(id, first);
      return ok ? id : (m ? fid : 0);
    };
    const int row_a = tile_row(ti), row_b = ti == tj ? row_a : tile_row(tj);
    f32x4 acc = ti == tj ? mmr_tile<T, true>(c, D, row_a, row_a, g) : mmr_tile<T, false>(c, D, row_a, row_b, g);
    if constexpr (SC) {  // row_a / row_b are valid rows: the scale of a dead slot is read but never used
      const float sj = row_scale[row_b];  // column 16 tj + r
#pragma unroll
      for (int e = 0; e < 4; ++e) {  // row 16 ti + 4 g + e: the row lane 4 g + e reads
        const float si = row_scale[__builtin_amdgcn_ds_bpermute(4 * (4 * g + e), row_a)];
        const float ss = si * sj;
        acc[e] = acc[e] * ss;
      }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) G[(16 * ti + 4 * g + e) * kMmrLd + 16 * tj + r] = acc[e];
  }
  __syncthreads();
  if (wave != 0) return;

  const int slot = lane & (kMmrSlots - 1);
  const int id = lane < R ? cq[lane] : kNoRow;
  bool live = (unsigned)id < (unsigned)N;
  const float myrel = lane < R ? rel[(size_t)qi * R + lane] : 0.f;
  const float base = myrel * lam;
  float v = live ? base : -__builtin_inff();
  int myid = live ? id : kNoRow;
  float pen = -__builtin_inff();
  for (int t = 0; t < k; ++t) {
    float bv = v;
    int bi = myid;
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
    const unsigned long long wm = __ballot(live && myid == bi);  // the ids are distinct: one owner, or none left
    const int wl = wm ? __ffsll(wm) - 1 : 0;
    const float wrel = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(myrel), wl));
    if (lane == 0) {
      const size_t o = (size_t)qi * k + t;
      out_ids[o] = id_base + (wm ? bi : kNoRow);
      out_rel[o] = wm ? wrel : -__builtin_inff();
      out_mmr[o] = wm ? bv : -__builtin_inff();
    }
    live = live && !(wm && lane == wl);
    myid = live ? myid : kNoRow;
    const float gw = G[slot * kMmrLd + wl];
    pen = wm ? fmaxf(pen, gw) : pen;
    const float mp = mu * pen;
    v = live ? base - mp : -__builtin_inff();
  }
}

template <typename T>
void mmr_launch(const int32_t* cand, const float* rel, const T* c, const float* row_scale, int64_t* out_ids,
                float* out_rel, float* out_mmr, int nq, int N, int D, int R, int k, float lam, float mu,
                int64_t id_base, hipStream_t stream) {
  if (row_scale)
    hipLaunchKernelGGL((mmr_kernel<T, true>), dim3((unsigned)nq), dim3(kMmrThreads), 0, stream, cand, rel, c, row_scale,
                       out_ids, out_rel, out_mmr, N, D, R, k, lam, mu, id_base);
  else
    hipLaunchKernelGGL((mmr_kernel<T, false>), dim3((unsigned)nq), dim3(kMmrThreads), 0, stream, cand, rel, c, row_scale,
                       out_ids, out_rel, out_mmr, N, D, R, k, lam, mu, id_base);
  ATPU_HIP_CHECK(hipGetLastError());
}

constexpr int kGatherRows = 4;  // rows (waves) per workgroup

template <bool SC>
__global__ __launch_bounds__(kGatherRows* kWave) void rows_gather_kernel(const int64_t* __restrict__ ids,
                                                                         const uint4* __restrict__ store,
                                                                         const float* __restrict__ row_scale,
                                                                         uint4* __restrict__ out,
                                                                         float* __restrict__ out_scale, int m, int N,
                                                                         int pieces, int64_t id_base) {
  const int lane = threadIdx.x & 63, i = blockIdx.x * kGatherRows + (threadIdx.x >> 6);
  if (i >= m) return;
  const int64_t row = ids[i] - id_base;
  const bool ok = row >= 0 && row < (int64_t)N;  // wave-uniform
  const uint4* src = store + (size_t)(ok ? row : 0) * pieces;
  for (int p = lane; p < pieces; p += kWave) out[(size_t)i * pieces + p] = ok ? src[p] : uint4{0u, 0u, 0u, 0u};
  if constexpr (SC)
    if (lane == 0) out_scale[i] = ok ? row_scale[row] : 1.f;
}

}  // namespace

void mmr_select(const int32_t* cand, const float* rel, const void* store, bool half, const float* row_scale,
                int64_t* out_ids, float* out_rel, float* out_mmr, int nq, int N, int D, int R, int k, float lam,
                float mu, int64_t id_base, hipStream_t stream) {
  ATPU_CHECK(nq >= 1 && N >= 1 && N <= 2147483647 - 256, "mmr_select: nq >= 1 and N in [1, 2^31 - 256]");
  ATPU_CHECK(D % 64 == 0 && D >= 64 && D <= 1024, "mmr_select: D must be a multiple of 64 in [64, 1024]");
  ATPU_CHECK(R == 16 || R == kMmrSlots, "mmr_select: R must be 16 or 32 (pad with 0x7fffffff)");
  ATPU_CHECK(k >= 1 && k <= R, "mmr_select: k must be in [1, R]");
  ATPU_CHECK(lam == lam && mu == mu, "mmr_select: lam and mu must be numbers");
  ATPU_CHECK(cand && rel && store && out_ids && out_rel && out_mmr, "mmr_select: null tensor");
  ATPU_CHECK(half || !row_scale, "mmr_select: row_scale goes with an fp16 store");
  ATPU_CHECK((reinterpret_cast<uintptr_t>(store) & 15) == 0 && (reinterpret_cast<uintptr_t>(out_ids) & 7) == 0 &&
                 ((reinterpret_cast<uintptr_t>(cand) | reinterpret_cast<uintptr_t>(rel) |
                   reinterpret_cast<uintptr_t>(row_scale) | reinterpret_cast<uintptr_t>(out_rel) |
                   reinterpret_cast<uintptr_t>(out_mmr)) & 3) == 0,
             "mmr_select: the store must be 16-byte, the ids out 8-byte, the other tensors 4-byte aligned");
  if (half)
    mmr_launch<_Float16>(cand, rel, static_cast<const _Float16*>(store), row_scale, out_ids, out_rel, out_mmr, nq, N, D,
                         R, k, lam, mu, id_base, stream);
  else
    mmr_launch<float>(cand, rel, static_cast<const float*>(store), nullptr, out_ids, out_rel, out_mmr, nq, N, D, R, k,
                      lam, mu, id_base, stream);
}

void rows_gather(const int64_t* ids, const void* store, bool half, const float* row_scale, void* out, float* out_scale,
                 int m, int N, int D, int64_t id_base, hipStream_t stream) {
  ATPU_CHECK(m >= 1 && N >= 1 && N <= 2147483647 - 256, "rows_gather: m >= 1 and N in [1, 2^31 - 256]");
  ATPU_CHECK(D % 64 == 0 && D >= 64 && D <= 1024, "rows_gather: D must be a multiple of 64 in [64, 1024]");
  ATPU_CHECK(ids && store && out, "rows_gather: null tensor");
  ATPU_CHECK((row_scale != nullptr) == (out_scale != nullptr) && (half || !row_scale),
             "rows_gather: row_scale and out_scale go together, with an fp16 store");
  ATPU_CHECK(((reinterpret_cast<uintptr_t>(store) | reinterpret_cast<uintptr_t>(out)) & 15) == 0 &&
                 (reinterpret_cast<uintptr_t>(ids) & 7) == 0 &&
                 ((reinterpret_cast<uintptr_t>(row_scale) | reinterpret_cast<uintptr_t>(out_scale)) & 3) == 0,
             "rows_gather: the store and out must be 16-byte, the ids 8-byte, the scales 4-byte aligned");
  const int pieces = D * (half ? 2 : 4) / 16;
  const dim3 grid((unsigned)((m + kGatherRows - 1) / kGatherRows)), block(kGatherRows * kWave);
  const uint4* s = static_cast<const uint4*>(store);
  uint4* o = static_cast<uint4*>(out);
  if (row_scale)
    hipLaunchKernelGGL((rows_gather_kernel<true>), grid, block, 0, stream, ids, s, row_scale, o, out_scale, m, N, pieces,
                       id_base);
  else
    hipLaunchKernelGGL((rows_gather_kernel<false>), grid, block, 0, stream, ids, s, row_scale, o, out_scale, m, N, pieces,
                       id_base);
  ATPU_HIP_CHECK(hipGetLastError());
}

}  // namespace atpu
