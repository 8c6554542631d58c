// Filtered top-k similarity search: sim_topk (sim_topk.hip, sim_topk_f16.hip) over the corpus rows
// that a bit mask allows, with the filter in the epilogue and in the step walk. The result is, bit
// for bit, sim_topk over the gathered allowed rows with the ids mapped back.
//
// Row mask: int32 words [ceil(N / 32)], bit b of word w = row 32 w + b: one word is one wave step
// (kSimRows = 32). It comes with the live-step list: live [n_live] int32, the indices of the
// non-zero words, ascending.
//
// sim_topk_masked_kernel / sim_topk_masked_f16_kernel are the unmasked kernels (their headers hold
// the tile, the k order, the LDS image, the prefetch and the register notes) with two differences:
//
// Step walk. A workgroup's steps are live[lo:hi] instead of [s_lo, s_hi): wave w takes entries
// lo + w, lo + w + NW, ...; the one-step-ahead prefetch targets the wave's next entry (the last
// entry once more past the end: a cache hit inside c[0:N]). A step whose word is zero is in no
// list, so it is never loaded and never multiplied. P comes from n_live as sim_topk_splits takes it
// from the step count, so the splits balance when the allowed rows are one contiguous block. The
// entry after next and the step's word are wave-uniform loads at the head of every stage, before
// the corpus loads: waiting for them leaves the prefetch in flight (as row_scale in sim_topk_f16.hip).
//
// Epilogue. Row 32 s + 16 t + 4 g + e enters the lists only if its bit is set and row < N;
// otherwise as (-inf, kNoRow) by select, as rows past the corpus do: never multiplied by 0, so a
// NaN in a masked row cannot leak. Bits of the last word at or past N are ignored.
//
// Score bits: the k order of one dot product (chunk map, j-major MFMA chain, one accumulator per
// pair; fp16 widened in registers, row_scale once into the finished accumulator) is that of the
// unmasked kernels, so a score has sim_topk's bits for the same (q, row).
//
// Read bounds: nothing outside c[0:N], row_scale[0:N], words[0:ceil(N/32)] and live[0:n_live] is
// read; an entry of live is clamped into the words.
//
// Mask builders: row_mask_from_ids (memset, atomicOr per id, optional inversion with the tail
// cleared), row_mask_from_labels (one wave per 64 rows: membership test, __ballot gives two words);
// the count of set bits is a popcount with one integer atomic per wave.
#include "atpu/common.h"
#include "atpu/kernels.h"
#include "atpu/topk.h"

namespace atpu {
namespace {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

constexpr int kSimRows = 32;  // corpus rows per wave step: two 16-row MFMA tiles, one mask word
constexpr int kNoRow = 0x7fffffff;
constexpr int kMaskThreads = 256;

// fp32 corpus: sim_topk.hip's step (64 columns, LDS row stride D + 4)
constexpr int kStep32 = 64;
constexpr int kPad32 = 4;
// fp16 corpus: sim_topk_f16.hip's step (128 columns, permuted LDS image, row stride D + 8)
constexpr int kStep16 = 128;
constexpr int kPad16 = 8;

struct SimFrag {
  f32x4 a[2][4];  // [corpus tile][chunk]
};
struct SimFrag16 {
  f16x8 a[2][4];  // [corpus tile][chunk of 32 columns]
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

__device__ __forceinline__ void sim_load(SimFrag16& f, const _Float16* __restrict__ c, int D, int N, int row0, int r,
                                         int g, int kb) {
  const int hi = kb + kStep16 <= D ? 64 : 0;  // a two-chunk tail step loads its chunks twice
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int row = min(row0 + t * 16 + r, N - 1);  // clamp, the score is discarded by select
    const _Float16* p = c + (size_t)row * D + kb + 8 * g;
    f.a[t][0] = *reinterpret_cast<const f16x8*>(p);
    f.a[t][1] = *reinterpret_cast<const f16x8*>(p + 32);
    f.a[t][2] = *reinterpret_cast<const f16x8*>(p + hi);
    f.a[t][3] = *reinterpret_cast<const f16x8*>(p + hi + 32);
  }
}

// entry i of the live list (i clamped into [0, n_hi)), itself clamped into the words
__device__ __forceinline__ int live_step(const int* __restrict__ live, int i, int n_hi, int nsteps) {
  return max(0, min(live[max(0, min(i, n_hi - 1))], nsteps - 1));
}

// Epilogue of one step: the 8 scores of a lane per query half into the lists, by the mask word.
template <int KM, int QH, bool SC>
__device__ __forceinline__ void sim_lists_take(float (&tv)[QH][KM], int (&ti)[QH][KM], const f32x4 (&acc)[2][QH],
                                               const float (&rs)[2][4], int s, int g, int N, unsigned word) {
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int bit = t * 16 + g * 4 + e;
      const int row = s * kSimRows + bit;
      const bool live = row < N && ((word >> bit) & 1u) != 0;
#pragma unroll
      for (int h = 0; h < QH; ++h) {
        float sv = acc[t][h][e];
        if constexpr (SC) sv *= rs[t][e];
        const float v = live ? sv : -__builtin_inff();
        const int id = live ? row : kNoRow;
        if (__ballot(better(v, id, tv[h][KM - 1], ti[h][KM - 1])) != 0) list_insert<KM>(tv[h], ti[h], v, id);
      }
    }
}

// End of a split, as in sim_topk.hip: the L = 4 NW lists of every query meet in LDS (over the query
// tile, which is no longer read), where L lanes per query pop the best head k times.
template <int KM, int QH, int NW>
__device__ __forceinline__ void sim_lists_merge(const float (&tv)[QH][KM], const int (&ti)[QH][KM], float* smem,
                                                float2* __restrict__ ws, int lane, int wave, int r, int g, int q0,
                                                int nq, int P, int split, int k) {
  constexpr int L = 4 * NW;
  __syncthreads();
  float2* ml = reinterpret_cast<float2*>(smem);
#pragma unroll
  for (int h = 0; h < QH; ++h) {
    float2* dst = ml + ((h * 16 + r) * L + wave * 4 + g) * KM;
#pragma unroll
    for (int e = 0; e < KM; ++e) dst[e] = float2{tv[h][e], __int_as_float(ti[h][e])};
  }
  __syncthreads();
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

template <int KM, int QH, int NW>
__global__ __launch_bounds__(NW * kWave) void sim_topk_masked_kernel(const float* __restrict__ q,
                                                                      const float* __restrict__ c,
                                                                      const int* __restrict__ words,
                                                                      const int* __restrict__ live,
                                                                      float2* __restrict__ ws, int nq, int N, int D,
                                                                      int k, int P, int n_live, int per_split) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int QT = 16 * QH;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 15, g = lane >> 4;
  const int split = blockIdx.x, q0 = blockIdx.y * QT;
  const int ldq = D + kPad32;

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
  const int n_lo = split * per_split, n_hi = min(n_lo + per_split, n_live);
  const int KS = D / kStep32;
  const float* qb = smem + r * ldq + 4 * g;

  // The wave's (live entry, columns) steps form one stream; two fragment buffers take turns, and
  // the loads of step i + 1 are issued before the MFMAs of step i: the next 64 columns, or the
  // first 64 of the wave's next live entry (past its last: that entry again, inside c[0:N]).
  SimFrag f0, f1;
  int idx = n_lo + wave, ks = 0;
  int s = live_step(live, idx, n_hi, nsteps), s_next = live_step(live, idx + NW, n_hi, nsteps);
  f32x4 acc[2][QH];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int h = 0; h < QH; ++h) acc[t][h] = f32x4{0.f, 0.f, 0.f, 0.f};
  const float rs[2][4] = {{1.f, 1.f, 1.f, 1.f}, {1.f, 1.f, 1.f, 1.f}};  // unused: no row scale
  if (idx < n_hi) sim_load(f0, c, D, N, s * kSimRows, r, g, 0);
  auto stage = [&](const SimFrag& cur, SimFrag& nxt) {
    const bool last = ks + 1 == KS;
    const int ns = last ? s_next : s, nks = last ? 0 : ks + 1;
    const unsigned word = (unsigned)words[s];
    const int s_after = live_step(live, idx + 2 * NW, n_hi, nsteps);
    __builtin_amdgcn_sched_barrier(0);
    sim_load(nxt, c, D, N, ns * kSimRows, r, g, nks * kStep32);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int ch = 0; ch < 4; ++ch) {
      f32x4 b[QH];
#pragma unroll
      for (int h = 0; h < QH; ++h)
        b[h] = *reinterpret_cast<const f32x4*>(qb + h * 16 * ldq + ks * kStep32 + 16 * ch);
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int h = 0; h < QH; ++h)
            acc[t][h] = __builtin_amdgcn_mfma_f32_16x16x4f32(cur.a[t][ch][j], b[h][j], acc[t][h], 0, 0, 0);
    }
    if (last) {  // the rows' scores are complete: into the lists, by the mask word
      sim_lists_take<KM, QH, false>(tv, ti, acc, rs, s, g, N, word);
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int h = 0; h < QH; ++h) acc[t][h] = f32x4{0.f, 0.f, 0.f, 0.f};
      idx += NW;
      s = s_next;
      s_next = s_after;
    }
    ks = nks;
  };
  while (idx < n_hi) {
    stage(f0, f1);
    if (idx < n_hi) stage(f1, f0);
  }

  sim_lists_merge<KM, QH, NW>(tv, ti, smem, ws, lane, wave, r, g, q0, nq, P, split, k);
}

template <int KM, int QH, int NW, bool SC>
__global__ __launch_bounds__(NW * kWave) void sim_topk_masked_f16_kernel(
    const float* __restrict__ q, const _Float16* __restrict__ c, const float* __restrict__ row_scale,
    const int* __restrict__ words, const int* __restrict__ live, float2* __restrict__ ws, int nq, int N, int D, int k,
    int P, int n_live, int per_split) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int QT = 16 * QH;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 15, g = lane >> 4;
  const int split = blockIdx.x, q0 = blockIdx.y * QT;
  const int ldq = D + kPad16;

  // query tile -> LDS, permuted (sim_topk_f16.hip's header); slots past nq repeat the last query
  const int c4 = D >> 2;
  for (int i = tid; i < QT * c4; i += NW * kWave) {
    const int qi = i / c4, cc = i - qi * c4;
    const int qr = min(q0 + qi, nq - 1);
    const int u = cc & 7, pc = (cc & ~7) + 4 * (u & 1) + (u >> 1);
    *reinterpret_cast<f32x4*>(smem + qi * ldq + pc * 4) = *reinterpret_cast<const f32x4*>(q + (size_t)qr * D + cc * 4);
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
  const int n_lo = split * per_split, n_hi = min(n_lo + per_split, n_live);
  const int KS = (D + kStep16 - 1) / kStep16;
  const float* qb = smem + r * ldq + 4 * g;

  SimFrag16 f0, f1;
  int idx = n_lo + wave, ks = 0;
  int s = live_step(live, idx, n_hi, nsteps), s_next = live_step(live, idx + NW, n_hi, nsteps);
  f32x4 acc[2][QH];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int h = 0; h < QH; ++h) acc[t][h] = f32x4{0.f, 0.f, 0.f, 0.f};
  if (idx < n_hi) sim_load(f0, c, D, N, s * kSimRows, r, g, 0);
  auto stage = [&](const SimFrag16& cur, SimFrag16& nxt) {
    const bool last = ks + 1 == KS;
    const int ns = last ? s_next : s, nks = last ? 0 : ks + 1;
    const int kb = ks * kStep16;
    const unsigned word = (unsigned)words[s];
    const int s_after = live_step(live, idx + 2 * NW, n_hi, nsteps);
    float rs[2][4];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if constexpr (SC) rs[t][e] = row_scale[min(s * kSimRows + t * 16 + g * 4 + e, N - 1)];
        else rs[t][e] = 1.f;
      }
    __builtin_amdgcn_sched_barrier(0);
    sim_load(nxt, c, D, N, ns * kSimRows, r, g, nks * kStep16);
    __builtin_amdgcn_sched_barrier(0);
    auto chunk = [&](int cp) {
#pragma unroll
      for (int hf = 0; hf < 2; ++hf) {
        f32x4 b[QH];
#pragma unroll
        for (int h = 0; h < QH; ++h)
          b[h] = *reinterpret_cast<const f32x4*>(qb + h * 16 * ldq + kb + 32 * cp + 16 * hf);
        float a[2][4];  // converted just in time: 8 registers live, not a step's 64
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int j = 0; j < 4; ++j) a[t][j] = (float)cur.a[t][cp][4 * hf + j];
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int h = 0; h < QH; ++h)
              acc[t][h] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t][j], b[h][j], acc[t][h], 0, 0, 0);
      }
    };
    chunk(0);
    chunk(1);
    if (kb + kStep16 <= D) {
      chunk(2);
      chunk(3);
    }
    if (last) {  // the rows' scores are complete: scaled, then into the lists, by the mask word
      sim_lists_take<KM, QH, SC>(tv, ti, acc, rs, s, g, N, word);
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int h = 0; h < QH; ++h) acc[t][h] = f32x4{0.f, 0.f, 0.f, 0.f};
      idx += NW;
      s = s_next;
      s_next = s_after;
    }
    ks = nks;
  };
  while (idx < n_hi) {
    stage(f0, f1);
    if (idx < n_hi) stage(f1, f0);
  }

  sim_lists_merge<KM, QH, NW>(tv, ti, smem, ws, lane, wave, r, g, q0, nq, P, split, k);
}

size_t sim_lds_bytes(int D, int pad, int KM, int QT, int NW) {
  const size_t qbytes = (size_t)QT * (D + pad) * sizeof(float);
  const size_t mbytes = (size_t)QT * 4 * NW * KM * sizeof(float2);
  return qbytes > mbytes ? qbytes : mbytes;
}

struct MaskedArgs {
  const float* q;
  const int* words;
  const int* live;
  float2* ws;
  int nq, N, D, k, P, n_live, per_split;
  hipStream_t stream;
};

template <int KM, int QH, int NW>
void sim_launch(const MaskedArgs& a, const float* c) {
  constexpr int QT = 16 * QH;
  const size_t lds = sim_lds_bytes(a.D, kPad32, KM, QT, NW);
  ATPU_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&sim_topk_masked_kernel<KM, QH, NW>),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL((sim_topk_masked_kernel<KM, QH, NW>), dim3(a.P, (a.nq + QT - 1) / QT), dim3(NW * kWave), lds,
                     a.stream, a.q, c, a.words, a.live, a.ws, a.nq, a.N, a.D, a.k, a.P, a.n_live, a.per_split);
  ATPU_HIP_CHECK(hipGetLastError());
}

template <int KM, int QH, int NW, bool SC>
void sim_launch(const MaskedArgs& a, const _Float16* c, const float* row_scale) {
  constexpr int QT = 16 * QH;
  const size_t lds = sim_lds_bytes(a.D, kPad16, KM, QT, NW);
  ATPU_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&sim_topk_masked_f16_kernel<KM, QH, NW, SC>),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL((sim_topk_masked_f16_kernel<KM, QH, NW, SC>), dim3(a.P, (a.nq + QT - 1) / QT), dim3(NW * kWave),
                     lds, a.stream, a.q, c, row_scale, a.words, a.live, a.ws, a.nq, a.N, a.D, a.k, a.P, a.n_live,
                     a.per_split);
  ATPU_HIP_CHECK(hipGetLastError());
}

template <bool SC>
void sim_dispatch(const MaskedArgs& a, const _Float16* c, const float* row_scale) {
  const bool wide = a.nq > 16;  // the launch forms of sim_topk_partial_f16
#define ATPU_SIM_CASE(KM, NWIDE)                                   \
  do {                                                             \
    if (wide) sim_launch<KM, 2, NWIDE, SC>(a, c, row_scale);       \
    else sim_launch<KM, 1, 8, SC>(a, c, row_scale);                \
  } while (0)
  if (a.k <= 8) ATPU_SIM_CASE(8, 8);
  else if (a.k <= 16) ATPU_SIM_CASE(16, 8);
  else ATPU_SIM_CASE(32, 4);
#undef ATPU_SIM_CASE
}

MaskedArgs masked_args(const float* q, const void* c, const int32_t* words, const int32_t* live, float* ws, int nq,
                       int N, int D, int k, int P, int n_live, hipStream_t stream) {
  ATPU_CHECK(nq >= 1 && N >= 1, "sim_topk: nq and N must be >= 1");
  ATPU_CHECK(D % 64 == 0 && D >= 64 && D <= 1024, "sim_topk: D must be a multiple of 64 in [64, 1024]");
  ATPU_CHECK(k >= 1 && k <= 32, "sim_topk: k must be in [1, 32]");
  ATPU_CHECK(n_live >= 1 && n_live <= (N + kSimRows - 1) / kSimRows,
             "sim_topk: n_live must be in [1, ceil(N / 32)]");
  ATPU_CHECK(P >= 1 && P == sim_topk_splits_live(n_live, P), "sim_topk: P must come from sim_topk_splits_live");
  ATPU_CHECK(q && c && ws && words && live, "sim_topk: null tensor");
  ATPU_CHECK(((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(c)) & 15) == 0 &&
                 (reinterpret_cast<uintptr_t>(ws) & 7) == 0 &&
                 ((reinterpret_cast<uintptr_t>(words) | reinterpret_cast<uintptr_t>(live)) & 3) == 0,
             "sim_topk: q and c must be 16-byte, the workspace 8-byte, the mask words and live 4-byte aligned");
  return MaskedArgs{q, words, live, reinterpret_cast<float2*>(ws), nq, N, D, k, P, n_live, (n_live + P - 1) / P,
                    stream};
}

// ------------------------------------------------------------------------------------ mask builders
__global__ __launch_bounds__(kMaskThreads) void row_mask_set_ids_kernel(const int64_t* __restrict__ ids, int64_t m,
                                                                        int64_t base, int N,
                                                                        unsigned* __restrict__ words) {
  for (int64_t i = blockIdx.x * (int64_t)kMaskThreads + threadIdx.x; i < m; i += (int64_t)gridDim.x * kMaskThreads) {
    const int64_t id = ids[i];
    if (id < base || id - base >= N) continue;  // another slice's row
    const int row = (int)(id - base);
    atomicOr(words + (row >> 5), 1u << (row & 31));
  }
}

// optional inversion (tail bits at or past N cleared), then the count of set bits
__global__ __launch_bounds__(kMaskThreads) void row_mask_finish_kernel(unsigned* __restrict__ words, int nwords, int N,
                                                                       int invert, int64_t* __restrict__ count) {
  const int lane = threadIdx.x & 63;
  int n = 0;
  for (int w = blockIdx.x * kMaskThreads + threadIdx.x; w < nwords; w += gridDim.x * kMaskThreads) {
    unsigned x = words[w];
    if (invert) {
      x = ~x;
      const int rows = N - w * 32;  // >= 1
      if (rows < 32) x &= (1u << rows) - 1u;
      words[w] = x;
    }
    n += __popc(x);
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) n += __shfl_xor(n, d);
  if (lane == 0 && n != 0) atomicAdd(reinterpret_cast<unsigned long long*>(count), (unsigned long long)n);
}

// one wave per 64 rows: membership, ballot -> two words; values sit sorted in LDS (m <= 256)
__global__ __launch_bounds__(kMaskThreads) void row_mask_labels_kernel(const int64_t* __restrict__ labels, int N,
                                                                       const int64_t* __restrict__ values, int m,
                                                                       int64_t lo, int64_t hi,
                                                                       unsigned* __restrict__ words, int nwords,
                                                                       int64_t* __restrict__ count) {
  __shared__ int64_t vals[kRowMaskMaxValues];
  if (values != nullptr)
    for (int i = threadIdx.x; i < m; i += kMaskThreads) vals[i] = values[i];
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int64_t row = blockIdx.x * (int64_t)kMaskThreads + threadIdx.x;
  bool hit = false;
  if (row < N) {
    const int64_t x = labels[row];
    if (values != nullptr) {
      int a = 0, b = m;  // first index with vals[i] >= x
      while (a < b) {
        const int mid = (a + b) >> 1;
        if (vals[mid] < x) a = mid + 1;
        else b = mid;
      }
      hit = a < m && vals[a] == x;
    } else {
      hit = lo <= x && x <= hi;
    }
  }
  const unsigned long long bal = __ballot(hit);
  if (lane == 0) {
    const int w = (int)((row >> 6) << 1);  // row is the wave's first
    if (w < nwords) words[w] = (unsigned)bal;
    if (w + 1 < nwords) words[w + 1] = (unsigned)(bal >> 32);
    if (bal != 0) atomicAdd(reinterpret_cast<unsigned long long*>(count), (unsigned long long)__popcll(bal));
  }
}

int mask_grid(int64_t items) {
  const int64_t wgs = (items + kMaskThreads - 1) / kMaskThreads;
  return (int)(wgs < 1 ? 1 : (wgs > 2048 ? 2048 : wgs));
}

}  // namespace

int sim_topk_splits_live(int n_live, int want) {
  const int p = want < 1 ? 1 : (want > kSimMaxSplits ? kSimMaxSplits : want);
  const int per = (n_live + p - 1) / p;
  return per < 1 ? 1 : (n_live + per - 1) / per;  // no empty split
}

void sim_topk_partial_masked(const float* q, const float* c, const int32_t* words, const int32_t* live, float* ws,
                             int nq, int N, int D, int k, int P, int n_live, hipStream_t stream) {
  const MaskedArgs a = masked_args(q, c, words, live, ws, nq, N, D, k, P, n_live, stream);
  const bool wide = nq > 16;  // the launch forms of sim_topk_partial
#define ATPU_SIM_CASE(KM, NWIDE)                      \
  do {                                                \
    if (wide) sim_launch<KM, 2, NWIDE>(a, c);         \
    else sim_launch<KM, 1, 4>(a, c);                  \
  } while (0)
  if (k <= 8) ATPU_SIM_CASE(8, 8);
  else if (k <= 16) ATPU_SIM_CASE(16, 8);
  else ATPU_SIM_CASE(32, 4);
#undef ATPU_SIM_CASE
}

void sim_topk_partial_masked_f16(const float* q, const _Float16* c, const float* row_scale, const int32_t* words,
                                 const int32_t* live, float* ws, int nq, int N, int D, int k, int P, int n_live,
                                 hipStream_t stream) {
  ATPU_CHECK((reinterpret_cast<uintptr_t>(row_scale) & 3) == 0, "sim_topk: row_scale must be 4-byte aligned");
  const MaskedArgs a = masked_args(q, c, words, live, ws, nq, N, D, k, P, n_live, stream);
  if (row_scale) sim_dispatch<true>(a, c, row_scale);
  else sim_dispatch<false>(a, c, nullptr);
}

void row_mask_from_ids(const int64_t* ids, int64_t m, int64_t base, int N, int exclude, int32_t* words,
                       int64_t* count, hipStream_t stream) {
  ATPU_CHECK(N >= 1 && m >= 0, "row_mask_from_ids: N must be >= 1 and m >= 0");
  ATPU_CHECK(words && count && (ids || m == 0), "row_mask_from_ids: null tensor");
  const int nwords = (N + 31) / 32;
  ATPU_HIP_CHECK(hipMemsetAsync(words, 0, (size_t)nwords * sizeof(int32_t), stream));
  ATPU_HIP_CHECK(hipMemsetAsync(count, 0, sizeof(int64_t), stream));
  unsigned* w = reinterpret_cast<unsigned*>(words);
  if (m > 0) {
    hipLaunchKernelGGL(row_mask_set_ids_kernel, dim3(mask_grid(m)), dim3(kMaskThreads), 0, stream, ids, m, base, N, w);
    ATPU_HIP_CHECK(hipGetLastError());
  }
  hipLaunchKernelGGL(row_mask_finish_kernel, dim3(mask_grid(nwords)), dim3(kMaskThreads), 0, stream, w, nwords, N,
                     exclude ? 1 : 0, count);
  ATPU_HIP_CHECK(hipGetLastError());
}

void row_mask_from_labels(const int64_t* labels, int N, const int64_t* values, int m, int64_t lo, int64_t hi,
                          int32_t* words, int64_t* count, hipStream_t stream) {
  ATPU_CHECK(N >= 1, "row_mask_from_labels: N must be >= 1");
  ATPU_CHECK(labels && words && count, "row_mask_from_labels: null tensor");
  ATPU_CHECK(values == nullptr || (m >= 1 && m <= kRowMaskMaxValues),
             "row_mask_from_labels: 1 to 256 sorted values, or none for a range");
  const int nwords = (N + 31) / 32;
  ATPU_HIP_CHECK(hipMemsetAsync(count, 0, sizeof(int64_t), stream));
  const int wgs = (N + kMaskThreads - 1) / kMaskThreads;  // N < 2^31: at most 2^23 workgroups
  hipLaunchKernelGGL(row_mask_labels_kernel, dim3(wgs), dim3(kMaskThreads), 0, stream, labels, N, values, m, lo, hi,
                     reinterpret_cast<unsigned*>(words), nwords, count);
  ATPU_HIP_CHECK(hipGetLastError());
}

}  // namespace atpu
