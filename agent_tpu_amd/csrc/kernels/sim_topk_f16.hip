// sim_topk over a float16 corpus: scores = Q [nq, D] fp32 . C [N, D]^T with C stored as fp16, each
// score the exact fp32 dot product of the stored values (an fp16 widens to fp32 exactly; the
// products and sums are those of v_mfma_f32_16x16x4_f32, as in sim_topk.hip), optionally times an
// fp32 row_scale[row] (cosine without storing rounded normalised rows: 4 bytes per row). Only the
// corpus bytes differ from sim_topk.hip: the workgroup shape, the register top-k lists, the LDS
// merge of a split, the workspace [nq, P, k] and sim_topk_merge are the same (that file's header).
//
// sim_topk_f16_kernel<KM, QH, NW, SC>: one workgroup (NW waves) per (corpus split, tile of 16 QH
// queries); a wave streams pairs of 16-row corpus tiles (A operand) against 16 queries (B).
//
// k order of one dot product (a function of D alone): the columns go in chunks of 32; lane
// (r = lane & 15, g = lane >> 4) loads the 16 bytes c[row r][32 cp + 8 g .. + 7], converts them to
// fp32 four at a time, just before use (v_cvt_f32_f16, the high halves through SDWA), and issues
// 8 MFMAs from them, MFMA j taking element j: the hardware's k index g stands for column
// 32 cp + 8 g + j, and the chain of a chunk runs j = 0 .. 7. One fp32 accumulator per (query, row),
// fed in that order whatever the query's slot, the wave, the split, N or P. With SC the
// accumulator is multiplied once by row_scale[row] before it meets the lists: the ranking uses
// the scaled value.
//
// The query tile in LDS is a permuted image: within every 32 columns the 16-byte piece 2 g + hf
// (columns 8 g + 4 hf .. + 3) sits at piece 4 hf + g, so the ds_read_b128 of (cp, hf) is at float
// r * ldq + 32 cp + 16 hf + 4 g: consecutive g are one 16-byte slot apart. With the row stride
// ldq = D + 8 floats (two slots) the two half-groups that a ds_read_b128 serves together (8 lanes
// of an even g and 8 of the next odd g) take the even and the odd slots of the 64 banks: no
// conflict. (The natural image, g two slots apart, puts both half-groups on even slots with this
// stride and has no conflict-free 16-byte-aligned stride at all.)
//
// A step is 128 columns (four chunks) of both corpus tiles, loaded one step ahead of the MFMAs
// that consume it into two fragment buffers that take turns: 8 x 16 B in flight per lane, the
// bytes of sim_topk.hip's step. Every step issues the same 8 loads, and no load sits under a
// branch: the s_waitcnt before a step's first MFMA then counts exactly the loads issued after
// the step's own and leaves all of them in flight (with two chunks' loads under a branch the
// compiler waited for half of the next step's loads there, and the kernel ran at the fp32
// kernel's time). When D is an odd multiple of 64 the last step of a row pair has two chunks: its
// other two loads repeat them (cache hits) and only their MFMAs are skipped, by a scalar branch
// (the wave index is made scalar for that). With SC the 8 row scales of a lane (rows past N
// clamped) are loaded at the head of every step, before the corpus loads, so the wait for them
// in the rows' last step leaves the next step's loads in flight as well.
//
// NW and registers (docs/PERF_NOTES.md; no form spills): 32 queries as in sim_topk.hip, 8 waves
// with KM <= 16 and 4 with KM = 32 (256 VGPRs + AGPRs, more than two waves per SIMD can have). The
// 16-query form has 8 waves for every KM (at most 223 VGPRs): its grid is one workgroup per
// split, never more than one per CU, so only the waves of a workgroup add loads in flight, and a
// step of fp16 carries twice the MFMAs per byte (N = 2^20, D = 768, 1 query: 409 us with 4 waves,
// 340 us with 8; the fp32 kernel 557 us).
//
// Rows past the corpus: the row index is clamped to N - 1 (for c and for row_scale) and the score
// discarded by select, never multiplied by 0: nothing outside c[0:N] and row_scale[0:N] is read.
#include "atpu/common.h"
#include "atpu/kernels.h"
#include "atpu/topk.h"

namespace atpu {
namespace {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

constexpr int kSimRows = 32;   // corpus rows per wave step: two 16-row MFMA tiles (sim_topk_splits' unit)
constexpr int kSimStep = 128;  // columns per full load step
constexpr int kSimPad = 8;     // floats of padding per LDS query row
constexpr int kNoRow = 0x7fffffff;

struct SimFrag16 {
  f16x8 a[2][4];  // [corpus tile][chunk of 32 columns]
};

__device__ __forceinline__ void sim_load(SimFrag16& f, const _Float16* __restrict__ c, int D, int N, int row0, int r,
                                         int g, int kb) {
  const int hi = kb + kSimStep <= D ? 64 : 0;  // a two-chunk tail step loads its chunks twice
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

template <int KM, int QH, int NW, bool SC>
__global__ __launch_bounds__(NW * kWave) void sim_topk_f16_kernel(const float* __restrict__ q,
                                                                   const _Float16* __restrict__ c,
                                                                   const float* __restrict__ row_scale,
                                                                   float2* __restrict__ ws, int nq, int N, int D,
                                                                   int k, int P, int steps_per_split) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int QT = 16 * QH;
  constexpr int L = 4 * NW;  // lists per query at the end of a split: 4 lane groups x NW waves
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 15, g = lane >> 4;
  const int split = blockIdx.x, q0 = blockIdx.y * QT;
  const int ldq = D + kSimPad;

  // query tile -> LDS, permuted (header); slots past nq repeat the last query
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
  const int s_lo = split * steps_per_split, s_hi = min(s_lo + steps_per_split, nsteps);
  const int KS = (D + kSimStep - 1) / kSimStep;
  const float* qb = smem + r * ldq + 4 * g;

  // The wave's (rows, columns) steps form one stream, as in sim_topk.hip: the loads of step i + 1
  // are issued before the MFMAs of step i; rows past this wave's last are clamped into c[0:N].
  SimFrag16 f0, f1;
  int s = s_lo + wave, ks = 0;
  f32x4 acc[2][QH];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int h = 0; h < QH; ++h) acc[t][h] = f32x4{0.f, 0.f, 0.f, 0.f};
  if (s < s_hi) sim_load(f0, c, D, N, s * kSimRows, r, g, 0);
  auto stage = [&](const SimFrag16& cur, SimFrag16& nxt) {
    const bool last = ks + 1 == KS;
    const int ns = last ? s + NW : s, nks = last ? 0 : ks + 1;
    const int kb = ks * kSimStep;
    float rs[2][4];
    if constexpr (SC) {
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int e = 0; e < 4; ++e) rs[t][e] = row_scale[min(s * kSimRows + t * 16 + g * 4 + e, N - 1)];
      __builtin_amdgcn_sched_barrier(0);
    }
    sim_load(nxt, c, D, N, ns * kSimRows, r, g, nks * kSimStep);
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
    if (kb + kSimStep <= D) {
      chunk(2);
      chunk(3);
    }
    if (last) {  // the rows' scores are complete: scaled, then into the lists
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int row = s * kSimRows + t * 16 + g * 4 + e;
          const bool live = row < N;
#pragma unroll
          for (int h = 0; h < QH; ++h) {
            float sv = acc[t][h][e];
            if constexpr (SC) sv *= rs[t][e];
            const float v = live ? sv : -__builtin_inff();
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

  // the L lists of every query -> LDS (over the query tile, which is no longer read), then L lanes
  // per query pop the best head k times: sim_topk.hip's split epilogue, unchanged
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

size_t sim_lds_bytes(int D, int KM, int QT, int NW) {
  const size_t qbytes = (size_t)QT * (D + kSimPad) * sizeof(float);
  const size_t mbytes = (size_t)QT * 4 * NW * KM * sizeof(float2);
  return qbytes > mbytes ? qbytes : mbytes;
}

template <int KM, int QH, int NW, bool SC>
void sim_launch(const float* q, const _Float16* c, const float* row_scale, float2* ws, int nq, int N, int D, int k,
                int P, int sps, hipStream_t stream) {
  constexpr int QT = 16 * QH;
  const size_t lds = sim_lds_bytes(D, KM, QT, NW);
  // up to 129 KiB of dynamic LDS (D = 1024, 32 queries); the attribute is per device
  ATPU_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&sim_topk_f16_kernel<KM, QH, NW, SC>),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL((sim_topk_f16_kernel<KM, QH, NW, SC>), dim3(P, (nq + QT - 1) / QT), dim3(NW * kWave), lds,
                     stream, q, c, row_scale, ws, nq, N, D, k, P, sps);
  ATPU_HIP_CHECK(hipGetLastError());
}

template <bool SC>
void sim_dispatch(const float* q, const _Float16* c, const float* row_scale, float2* w, int nq, int N, int D, int k,
                  int P, int sps, hipStream_t stream) {
  const bool wide = nq > 16;  // one or two 16-query halves per workgroup, as sim_topk_partial
#define ATPU_SIM_CASE(KM, NWIDE)                                                              \
  do {                                                                                        \
    if (wide) sim_launch<KM, 2, NWIDE, SC>(q, c, row_scale, w, nq, N, D, k, P, sps, stream);  \
    else sim_launch<KM, 1, 8, SC>(q, c, row_scale, w, nq, N, D, k, P, sps, stream);           \
  } while (0)
  if (k <= 8) ATPU_SIM_CASE(8, 8);
  else if (k <= 16) ATPU_SIM_CASE(16, 8);
  else ATPU_SIM_CASE(32, 4);
#undef ATPU_SIM_CASE
}

}  // namespace

void sim_topk_partial_f16(const float* q, const _Float16* c, const float* row_scale, float* ws, int nq, int N, int D,
                          int k, int P, hipStream_t stream) {
  ATPU_CHECK(nq >= 1 && N >= 1, "sim_topk: nq and N must be >= 1");
  ATPU_CHECK(D % 64 == 0 && D >= 64 && D <= 1024, "sim_topk: D must be a multiple of 64 in [64, 1024]");
  ATPU_CHECK(k >= 1 && k <= 32, "sim_topk: k must be in [1, 32]");
  ATPU_CHECK(P >= 1 && P == sim_topk_splits(N, P), "sim_topk: P must come from sim_topk_splits");
  ATPU_CHECK(q && c && ws, "sim_topk: null tensor");
  ATPU_CHECK(((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(c)) & 15) == 0 &&
                 (reinterpret_cast<uintptr_t>(ws) & 7) == 0 && (reinterpret_cast<uintptr_t>(row_scale) & 3) == 0,
             "sim_topk: q and c must be 16-byte, the workspace 8-byte and row_scale 4-byte aligned");
  const int nsteps = (N + kSimRows - 1) / kSimRows;
  const int sps = (nsteps + P - 1) / P;
  float2* w = reinterpret_cast<float2*>(ws);
  if (row_scale) sim_dispatch<true>(q, c, row_scale, w, nq, N, D, k, P, sps, stream);
  else sim_dispatch<false>(q, c, nullptr, w, nq, N, D, k, P, sps, stream);
}

}  // namespace atpu
