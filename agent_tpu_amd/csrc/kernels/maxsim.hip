// Late-interaction (ColBERT) scoring: unit token vectors and the fused MaxSim of a (query, passage) pair,
//   score(q, d) = sum_{i < len_q} max_{j < len_d} <Q[q, i], D[d, j]>,
// in exact fp32 on v_mfma_f32_16x16x4_f32. The [S, S] matrix of dot products never exists: the max
// over the passage tokens is taken on the accumulator registers, the sum over the query tokens by
// one lane.
//
// token_unit_kernel: one wave per row of x [M, P] (bf16 or fp32), four rows per workgroup. Lane l holds
// columns l, l + 64, ...; the squares are summed per lane in increasing column, then by wave_sum's
// fixed butterfly: an order that depends on P alone. out = x / max(||x||, 1e-12), pool_embed's
// arithmetic (a zero row stays zero).
//
// maxsim_kernel: one workgroup of four waves per pair. It walks the query's tokens i < len_q in tiles
// of 16; the tile sits in LDS (row stride P + 4 floats, as sim_topk's query tile: the 16 rows a
// ds_read_b128 touches start 4 banks apart). The waves split the passage's tokens j < len_d in steps
// of 32 (two 16-row MFMA tiles, two independent accumulators per wave for the 40-cycle dependent
// latency): passage tokens are the A operand, the 16 query tokens B, so in the C/D layout
// col = lane & 15 is the query token and row = (lane >> 4) * 4 + reg the passage token.
//
// k order of one dot product: sim_topk's. The columns go in chunks of 16; lane (r = lane & 15,
// g = lane >> 4) loads the 16 bytes d[row r][16 ch + 4 g .. + 3] and issues 4 MFMAs from them, MFMA j
// taking element j: columns 0, 4, 8, 12, 1, 5, ... of a chunk, chunks ascending, into one accumulator
// per (query token, passage token). A dot product's bits are a function of P and its two rows alone.
// 64 columns of both passage tiles are loaded one step ahead of the MFMAs that consume them, into two
// fragment buffers that take turns.
//
// Each lane keeps the running max of its accumulator registers for its query token; the four lane
// groups meet by xor16 / xor32, the four waves in LDS, and thread 0 adds the tile's maxima to the
// pair's sum in increasing token index: ((m0 + m1) + m2) + ... in fp32. The score is a function of the
// pair's own rows and lengths only, not of n, the pair's position, Qn, Dn or the launch.
//
// Masking is clamp-then-select (rerank.hip's rule): qidx / didx are clamped into [0, Qn) / [0, Dn) and
// the lens into [1, S] before they form an address; token rows past S are clamped to S - 1; a passage
// token j >= len_d enters the max as -inf by select (never multiplied by 0, never biased), a query
// token i >= len_q is not added. An MFMA output depends on its own A row and B column only, so
// whatever padding rows hold, NaN included, reaches no live score. Nothing outside the given tensors
// is read. A NaN in a live dot product: undefined, as in sim_topk.
#include "atpu/common.h"
#include "atpu/kernels.h"

namespace atpu {
namespace {

constexpr int kMsThreads = 256;
constexpr int kMsWaves = kMsThreads / kWave;
constexpr int kMsRows = 32;  // passage tokens per wave step: two 16-row MFMA tiles
constexpr int kMsStep = 64;  // columns per load step
constexpr int kMsPad = 4;    // floats of padding per LDS query row

__device__ __forceinline__ int ms_clamp(int x, int lo, int hi) { return min(max(x, lo), hi); }

template <bool BF>
__global__ __launch_bounds__(256) void token_unit_kernel(const void* __restrict__ xv, float* __restrict__ out, int M,
                                                         int P) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;  // wave-uniform: the reduction below runs with all 64 lanes
  const int n = P >> 6;  // 1 .. 16 columns per lane
  float v[16];
  float ss = 0.f;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    v[i] = 0.f;
    if (i < n) {
      const size_t at = (size_t)row * P + i * 64 + lane;
      v[i] = BF ? bf2f(static_cast<const bf16*>(xv)[at]) : static_cast<const float*>(xv)[at];
      ss = fmaf(v[i], v[i], ss);
    }
  }
  ss = wave_sum(ss);
  const float den = fmaxf(sqrtf(ss), 1e-12f);  // F.normalize: x / max(||x||, eps)
#pragma unroll
  for (int i = 0; i < 16; ++i)
    if (i < n) out[(size_t)row * P + i * 64 + lane] = v[i] / den;
}

struct MsFrag {
  f32x4 a[2][4];  // [passage tile][chunk]
};

// rows row0 + r and row0 + 16 + r of the passage (clamped into [0, S): the score is discarded by select)
__device__ __forceinline__ void ms_load(MsFrag& f, const float* __restrict__ d, int P, int S, int row0, int r, int g,
                                        int kb) {
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int row = min(row0 + t * 16 + r, S - 1);
    const float* p = d + (size_t)row * P + kb + 4 * g;
#pragma unroll
    for (int ch = 0; ch < 4; ++ch) f.a[t][ch] = *reinterpret_cast<const f32x4*>(p + 16 * ch);
  }
}

__global__ __launch_bounds__(kMsThreads) void maxsim_kernel(const float* __restrict__ qv,
                                                            const int32_t* __restrict__ lens_q,
                                                            const float* __restrict__ dv,
                                                            const int32_t* __restrict__ lens_d,
                                                            const int32_t* __restrict__ qidx,
                                                            const int32_t* __restrict__ didx,
                                                            float* __restrict__ scores, int Qn, int Dn, int S, int P) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int pair = blockIdx.x;
  const int ldq = P + kMsPad;
  float* wmax = smem + 16 * ldq;  // [wave][query token of the tile]
  // indices and lens are device data: clamped before they form an address
  const int qi = ms_clamp(qidx[pair], 0, Qn - 1), di = ms_clamp(didx[pair], 0, Dn - 1);
  const int lq = ms_clamp(lens_q[qi], 1, S), ld = ms_clamp(lens_d[di], 1, S);
  const float* q = qv + (size_t)qi * S * P;
  const float* d = dv + (size_t)di * S * P;
  const int c4 = P >> 2, KS = P / kMsStep;
  const int nsteps = (ld + kMsRows - 1) / kMsRows;  // steps of 32 passage tokens, split over the waves
  const float ninf = -__builtin_inff();
  const float* qb = smem + r * ldq + 4 * g;
  float sum = 0.f;  // thread 0: the pair's score so far

  for (int i0 = 0; i0 < lq; i0 += 16) {  // trip count uniform over the workgroup
    // query tile -> LDS (token rows past S repeat the last row; tokens >= len_q are not added below)
    for (int i = tid; i < 16 * c4; i += kMsThreads) {
      const int ti = i / c4, cc = i - ti * c4;
      const int row = min(i0 + ti, S - 1);
      *reinterpret_cast<f32x4*>(smem + ti * ldq + cc * 4) = *reinterpret_cast<const f32x4*>(q + (size_t)row * P + cc * 4);
    }
    __syncthreads();

    // the wave's (passage rows, columns) steps form one stream; two fragment buffers take turns and
    // the loads of step i + 1 are issued before the MFMAs of step i
    float m = ninf;  // max over this wave's passage tokens for query token i0 + r
    MsFrag f0, f1;
    int s = wave, ks = 0;
    f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
    if (s < nsteps) ms_load(f0, d, P, S, s * kMsRows, r, g, 0);
    auto stage = [&](const MsFrag& cur, MsFrag& nxt) {
      const bool last = ks + 1 == KS;
      const int ns = last ? s + kMsWaves : s, nks = last ? 0 : ks + 1;
      ms_load(nxt, d, P, S, ns * kMsRows, r, g, nks * kMsStep);  // past the stream's end: row S - 1, unused
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int ch = 0; ch < 4; ++ch) {
        const f32x4 b = *reinterpret_cast<const f32x4*>(qb + ks * kMsStep + 16 * ch);
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int t = 0; t < 2; ++t)
            acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(cur.a[t][ch][j], b[j], acc[t], 0, 0, 0);
      }
      if (last) {  // the rows' dot products are complete: into the running max
#pragma unroll
        for (int t = 0; t < 2; ++t) {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int row = s * kMsRows + t * 16 + g * 4 + e;
            m = fmaxf(m, row < ld ? acc[t][e] : ninf);
          }
          acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
      }
      s = ns;
      ks = nks;
    };
    while (s < nsteps) {  // wave-uniform
      stage(f0, f1);
      if (s < nsteps) stage(f1, f0);
    }
    // the four lane groups of a query token, then the four waves
    m = fmaxf(m, xor16f(m));
    m = fmaxf(m, xor32f(m));
    if (g == 0) wmax[wave * 16 + r] = m;
    __syncthreads();  // also: every read of the query tile is done
    if (tid == 0) {
      const int cnt = min(16, lq - i0);
      for (int i = 0; i < cnt; ++i) {  // increasing token index, left to right
        float v = wmax[i];
#pragma unroll
        for (int w = 1; w < kMsWaves; ++w) v = fmaxf(v, wmax[w * 16 + i]);
        sum += v;
      }
    }
    // the next tile's wmax is written after its barrier, which thread 0 reaches after these reads
  }
  if (tid == 0) scores[pair] = sum;
}

size_t ms_lds_bytes(int P) { return (size_t)(16 * (P + kMsPad) + kMsWaves * 16) * sizeof(float); }

}  // namespace

void token_unit(const void* x, float* out, int M, int P, int is_bf16, hipStream_t stream) {
  ATPU_CHECK(P % 64 == 0 && P >= 64 && P <= 1024, "token_unit: P must be a multiple of 64 in [64, 1024]");
  ATPU_CHECK(M >= 0, "token_unit: M must be >= 0");
  if (M == 0) return;
  ATPU_CHECK(x && out, "token_unit: null tensor");
  if (is_bf16)
    hipLaunchKernelGGL((token_unit_kernel<true>), dim3((M + 3) / 4), dim3(256), 0, stream, x, out, M, P);
  else
    hipLaunchKernelGGL((token_unit_kernel<false>), dim3((M + 3) / 4), dim3(256), 0, stream, x, out, M, P);
  ATPU_HIP_CHECK(hipGetLastError());
}

void maxsim(const float* qv, const int32_t* lens_q, const float* dv, const int32_t* lens_d, const int32_t* qidx,
            const int32_t* didx, float* scores, int n, int Qn, int Dn, int S, int P, hipStream_t stream) {
  ATPU_CHECK(P % 64 == 0 && P >= 64 && P <= 1024, "maxsim: P must be a multiple of 64 in [64, 1024]");
  ATPU_CHECK(S >= 1 && Qn >= 1 && Dn >= 1 && n >= 0, "maxsim: S, Qn and Dn must be >= 1");
  if (n == 0) return;
  ATPU_CHECK(qv && lens_q && dv && lens_d && qidx && didx && scores, "maxsim: null tensor");
  ATPU_CHECK(((reinterpret_cast<uintptr_t>(qv) | reinterpret_cast<uintptr_t>(dv)) & 15) == 0,
             "maxsim: qv and dv must be 16-byte aligned");
  const size_t lds = ms_lds_bytes(P);
  // up to 66.3 KiB of dynamic LDS (P = 1024); the attribute is per device
  ATPU_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&maxsim_kernel),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(maxsim_kernel, dim3(n), dim3(kMsThreads), lds, stream, qv, lens_q, dv, lens_d, qidx, didx, scores,
                     Qn, Dn, S, P);
  ATPU_HIP_CHECK(hipGetLastError());
}

}  // namespace atpu
