// Extractive question answering head: start / end logits of every token of a pair row
// ([CLS] question [SEP] passage [SEP], rerank.hip pair_assemble) and the n best answer spans
// of its passage, in one launch.
//
// Phase 1, logits. On the LayerNorm-folded encoder the last layer leaves raw rows g_j and their
// statistics fin = (rstd_j, rstd_j * mu_j). The span head is linear, so the LayerNorm that would
// finish the rows folds into it (u = gamma * W, su = row sums of u, c = beta . W + b):
//   logit_c[j] = LN(g_j) . W_c + b_c = rstd_j * (g_j . u_c) - (rstd_j mu_j) * su_c + c_c
// and no [B*S, H] tensor is written. Without fin the rows are already normalised:
// logit_c[j] = x_j . u_c + c_c. One workgroup (512 threads, 8 waves) per pair row; wave w takes
// tokens w, w + 8, ..., four at a time (up to 8 x 16 B in flight per lane). A lane owns the
// 16-B column chunks `lane` and `lane + 64` of every row (H <= 1024: at most 128 chunks), so its
// 2 x 16 weights are staged in LDS once per workgroup and then live in registers. Per lane the
// products are summed in column order, the 64 lanes by wave_sum: the order is fixed, there are
// no atomics, a row's bits do not depend on the batch or on the run.
//
// Rows >= len: the row index is clamped to len - 1 (a row the encoder computed) and nothing is
// stored for them; their logits are -inf. len is clamped to [2, S]. No address is formed from
// type_ids; lens only reaches one through that clamp.
//
// Phase 2, spans, in LDS and registers. lo = the first j with type_ids[b, j] == 1 (S when there is
// none), hi = len - 2. Candidates are (i, j), lo <= i <= j <= hi, j - i < max_len, valued
// logit_0[i] + logit_1[j] (a NaN ranks as -inf), ordered by value descending, then id = i * S + j
// ascending (better() of atpu/topk.h). Round r picks the best candidate that comes after round
// r - 1's pick, the scheme of group_topk_kernel: wave w scans the starts lo + w, lo + w + 8, ...,
// its lanes the ends; the wave's best by the butterfly, the 8 waves' bests through LDS in wave
// order. Once a round finds nothing the remaining slots are (-1, -1) with -inf.
//
// own [B, 2] (optional; the OWN instantiations): the window rows of window.hip let a row propose only
// the spans whose start it owns: lo + clamp(own0, 0, S) <= i < lo + clamp(own1, 0, S). Ends, ids, the
// order and the passage-relative output are unchanged. Without own the kernel is the one it was.
#include "atpu/common.h"
#include "atpu/kernels.h"
#include "atpu/topk.h"

namespace atpu {
namespace {

constexpr int kSpanThreads = 512;
constexpr int kSpanWaves = kSpanThreads / kWave;
constexpr int kSpanUnroll = 4;
constexpr int kSpanMaxS = 512;
constexpr int kSpanMaxH = 1024;
constexpr int kSpanNoIdx = 0x7fffffff;

__device__ __forceinline__ void dot8(const u32x4& v, const float (&w0)[8], const float (&w1)[8], float& a0,
                                     float& a1) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float lo = __uint_as_float(v[e] << 16), hi = __uint_as_float(v[e] & 0xffff0000u);
    a0 = fmaf(lo, w0[2 * e], a0);
    a0 = fmaf(hi, w0[2 * e + 1], a0);
    a1 = fmaf(lo, w1[2 * e], a1);
    a1 = fmaf(hi, w1[2 * e + 1], a1);
  }
}

template <bool FIN, bool OWN>
__global__ __launch_bounds__(kSpanThreads) void span_topk_kernel(
    const bf16* __restrict__ x, const float* __restrict__ fin, const float* __restrict__ u,
    const float* __restrict__ su, const float* __restrict__ c, const int32_t* __restrict__ type_ids,
    const int32_t* __restrict__ lens, int32_t* __restrict__ span, float* __restrict__ score, float* __restrict__ null,
    float* __restrict__ logits, const int32_t* __restrict__ own, int S, int H, int max_len, int n) {
  __shared__ __attribute__((aligned(16))) float us[2 * kSpanMaxH];  // u [2][H]
  __shared__ float l0[kSpanMaxS], l1[kSpanMaxS];                    // start / end logits
  __shared__ float redv[2][kSpanWaves];
  __shared__ int redi[2][kSpanWaves];
  __shared__ int lo_w[kSpanWaves];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int lane = tid & (kWave - 1), wave = tid / kWave;
  const int C = H >> 3;                         // 16-B chunks per row: 8 .. 128
  const int len = min(max(lens[b], 2), S);      // device data: clamped before any use
  const float ninf = -__builtin_inff();

  for (int i = tid; i < 2 * H; i += kSpanThreads) us[i] = u[i];
  // first passage position: position j = tid (S <= 512 = threads); a wave's first set lane
  {
    const int t = type_ids[(size_t)b * S + min(tid, S - 1)];
    const unsigned long long m = __ballot(tid < S && t == 1);
    if (lane == 0) lo_w[wave] = m ? wave * kWave + __builtin_ctzll(m) : S;
  }
  __syncthreads();

  // ---- phase 1: this lane's weights, then the wave's tokens
  const bool live0 = lane < C, live1 = lane + kWave < C;
  const int c0 = min(lane, C - 1), c1 = min(lane + kWave, C - 1);
  float w00[8], w01[8], w10[8], w11[8];  // [chunk][class]
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    w00[e] = us[c0 * 8 + e];
    w01[e] = us[H + c0 * 8 + e];
    w10[e] = us[c1 * 8 + e];
    w11[e] = us[H + c1 * 8 + e];
  }
  const float su0 = FIN ? su[0] : 0.f, su1 = FIN ? su[1] : 0.f;
  const float cc0 = c[0], cc1 = c[1];
  const bf16* xb = x + (size_t)b * S * H;
  const float* fb = FIN ? fin + (size_t)b * S * 2 : nullptr;
  const bool two = C > kWave;  // workgroup-uniform: rows of more than 64 chunks
  for (int j0 = wave; j0 < len; j0 += kSpanWaves * kSpanUnroll) {  // wave-uniform trip count
    u32x4 va[kSpanUnroll], vb[kSpanUnroll];
    float2 f[kSpanUnroll];
#pragma unroll
    for (int q = 0; q < kSpanUnroll; ++q) {
      const int jc = min(j0 + q * kSpanWaves, len - 1);  // clamp; the store below is what selects
      const bf16* row = xb + (size_t)jc * H;
      va[q] = *reinterpret_cast<const u32x4*>(row + c0 * 8);
      vb[q] = two ? *reinterpret_cast<const u32x4*>(row + c1 * 8) : u32x4{0u, 0u, 0u, 0u};
      if (FIN) f[q] = *reinterpret_cast<const float2*>(fb + jc * 2);
    }
#pragma unroll
    for (int q = 0; q < kSpanUnroll; ++q) {
      float a0 = 0.f, a1 = 0.f, b0 = 0.f, b1 = 0.f;
      dot8(va[q], w00, w01, a0, a1);
      dot8(vb[q], w10, w11, b0, b1);
      // a chunk this lane does not own is discarded by select, never multiplied by 0
      float d0 = (live0 ? a0 : 0.f) + (live1 ? b0 : 0.f);
      float d1 = (live0 ? a1 : 0.f) + (live1 ? b1 : 0.f);
      d0 = wave_sum(d0);
      d1 = wave_sum(d1);
      const int j = j0 + q * kSpanWaves;
      if (lane == 0 && j < len) {
        l0[j] = FIN ? fmaf(f[q].x, d0, fmaf(-f[q].y, su0, cc0)) : d0 + cc0;
        l1[j] = FIN ? fmaf(f[q].x, d1, fmaf(-f[q].y, su1, cc1)) : d1 + cc1;
      }
    }
  }
  if (tid >= len && tid < S) {
    l0[tid] = ninf;
    l1[tid] = ninf;
  }
  __syncthreads();
  if (logits && tid < S) {
    float* lg = logits + ((size_t)b * S + tid) * 2;
    lg[0] = l0[tid];
    lg[1] = l1[tid];
  }
  if (tid == 0) null[b] = l0[0] + l1[0];

  // ---- phase 2: n rounds of "the best candidate after the previous pick"
  int lo = S;
#pragma unroll
  for (int w = 0; w < kSpanWaves; ++w) lo = min(lo, lo_w[w]);
  const int hi = len - 2;  // lo in [0, S], hi in [0, S - 2]: every LDS index below lies in [0, S)
  // the starts this row may propose: [i_lo, i_hi] inside [lo, hi] (own is device data: clamped)
  const int i_lo = OWN ? lo + min(max(own[2 * b], 0), S) : lo;
  const int i_hi = OWN ? min(hi, lo + min(max(own[2 * b + 1], 0), S) - 1) : hi;
  int32_t* sp = span + (size_t)b * n * 2;
  float* sc = score + (size_t)b * n;
  float pv = __builtin_inff();  // the previous pick: everything comes after (+inf, -1)
  int pi = -1;
  int r = 0;
  for (; r < n; ++r) {
    float bv = ninf;
    int bi = kSpanNoIdx;
    for (int i = i_lo + wave; i <= i_hi; i += kSpanWaves) {  // wave-uniform
      const float a = l0[i];
      const int w = min(max_len, hi - i + 1);
      for (int d = lane; d < w; d += kWave) {
        const int j = i + d;
        float v = a + l1[j];
        v = v != v ? ninf : v;  // a NaN ranks as -inf
        const int id = i * S + j;
        if (better(pv, pi, v, id) && better(v, id, bv, bi)) {
          bv = v;
          bi = id;
        }
      }
    }
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
    if (lane == 0) {
      redv[r & 1][wave] = bv;
      redi[r & 1][wave] = bi;
    }
    __syncthreads();  // one barrier per round: round r + 1 writes the other half of red
    bv = redv[r & 1][0];
    bi = redi[r & 1][0];
#pragma unroll
    for (int w = 1; w < kSpanWaves; ++w) step(redv[r & 1][w], redi[r & 1][w]);
    if (bi == kSpanNoIdx) break;  // workgroup-uniform: every thread reduced the same 8 picks
    if (tid == 0) {
      const int i = bi / S, j = bi - i * S;
      sp[2 * r] = i - lo;
      sp[2 * r + 1] = j - lo;
      sc[r] = bv;
    }
    pv = bv;
    pi = bi;
  }
  // exhausted slots
  for (int q = r + tid; q < n; q += kSpanThreads) {
    sp[2 * q] = -1;
    sp[2 * q + 1] = -1;
    sc[q] = ninf;
  }
}

}  // namespace

void span_topk(const bf16* x, const float* fin, const float* u, const float* su, const float* c,
               const int32_t* type_ids, const int32_t* lens, int32_t* span, float* score, float* null, float* logits,
               int B, int S, int H, int max_len, int n, hipStream_t stream, const int32_t* own) {
  ATPU_CHECK(S >= 4 && S <= kSpanMaxS, "span_topk: S must be in [4, 512]");
  ATPU_CHECK(H % 64 == 0 && H >= 64 && H <= kSpanMaxH, "span_topk: H must be a multiple of 64 in [64, 1024]");
  ATPU_CHECK(n >= 1 && n <= 32, "span_topk: n must be in [1, 32]");
  ATPU_CHECK(max_len >= 1 && max_len <= S, "span_topk: max_len must be in [1, S]");
  ATPU_CHECK(B >= 0, "span_topk: B must be >= 0");
  if (B == 0) return;
  ATPU_CHECK(x && u && su && c && type_ids && lens && span && score && null, "span_topk: null tensor");
  ATPU_CHECK(((reinterpret_cast<uintptr_t>(x) & 15) | (reinterpret_cast<uintptr_t>(fin) & 7) |
              (reinterpret_cast<uintptr_t>(u) & 3)) == 0, "span_topk: x must be 16-byte and fin 8-byte aligned");
#define ATPU_SPAN_LAUNCH(FIN, OWN)                                                                               \
  hipLaunchKernelGGL((span_topk_kernel<FIN, OWN>), dim3(B), dim3(kSpanThreads), 0, stream, x, fin, u, su, c, type_ids, \
                     lens, span, score, null, logits, own, S, H, max_len, n)
  if (fin && own)
    ATPU_SPAN_LAUNCH(true, true);
  else if (fin)
    ATPU_SPAN_LAUNCH(true, false);
  else if (own)
    ATPU_SPAN_LAUNCH(false, true);
  else
    ATPU_SPAN_LAUNCH(false, false);
#undef ATPU_SPAN_LAUNCH
  ATPU_HIP_CHECK(hipGetLastError());
}

}  // namespace atpu
