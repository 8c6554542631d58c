// Masked-language-model head: the rows of the mask positions (mask_gather) and the vocabulary
// product with a fused log-sum-exp and top-k (vocab_topk_partial + vocab_topk_merge). No [R, V]
// tensor is written unless a test asks for it (logits_out).
//
// mask_gather_kernel. One 64-wide wave per mask slot r, four slots per workgroup. b = mrow[r],
// o = mord[r], p = pos[b, o]; the slot is valid when 0 <= b < B, 0 <= o < M and 0 <= p < S. The row
// b * S + p of x (every index clamped first, the result selected) goes to xm[r]: copied when x holds
// normalised rows, or finished with the last LayerNorm when fin = (rstd, rstd * mu) is given:
// y = (x * rstd - rstd mu) * gamma + beta in fp32 (one fma, one fma), rounded once to bf16. An
// invalid slot writes zeros and valid[r] = 0.
//
// vocab_topk_partial_kernel<KM, LG> (LG: the form that also writes logits_out; the workspace is the
// [R, P, k] list entries followed by the [R, P] (max, sum) pairs): sim_topk_f16.hip's workgroup with bf16 in place of fp16, one
// shape for every R: 4 waves, a tile of 16 slots (B operand, fp32, the permuted LDS image of that
// file) against one vocabulary split; a wave streams pairs of 16-token tiles of E (A operand, bf16
// widened to fp32 in registers, which is exact) through v_mfma_f32_16x16x4_f32.
//
// Batch invariance (the bits of a slot's tok / logit / prob / lse do not depend on R, on the slot's
// index or on the other slots of the launch):
//   * logit[r, v]: one fp32 accumulator per (slot, token); the k order is that of sim_topk_f16.hip,
//     a function of H alone (chunks of 32 columns, MFMA j of a chunk takes element j of every lane
//     group's 8); the bias is added once, after the chain. An MFMA column depends on no other
//     column, so neither the slot's place in its tile nor its neighbours matter.
//   * the top-k is exact in the total order (logit desc, token asc): any partition gives the same.
//   * lse: the partition of the vocabulary is a function of V alone. A split is kVocSteps = 16
//     steps of 32 tokens (P = ceil(ceil(V / 32) / 16) splits; never from R or the CU count), step s
//     of a split belongs to wave s % 4, and lane group g of that wave holds tokens 16 t + 4 g + e
//     (t = 0, 1; e = 0 .. 3) of the step for every slot. Each (wave, lane group) keeps one running
//     (max, sum) per slot: a step's 8 values raise the max, the sum is rescaled once and the 8
//     exponentials are added in (t, e) order. At the end of the split the 16 pairs of a slot are
//     combined by one thread: the max over them (exact in any order), then the rescaled sums added
//     in (wave, g) order. vocab_topk_merge combines the P split pairs of a slot the same way: the
//     max, then lane l adds the rescaled sums of splits l, l + 64, ... in order and the 64 lane
//     sums meet in the fixed xor butterfly of wave_sum. Depth of the additions a value can pass:
//     9 per step x 4 steps of a wave + 16 + ceil(P / 64) + 6.
//   A NaN logit ranks and returns as -inf and adds 0 to the sum; a term equal to the maximum adds
//   exactly 1.
//
// Tokens past V: the row index is clamped to V - 1 (for E and for the bias) and the value discarded
// by select: nothing outside E[0:V] and bias[0:V] is read. Slots past R repeat the last slot and are
// not written.
//
// vocab_topk_merge_kernel: one wave per slot. The slot's P * k partial entries are searched k times
// (the round scheme of window_best_kernel: round n takes the best entry after round n - 1's pick
// in the total order; tokens are distinct). prob = exp(logit - lse), with lse_in[r] when given.
// Past the last token (-1, -inf, 0). A slot with valid[r] == 0 returns (-1, -inf, 0) and lse = 0.
#include "atpu/common.h"
#include "atpu/kernels.h"
#include "atpu/topk.h"

namespace atpu {
namespace {

constexpr int kVocRows = 32;    // tokens per wave step: two 16-row MFMA tiles
constexpr int kVocSteps = 16;   // steps per vocabulary split (512 tokens)
constexpr int kVocStep = 128;   // columns per full load step
constexpr int kVocPad = 8;      // floats of padding per LDS slot row
constexpr int kVocWaves = 4;
constexpr int kVocTile = 16;    // slots per workgroup
constexpr int kVocLists = 4 * kVocWaves;
constexpr int kNoTok = 0x7fffffff;

__device__ __forceinline__ int clampi(int x, int lo, int hi) { return min(max(x, lo), hi); }

__global__ __launch_bounds__(256) void mask_gather_kernel(const bf16* __restrict__ x, const float* __restrict__ fin,
                                                          const float* __restrict__ gamma,
                                                          const float* __restrict__ beta,
                                                          const int32_t* __restrict__ pos,
                                                          const int32_t* __restrict__ mrow,
                                                          const int32_t* __restrict__ mord, bf16* __restrict__ xm,
                                                          int32_t* __restrict__ valid, int R, int B, int S, int M,
                                                          int H) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= R) return;
  const int b = mrow[r], o = mord[r];
  const int bc = clampi(b, 0, B - 1), oc = clampi(o, 0, M - 1);
  const int p = pos[(size_t)bc * M + oc];
  const bool ok = b == bc && o == oc && p >= 0 && p < S;
  const size_t row = (size_t)bc * S + clampi(p, 0, S - 1);
  float rstd = 1.f, rm = 0.f;
  if (fin) {
    rstd = fin[2 * row];
    rm = fin[2 * row + 1];
  }
  for (int c = lane; c < H / 8; c += 64) {
    const bf16x8 v = *reinterpret_cast<const bf16x8*>(x + row * H + 8 * c);
    bf16x8 y;
    if (fin) {
#pragma unroll
      for (int e = 0; e < 8; ++e) y[e] = f2bf(fmaf(fmaf(bf2f(v[e]), rstd, -rm), gamma[8 * c + e], beta[8 * c + e]));
    } else {
      y = v;
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) y[e] = ok ? y[e] : f2bf(0.f);
    *reinterpret_cast<bf16x8*>(xm + (size_t)r * H + 8 * c) = y;
  }
  if (lane == 0) valid[r] = ok ? 1 : 0;
}

struct VocFrag {
  bf16x8 a[2][4];  // [token tile][chunk of 32 columns]
};

__device__ __forceinline__ void voc_load(VocFrag& f, const bf16* __restrict__ E, int H, int V, int row0, int r, int g,
                                         int kb) {
  const int hi = kb + kVocStep <= H ? 64 : 0;  // a two-chunk tail step loads its chunks twice
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int row = min(row0 + t * 16 + r, V - 1);  // clamp, the value is discarded by select
    const bf16* p = E + (size_t)row * H + kb + 8 * g;
    f.a[t][0] = *reinterpret_cast<const bf16x8*>(p);
    f.a[t][1] = *reinterpret_cast<const bf16x8*>(p + 32);
    f.a[t][2] = *reinterpret_cast<const bf16x8*>(p + hi);
    f.a[t][3] = *reinterpret_cast<const bf16x8*>(p + hi + 32);
  }
}

// exp(x - m) for the running sums: -inf adds 0, a term equal to the maximum exactly 1
__device__ __forceinline__ float voc_exp(float x, float m) {
  const float e = x == m ? 1.f : expf(x - m);
  return x == -__builtin_inff() ? 0.f : e;
}

template <int KM, bool LG>
__global__ __launch_bounds__(kVocWaves* kWave) void vocab_topk_partial_kernel(
    const float* __restrict__ t, const bf16* __restrict__ E, const float* __restrict__ bias, float2* __restrict__ ws,
    float* __restrict__ logits_out, int R, int V, int H, int k) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int NW = kVocWaves, L = kVocLists;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 15, g = lane >> 4;
  const int split = blockIdx.x, q0 = blockIdx.y * kVocTile, P = gridDim.x;
  const int ldq = H + kVocPad;
  const float ninf = -__builtin_inff();

  // slot tile -> LDS, permuted (sim_topk_f16.hip's header); slots past R repeat the last slot
  const int c4 = H >> 2;
  for (int i = tid; i < kVocTile * c4; i += NW * kWave) {
    const int qi = i / c4, cc = i - qi * c4;
    const int qr = min(q0 + qi, R - 1);
    const int u = cc & 7, pc = (cc & ~7) + 4 * (u & 1) + (u >> 1);
    *reinterpret_cast<f32x4*>(smem + qi * ldq + pc * 4) = *reinterpret_cast<const f32x4*>(t + (size_t)qr * H + cc * 4);
  }
  __syncthreads();

  float tv[KM];
  int ti[KM];
#pragma unroll
  for (int e = 0; e < KM; ++e) {
    tv[e] = ninf;
    ti[e] = kNoTok;
  }
  float lm = ninf, ls = 0.f;  // this (wave, lane group)'s running (max, sum) of slot r

  const int nsteps = (V + kVocRows - 1) / kVocRows;
  const int s_lo = split * kVocSteps, s_hi = min(s_lo + kVocSteps, nsteps);
  const int KS = (H + kVocStep - 1) / kVocStep;
  const float* qb = smem + r * ldq + 4 * g;
  const int slot = q0 + r;

  VocFrag f0, f1;
  int s = s_lo + wave, ks = 0;
  f32x4 acc[2];
  acc[0] = f32x4{0.f, 0.f, 0.f, 0.f};
  acc[1] = f32x4{0.f, 0.f, 0.f, 0.f};
  if (s < s_hi) voc_load(f0, E, H, V, s * kVocRows, r, g, 0);
  auto stage = [&](const VocFrag& cur, VocFrag& nxt) {
    const bool last = ks + 1 == KS;
    const int ns = last ? s + NW : s, nks = last ? 0 : ks + 1;
    const int kb = ks * kVocStep;
    float bs[2][4];
#pragma unroll
    for (int tt = 0; tt < 2; ++tt)
#pragma unroll
      for (int e = 0; e < 4; ++e) bs[tt][e] = bias[min(s * kVocRows + tt * 16 + g * 4 + e, V - 1)];
    __builtin_amdgcn_sched_barrier(0);
    voc_load(nxt, E, H, V, ns * kVocRows, r, g, nks * kVocStep);
    __builtin_amdgcn_sched_barrier(0);
    auto chunk = [&](int cp) {
#pragma unroll
      for (int hf = 0; hf < 2; ++hf) {
        const f32x4 b = *reinterpret_cast<const f32x4*>(qb + kb + 32 * cp + 16 * hf);
        float a[2][4];
#pragma unroll
        for (int tt = 0; tt < 2; ++tt)
#pragma unroll
          for (int j = 0; j < 4; ++j) a[tt][j] = bf2f(cur.a[tt][cp][4 * hf + j]);
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int tt = 0; tt < 2; ++tt)
            acc[tt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[tt][j], b[j], acc[tt], 0, 0, 0);
      }
    };
    chunk(0);
    chunk(1);
    if (kb + kVocStep <= H) {
      chunk(2);
      chunk(3);
    }
    if (last) {  // the tokens' logits are complete: bias, then the lists and the running (max, sum)
      float xv[2][4];
      float mx = lm;
#pragma unroll
      for (int tt = 0; tt < 2; ++tt)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int row = s * kVocRows + tt * 16 + g * 4 + e;
          const bool live = row < V;
          const float lg = acc[tt][e] + bs[tt][e];
          if constexpr (LG) {
            if (live && slot < R) logits_out[(size_t)slot * V + row] = lg;
          }
          const float v = (live && lg == lg) ? lg : ninf;  // a NaN ranks as -inf
          const int id = live ? row : kNoTok;
          xv[tt][e] = v;
          mx = fmaxf(mx, v);
          if (__ballot(better(v, id, tv[KM - 1], ti[KM - 1])) != 0) list_insert<KM>(tv, ti, v, id);
        }
      ls *= voc_exp(lm, mx);
#pragma unroll
      for (int tt = 0; tt < 2; ++tt)
#pragma unroll
        for (int e = 0; e < 4; ++e) ls += voc_exp(xv[tt][e], mx);
      lm = mx;
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

  // the L lists and (max, sum) pairs of every slot -> LDS (the lists over the slot tile, which is
  // no longer read; the pairs behind both), then L lanes per slot pop the best head k times
  __syncthreads();
  float2* ml = reinterpret_cast<float2*>(smem);
  float2* pl = reinterpret_cast<float2*>(smem) + max(kVocTile * (H + kVocPad) / 2, kVocTile * kVocLists * KM);
  {
    float2* dst = ml + (r * L + wave * 4 + g) * KM;
#pragma unroll
    for (int e = 0; e < KM; ++e) dst[e] = float2{tv[e], __int_as_float(ti[e])};
    pl[r * L + wave * 4 + g] = float2{lm, ls};
  }
  __syncthreads();
  if (tid < kVocTile && q0 + tid < R) {
    float m = ninf;
    for (int i = 0; i < L; ++i) m = fmaxf(m, pl[tid * L + i].x);
    float sum = 0.f;
    for (int i = 0; i < L; ++i) {
      const float2 pr = pl[tid * L + i];
      sum += pr.y * voc_exp(pr.x, m);
    }
    ws[(size_t)R * P * k + (size_t)(q0 + tid) * P + split] = float2{m, sum};  // the pairs follow the lists
  }
  const int li = lane & (L - 1);
  const int qi = wave * (kWave / L) + lane / L;
  const float2* src = ml + (qi * L + li) * KM;
  int pos = 0;
  for (int n = 0; n < k; ++n) {
    const float2 hd = src[min(pos, KM - 1)];
    const float hv = pos < KM ? hd.x : ninf;
    const int hi = pos < KM ? __float_as_int(hd.y) : kNoTok;
    float bv = hv;
    int bi = hi;
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
    if (hi == bi && bi != kNoTok) ++pos;  // tokens are distinct: exactly one owner
    if (li == 0 && q0 + qi < R) ws[((size_t)(q0 + qi) * P + split) * k + n] = float2{bv, __int_as_float(bi)};
  }
}

__global__ __launch_bounds__(256) void vocab_topk_merge_kernel(const float2* __restrict__ ws,
                                                               const float2* __restrict__ wl,
                                                               const int32_t* __restrict__ valid,
                                                               const float* __restrict__ lse_in,
                                                               int32_t* __restrict__ tok, float* __restrict__ logit,
                                                               float* __restrict__ prob, float* __restrict__ lse,
                                                               int R, int P, int k) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= R) return;  // wave-uniform: the butterflies below run with all 64 lanes
  const float ninf = -__builtin_inff();
  const bool ok = valid == nullptr || valid[r] != 0;
  // log-sum-exp: the max over the splits, then the rescaled sums in the fixed order of the header
  float m = ninf;
  for (int p = lane; p < P; p += 64) m = fmaxf(m, wl[(size_t)r * P + p].x);
  m = wave_max(m);
  float sum = 0.f;
  for (int p = lane; p < P; p += 64) {
    const float2 pr = wl[(size_t)r * P + p];
    sum += pr.y * voc_exp(pr.x, m);
  }
  sum = wave_sum(sum);
  const float own = m == ninf ? ninf : m + logf(sum);
  const float norm = lse_in != nullptr ? lse_in[r] : own;
  if (lane == 0) lse[r] = ok ? own : 0.f;

  const int len = P * k;
  const float2* src = ws + (size_t)r * len;
  float pv = __builtin_inff();  // the previous pick: everything comes after (+inf, -1)
  int pi = -1;
  for (int n = 0; n < k; ++n) {
    float bv = ninf;
    int bi = kNoTok;
    for (int base = 0; base < len; base += 64) {  // wave-uniform trip count
      const int i = base + lane;
      const float2 e = src[min(i, len - 1)];
      const float x = e.x;
      const int id = i < len ? __float_as_int(e.y) : kNoTok;
      if (id != kNoTok && better(pv, pi, x, id) && better(x, id, bv, bi)) {
        bv = x;
        bi = id;
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
      const bool got = ok && bi != kNoTok;
      tok[(size_t)r * k + n] = got ? bi : -1;
      logit[(size_t)r * k + n] = got ? bv : ninf;
      prob[(size_t)r * k + n] = (got && bv != ninf) ? expf(bv - norm) : 0.f;
    }
    pv = bv;
    pi = bi;
  }
}

size_t voc_lds_bytes(int H, int KM) {
  const size_t qbytes = (size_t)kVocTile * (H + kVocPad) * sizeof(float);
  const size_t mbytes = (size_t)kVocTile * kVocLists * KM * sizeof(float2);
  return qbytes > mbytes ? qbytes : mbytes;
}

template <int KM>
void voc_launch(const float* t, const bf16* E, const float* bias, float2* ws, float* logits_out, int R, int V, int H,
                int k, int P, hipStream_t stream) {
  // the lists (over the slot tile), then the (max, sum) pairs: the kernel recomputes this offset
  const size_t lds = voc_lds_bytes(H, KM) + (size_t)kVocTile * kVocLists * sizeof(float2);
  // up to 66 KiB of dynamic LDS (KM = 32); the attribute is per device
  if (logits_out) {
    ATPU_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&vocab_topk_partial_kernel<KM, true>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL((vocab_topk_partial_kernel<KM, true>), dim3(P, (R + kVocTile - 1) / kVocTile),
                       dim3(kVocWaves * kWave), lds, stream, t, E, bias, ws, logits_out, R, V, H, k);
  } else {
    ATPU_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&vocab_topk_partial_kernel<KM, false>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL((vocab_topk_partial_kernel<KM, false>), dim3(P, (R + kVocTile - 1) / kVocTile),
                       dim3(kVocWaves * kWave), lds, stream, t, E, bias, ws, logits_out, R, V, H, k);
  }
  ATPU_HIP_CHECK(hipGetLastError());
}

}  // namespace

void mask_gather(const bf16* x, const float* fin, const float* gamma, const float* beta, const int32_t* pos,
                 const int32_t* mrow, const int32_t* mord, bf16* xm, int32_t* valid, int R, int B, int S, int M, int H,
                 hipStream_t stream) {
  ATPU_CHECK(S >= 1 && M >= 1 && M <= 16, "mask_gather: S must be >= 1 and M in [1, 16]");
  ATPU_CHECK(H % 64 == 0 && H >= 64 && H <= 1024, "mask_gather: H must be a multiple of 64 in [64, 1024]");
  if (R <= 0) return;
  ATPU_CHECK(B >= 1, "mask_gather: B must be >= 1");
  ATPU_CHECK(x && pos && mrow && mord && xm && valid, "mask_gather: null tensor");
  ATPU_CHECK(!fin || (gamma && beta), "mask_gather: fin needs gamma and beta");
  ATPU_CHECK(((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(xm)) & 15) == 0 &&
                 (reinterpret_cast<uintptr_t>(fin) & 7) == 0,
             "mask_gather: x and xm must be 16-byte and fin 8-byte aligned");
  hipLaunchKernelGGL(mask_gather_kernel, dim3((R + 3) / 4), dim3(256), 0, stream, x, fin, gamma, beta, pos, mrow,
                     mord, xm, valid, R, B, S, M, H);
  ATPU_HIP_CHECK(hipGetLastError());
}

int vocab_topk_splits(int V) {
  const int nsteps = (V + kVocRows - 1) / kVocRows;
  return (nsteps + kVocSteps - 1) / kVocSteps;
}

void vocab_topk_partial(const float* t, const bf16* E, const float* bias, float* ws, float* logits_out, int R, int V,
                        int H, int k, hipStream_t stream) {
  ATPU_CHECK(V >= 1 && V < 0x7fffffff - 1024, "vocab_topk: V must be in [1, 2^31 - 1024)");
  ATPU_CHECK(H % 64 == 0 && H >= 64 && H <= 1024, "vocab_topk: H must be a multiple of 64 in [64, 1024]");
  ATPU_CHECK(k >= 1 && k <= 32, "vocab_topk: k must be in [1, 32]");
  if (R <= 0) return;
  ATPU_CHECK(t && E && bias && ws, "vocab_topk: null tensor");
  ATPU_CHECK(((reinterpret_cast<uintptr_t>(t) | reinterpret_cast<uintptr_t>(E)) & 15) == 0 &&
                 (reinterpret_cast<uintptr_t>(ws) & 7) == 0 &&
                 ((reinterpret_cast<uintptr_t>(bias) | reinterpret_cast<uintptr_t>(logits_out)) & 3) == 0,
             "vocab_topk: t and E must be 16-byte, the workspace 8-byte, bias and logits_out 4-byte aligned");
  const int P = vocab_topk_splits(V);
  ATPU_CHECK((R + kVocTile - 1) / kVocTile <= 65535, "vocab_topk: R must be <= 16 * 65535");
  float2* w = reinterpret_cast<float2*>(ws);
  if (k <= 8) voc_launch<8>(t, E, bias, w, logits_out, R, V, H, k, P, stream);
  else if (k <= 16) voc_launch<16>(t, E, bias, w, logits_out, R, V, H, k, P, stream);
  else voc_launch<32>(t, E, bias, w, logits_out, R, V, H, k, P, stream);
}

void vocab_topk_merge(const float* ws, const int32_t* valid, const float* lse_in, int32_t* tok, float* logit,
                      float* prob, float* lse, int R, int V, int k, hipStream_t stream) {
  ATPU_CHECK(V >= 1 && k >= 1 && k <= 32, "vocab_topk_merge: V must be >= 1 and k in [1, 32]");
  if (R <= 0) return;
  ATPU_CHECK(ws && tok && logit && prob && lse, "vocab_topk_merge: null tensor");
  const int P = vocab_topk_splits(V);
  ATPU_CHECK((long long)P * k < 0x7fffffffLL, "vocab_topk_merge: P * k must be < 2^31");
  hipLaunchKernelGGL(vocab_topk_merge_kernel, dim3((R + 3) / 4), dim3(256), 0, stream,
                     reinterpret_cast<const float2*>(ws), reinterpret_cast<const float2*>(ws) + (size_t)R * P * k, valid,
                     lse_in, tok, logit, prob, lse, R, P, k);
  ATPU_HIP_CHECK(hipGetLastError());
}

}  // namespace atpu
