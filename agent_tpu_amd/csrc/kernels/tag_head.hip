// Token classification head: a label and its probability for every text token of a row
// ([CLS] text [SEP]) and the row's grouped entities, in one launch.
//
// Phase 1, logits of the text tokens j in [1, len - 2] (position 0 is [CLS], len - 1 is [SEP]). On
// the LayerNorm-folded encoder the last layer leaves raw rows g_j and their statistics
// fin = (rstd_j, rstd_j * mu_j); the head is linear, so the LayerNorm folds into it (u = gamma * W,
// su = row sums of u, c = beta . W + b):
//   logit_c[j] = rstd_j * (g_j . u_c) - (rstd_j mu_j) * su_c + c_c
// and no [B*S, H] tensor is written. Without fin the rows are already normalised:
// logit_c[j] = x_j . u_c + c_c. One workgroup (512 threads, 8 waves) per row. The dot products run
// on the exact f32 MFMA (v_mfma_f32_16x16x4_f32): a tile is 16 tokens (A operand) by 16 labels
// (B); wave w owns the token tiles w, w + 8, w + 16, w + 24 and, per tile, the accumulators of
// all G = ceil(L / 16) label groups, so a row tile is loaded once. The columns go in
// chunks of 128: u [16 G, 128] is staged through LDS per chunk (34 KB at four groups) and the
// accumulators live across the chunks.
//
// k order of one dot product: within a chunk the columns go in pieces of
// 32; lane (r = lane & 15, g = lane >> 4) loads the 16 bytes x[token r][32 cp + 8 g .. + 7], widens
// the bf16 elements by a 16-bit shift and issues 8 MFMAs, MFMA e taking element e: the hardware's
// k index g stands for column 32 cp + 8 g + e. With one or two label groups, elements 0..3 feed
// accumulator 0 and 4..7 accumulator 1 and the dot product is acc0 + acc1; with three or four
// groups there is one chain per group. Either way a wave has at least two independent
// accumulators per tile (the instruction's dependent latency is 40 cycles against a 32-cycle
// issue), and the order is a function of H and ceil(L / 16) alone. The u image in LDS is
// permuted as in sim_topk_f16.hip: within 32 columns the 16-byte piece 2 g + hf sits at piece
// 4 hf + g, the row stride is 128 + 8 floats.
//
// Token rows >= len are never loaded: the row index is clamped to len - 1 and the result
// discarded by select. Label columns >= L are zeros in LDS and never take part in a max, a sum or
// a store (select, never a multiply). len = clamp(lens[b], 2, S). ids only reaches an address
// (cont) under a range test; label_type / label_begin are indexed by an argmax in [0, L).
//
// Per token, in the 16 lanes that hold its labels: y = argmax in the order of better() (logit
// descending, label ascending, a NaN ranks as -inf, all NaN: label 0); p = 1 / sum_c exp(logit_c -
// max) with __expf, a NaN logit adds 0, a logit equal to the max adds exactly 1 (so infinities
// are defined), an all-NaN token has p = 0. The sums run in label-group order per lane and then
// over the mirror / half-mirror / xor 2 / xor 1 butterfly: fixed, the same in all 16 lanes.
//
// Phase 2, grouping, in LDS; thread j owns position j (S <= 512). t = label_type[y], b =
// label_begin[y]. Mode 2: a continuation token (cont[ids[j]] != 0, j != 1) first takes y of its
// word's head (the nearest earlier non-continuation token) and is not scored.
//   mode 0: every text token with t >= 0 is the record (j - 1, j - 1, y, 1), sum = p.
//   mode 1: token j starts a group when t >= 0 and (j == 1 or t[j-1] != t or b); the group runs
//           until the next start, type change or the end of the text.
//   mode 2: as mode 1 on word heads; a continuation never starts and always extends.
// Records (first, last, type, n) with text-relative positions, ent_sum = the fp32 sum of the n
// probabilities in token order, added by the first token's thread. Groups are numbered by a block
// prefix sum of the start flags; the first E are written, count[b] is the true number, unused
// slots are (-1, -1, -1, 0) with 0.0.
#include "atpu/common.h"
#include "atpu/kernels.h"
#include "atpu/topk.h"

namespace atpu {
namespace {

constexpr int kTagThreads = 512;
constexpr int kTagWaves = kTagThreads / kWave;
constexpr int kTagMaxS = 512;
constexpr int kTagTiles = kTagMaxS / 16 / kTagWaves;  // token tiles per wave: 4
constexpr int kTagKC = 128;                           // columns per staged chunk of u
constexpr int kTagLd = kTagKC + 8;                    // LDS row stride of the u image, floats
constexpr int kTagNoIdx = 0x7fffffff;

template <bool FIN, int G>
__global__ __launch_bounds__(kTagThreads) void tag_entities_kernel(
    const bf16* __restrict__ x, const float* __restrict__ fin, const float* __restrict__ u,
    const float* __restrict__ su, const float* __restrict__ c, const int32_t* __restrict__ lens,
    const int32_t* __restrict__ label_type, const int32_t* __restrict__ label_begin, const int32_t* __restrict__ ids,
    const uint8_t* __restrict__ cont, int32_t* __restrict__ ent, float* __restrict__ ent_sum,
    int32_t* __restrict__ count, int32_t* __restrict__ label_out, float* __restrict__ prob_out,
    float* __restrict__ logits_out, int S, int H, int L, int V, int mode, int E) {
  __shared__ __attribute__((aligned(16))) float us[16 * G * kTagLd];
  __shared__ int ys[kTagMaxS];    // argmax label; phase 2: the label the grouping uses
  __shared__ float ps[kTagMaxS];  // its probability
  __shared__ int ts[kTagMaxS];    // entity type, -1 outside
  __shared__ unsigned char isc[kTagMaxS], st[kTagMaxS];  // continuation / group start
  __shared__ int wcnt[kTagWaves];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int lane = tid & (kWave - 1), wave = __builtin_amdgcn_readfirstlane(tid / kWave);
  const int r = lane & 15, g = lane >> 4;
  const int len = min(max(lens[b], 2), S);  // device data: clamped before any use
  const float ninf = -__builtin_inff();
  const bf16* xb = x + (size_t)b * S * H;

  // ---- phase 1: logits on the MFMA
  constexpr int NA = G <= 2 ? 2 : 1;  // chains per (tile, group): at least two independent per tile
  f32x4 acc[kTagTiles][G][NA];
#pragma unroll
  for (int t = 0; t < kTagTiles; ++t)
#pragma unroll
    for (int q = 0; q < G; ++q)
#pragma unroll
      for (int h = 0; h < NA; ++h) acc[t][q][h] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int kb = 0; kb < H; kb += kTagKC) {
    const int ncp = min(kTagKC, H - kb) >> 5;  // 32-column pieces of this chunk: 4, or 2 in a tail
    // this lane's row pieces of the chunk: in flight while u is staged
    u32x4 xa[kTagTiles][4];
#pragma unroll
    for (int t = 0; t < kTagTiles; ++t) {
      const int j0 = (wave + t * kTagWaves) * 16;
      if (j0 < len) {  // wave-uniform
        const bf16* row = xb + (size_t)min(j0 + r, len - 1) * H + kb + 8 * g;
#pragma unroll
        for (int cp = 0; cp < 4; ++cp)
          xa[t][cp] = *reinterpret_cast<const u32x4*>(row + (cp < ncp ? 32 * cp : 0));
      }
    }
    if (kb) __syncthreads();  // the previous chunk's image has been read
    for (int i = tid; i < 16 * G * (kTagKC / 4); i += kTagThreads) {
      const int lab = i >> 5, cc = i & 31, col = kb + cc * 4;
      f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
      if (lab < L && col < H) v = *reinterpret_cast<const f32x4*>(u + (size_t)lab * H + col);
      const int w = cc & 7, pc = (cc & ~7) + 4 * (w & 1) + (w >> 1);
      *reinterpret_cast<f32x4*>(us + lab * kTagLd + pc * 4) = v;
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < kTagTiles; ++t) {
      const int j0 = (wave + t * kTagWaves) * 16;
      if (j0 < len) {
#pragma unroll
        for (int cp = 0; cp < 4; ++cp) {
          if (cp < ncp) {
#pragma unroll
            for (int hf = 0; hf < 2; ++hf) {
              f32x4 bq[G];
#pragma unroll
              for (int q = 0; q < G; ++q)
                bq[q] = *reinterpret_cast<const f32x4*>(us + (q * 16 + r) * kTagLd + 32 * cp + 16 * hf + 4 * g);
              float a[4];
#pragma unroll
              for (int e = 0; e < 2; ++e) {
                const unsigned v = xa[t][cp][2 * hf + e];
                a[2 * e] = __uint_as_float(v << 16);
                a[2 * e + 1] = __uint_as_float(v & 0xffff0000u);
              }
#pragma unroll
              for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int q = 0; q < G; ++q)
                  acc[t][q][hf % NA] =
                      __builtin_amdgcn_mfma_f32_16x16x4f32(a[e], bq[q][e], acc[t][q][hf % NA], 0, 0, 0);
            }
          }
        }
      }
    }
  }

  // logits_out of every position that is not a text token; the text tokens follow below
  if (logits_out)
    for (int i = tid; i < S * L; i += kTagThreads) {
      const int j = i / L;
      if (j < 1 || j > len - 2) logits_out[(size_t)b * S * L + i] = ninf;
    }

  // ---- per token: the accumulator of lane (r, g) holds label q * 16 + r of token j0 + 4 g + e
  float suq[G], cq[G];
#pragma unroll
  for (int q = 0; q < G; ++q) {
    const int lab = min(q * 16 + r, L - 1);
    suq[q] = FIN ? su[lab] : 0.f;
    cq[q] = c[lab];
  }
#pragma unroll
  for (int t = 0; t < kTagTiles; ++t) {
    const int j0 = (wave + t * kTagWaves) * 16;
    if (j0 < len) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int j = j0 + 4 * g + e;
        const bool text = j >= 1 && j <= len - 2;
        float2 f = float2{0.f, 0.f};
        if (FIN) f = *reinterpret_cast<const float2*>(fin + ((size_t)b * S + min(j, len - 1)) * 2);
        float lg[G];
        float bv = ninf;
        int bi = kTagNoIdx;
#pragma unroll
        for (int q = 0; q < G; ++q) {
          const float d = NA == 2 ? acc[t][q][0][e] + acc[t][q][NA - 1][e] : acc[t][q][0][e];
          lg[q] = FIN ? fmaf(f.x, d, fmaf(-f.y, suq[q], cq[q])) : d + cq[q];
          const int lab = q * 16 + r;
          const bool ok = lab < L;
          const float v = (ok && lg[q] == lg[q]) ? lg[q] : ninf;  // a NaN ranks as -inf
          const int id = ok ? lab : kTagNoIdx;
          if (better(v, id, bv, bi)) {
            bv = v;
            bi = id;
          }
        }
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
        float s = 0.f;
#pragma unroll
        for (int q = 0; q < G; ++q) {
          const bool ok = q * 16 + r < L && lg[q] == lg[q];
          const float ex = lg[q] == bv ? 1.f : __expf(lg[q] - bv);
          s += ok ? ex : 0.f;
        }
        s += dppf<kDppMirror>(s);
        s += dppf<kDppHalfMirror>(s);
        s += dppf<kDppXor2>(s);
        s += dppf<kDppXor1>(s);
        if (text) {
          if (r == 0) {
            ys[j] = bi;
            ps[j] = s > 0.f ? 1.f / s : 0.f;  // all NaN: 0
          }
          if (logits_out) {
#pragma unroll
            for (int q = 0; q < G; ++q)
              if (q * 16 + r < L) logits_out[((size_t)b * S + j) * L + q * 16 + r] = lg[q];
          }
        }
      }
    }
  }
  __syncthreads();

  // ---- phase 2: thread j owns position j
  const int j = tid;
  const bool text = j >= 1 && j <= len - 2;
  if (j < S) {
    if (label_out) label_out[(size_t)b * S + j] = text ? ys[j] : -1;
    if (prob_out) prob_out[(size_t)b * S + j] = text ? ps[j] : 0.f;
  }
  bool co = false;
  if (mode == 2 && text && j != 1) {
    const int id = ids[(size_t)b * S + j];
    if (id >= 0 && id < V) co = cont[id] != 0;  // out of range: not a continuation, no load
  }
  if (j < kTagMaxS) isc[j] = co;
  __syncthreads();
  int y = 0;
  if (text) {
    int h = j;
    while (h > 1 && isc[h]) --h;  // token 1 is never a continuation
    y = ys[h];
  }
  __syncthreads();  // every head's own label has been read
  int ty = -1;
  bool bg = false;
  if (text) {
    ys[j] = y;
    ty = label_type[y];
    bg = label_begin[y] != 0;
  }
  ts[j] = ty;
  __syncthreads();
  bool start = text && ty >= 0;
  if (mode != 0) start = start && !co && (j == 1 || ts[max(j - 1, 0)] != ty || bg);
  st[j] = start;
  __syncthreads();
  int last = j, n = 0;
  float sum = 0.f;
  if (start) {
    n = 1;
    sum = ps[j];
    if (mode != 0)
      for (int k = j + 1; k <= len - 2 && !st[k] && ts[k] == ty; ++k) {
        last = k;
        if (!isc[k]) {
          sum += ps[k];
          ++n;
        }
      }
  }
  const unsigned long long m = __ballot(start);
  if (lane == 0) wcnt[wave] = __popcll(m);
  __syncthreads();
  int idx = __popcll(m & ((1ull << lane) - 1ull)), total = 0;
#pragma unroll
  for (int w = 0; w < kTagWaves; ++w) {
    idx += w < wave ? wcnt[w] : 0;
    total += wcnt[w];
  }
  int32_t* eb = ent + (size_t)b * E * 4;
  float* sb = ent_sum + (size_t)b * E;
  if (start && idx < E) {
    eb[4 * idx] = j - 1;
    eb[4 * idx + 1] = last - 1;
    eb[4 * idx + 2] = mode == 0 ? y : ty;
    eb[4 * idx + 3] = n;
    sb[idx] = sum;
  }
  for (int q = total + tid; q < E; q += kTagThreads) {
    eb[4 * q] = -1;
    eb[4 * q + 1] = -1;
    eb[4 * q + 2] = -1;
    eb[4 * q + 3] = 0;
    sb[q] = 0.f;
  }
  if (tid == 0) count[b] = total;
}

template <bool FIN>
void tag_launch(int G, int B, hipStream_t stream, const bf16* x, const float* fin, const float* u, const float* su,
                const float* c, const int32_t* lens, const int32_t* label_type, const int32_t* label_begin,
                const int32_t* ids, const uint8_t* cont, int32_t* ent, float* ent_sum, int32_t* count,
                int32_t* label_out, float* prob_out, float* logits_out, int S, int H, int L, int V, int mode, int E) {
#define ATPU_TAG_CASE(GG)                                                                                          \
  case GG:                                                                                                         \
    hipLaunchKernelGGL((tag_entities_kernel<FIN, GG>), dim3(B), dim3(kTagThreads), 0, stream, x, fin, u, su, c,    \
                       lens, label_type, label_begin, ids, cont, ent, ent_sum, count, label_out, prob_out,         \
                       logits_out, S, H, L, V, mode, E);                                                           \
    break;
  switch (G) {
    ATPU_TAG_CASE(1)
    ATPU_TAG_CASE(2)
    ATPU_TAG_CASE(3)
    ATPU_TAG_CASE(4)
  }
#undef ATPU_TAG_CASE
}

}  // namespace

void tag_entities(const bf16* x, const float* fin, const float* u, const float* su, const float* c,
                  const int32_t* lens, const int32_t* label_type, const int32_t* label_begin, const int32_t* ids,
                  const uint8_t* cont, int32_t* ent, float* ent_sum, int32_t* count, int32_t* label_out,
                  float* prob_out, float* logits_out, int B, int S, int H, int L, int V, int mode, int E,
                  hipStream_t stream) {
  ATPU_CHECK(S >= 3 && S <= kTagMaxS, "tag_entities: S must be in [3, 512]");
  ATPU_CHECK(H % 64 == 0 && H >= 64 && H <= 1024, "tag_entities: H must be a multiple of 64 in [64, 1024]");
  ATPU_CHECK(L >= 1 && L <= 64, "tag_entities: L must be in [1, 64]");
  ATPU_CHECK(E >= 1 && E <= 512, "tag_entities: E must be in [1, 512]");
  ATPU_CHECK(mode >= 0 && mode <= 2, "tag_entities: mode must be 0, 1 or 2");
  ATPU_CHECK(B >= 0, "tag_entities: B must be >= 0");
  if (B == 0) return;
  ATPU_CHECK(x && u && c && lens && label_type && label_begin && ent && ent_sum && count,
             "tag_entities: null tensor");
  ATPU_CHECK(!fin || su, "tag_entities: fin needs su");
  ATPU_CHECK(mode != 2 || (ids && cont && V >= 1), "tag_entities: mode 2 needs ids and cont");
  ATPU_CHECK(((reinterpret_cast<uintptr_t>(x) & 15) | (reinterpret_cast<uintptr_t>(fin) & 7) |
              (reinterpret_cast<uintptr_t>(u) & 15)) == 0,
             "tag_entities: x and u must be 16-byte and fin 8-byte aligned");
  const int G = (L + 15) / 16;
  if (fin)
    tag_launch<true>(G, B, stream, x, fin, u, su, c, lens, label_type, label_begin, ids, cont, ent, ent_sum, count,
                     label_out, prob_out, logits_out, S, H, L, V, mode, E);
  else
    tag_launch<false>(G, B, stream, x, fin, u, su, c, lens, label_type, label_begin, ids, cont, ent, ent_sum, count,
                      label_out, prob_out, logits_out, S, H, L, V, mode, E);
  ATPU_HIP_CHECK(hipGetLastError());
}

}  // namespace atpu
