// Sliding windows over long passages ("atpu-window v1", Python twins: agent_tpu_amd/tokenizer.py
// window_table / window_rows): the window rows of a reader and the fold of their answer spans back
// into one row per (question, passage) pair.
//
// Geometry, in passage tokens without specials. For a pair with nq question tokens (cut at mq and
// S - 3) cap = S - 3 - nq passage tokens fit a row; step = min(doc_stride, cap), h = (cap - step) / 2.
// A passage of T tokens has one window when T <= cap (or cap < 1: an empty passage), else
// ceil((T - cap) / step) + 1, window w starting at a_w = w * step with len_w = min(cap, T - a_w)
// tokens. Window w owns the window-relative start positions [own_lo, own_hi): own_lo = 0 for the
// first window, else h; own_hi = len_w for the last, else step + h. The owned ranges partition
// [0, T), so a span whose start a window owns is a candidate of that window alone.
//
// window_assemble_kernel. The frame of pair_assemble_kernel (rerank.hip): one 64-wide wave per
// window row, four rows per workgroup; position j of the row is a pure function of (j, nq, len_w,
// a_w), a lane reads at most one id of each source row per position and writes ids / type_ids at
// j, j + 64, ...; no LDS, no scan. Every index from device data is clamp-then-select: win_pair into
// [0, Pp), qidx into [0, Q), the lens into [2, S] / [2, L], win_start into [0, max(T - 1, 0)], and
// the token loads clamp their column into the row and discard what a position does not take.
// "First" and "last" are read off the start itself (a_w == 0; a_w + cap >= T), which on the
// table's starts is w == 0 and w == W - 1.
//
// window_best_kernel. The frame and the round scheme of group_topk_kernel: one wave per pair, four
// pairs per workgroup; round r picks the best of the pair's (window row, slot) elements that comes
// after round r - 1's pick in the total order (value desc, flattened index asc; a NaN ranks as
// -inf). The pick's span moves by its row's start to passage-absolute tokens. null = the minimum
// of the rows' null scores, folded in row order by lane 0 (fminf: a NaN operand is skipped).
#include "atpu/common.h"
#include "atpu/kernels.h"
#include "atpu/topk.h"

namespace atpu {
namespace {

constexpr int kNoIdx = 0x7fffffff;

__device__ __forceinline__ int clampi(int x, int lo, int hi) { return min(max(x, lo), hi); }

__global__ __launch_bounds__(256) void window_assemble_kernel(
    const int32_t* __restrict__ ids_q, const int32_t* __restrict__ lens_q, const int32_t* __restrict__ ids_p,
    const int32_t* __restrict__ lens_p, const int32_t* __restrict__ qidx, const int32_t* __restrict__ win_pair,
    const int32_t* __restrict__ win_start, int32_t* __restrict__ ids, int32_t* __restrict__ type_ids,
    int32_t* __restrict__ lens, int32_t* __restrict__ own, int R, int Pp, int Q, int S, int L, int mq, int stride,
    int cls, int sep, int pad) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= R) return;
  // the table, qidx and the lens are device data: clamped before they form an address
  const int p = clampi(win_pair[row], 0, Pp - 1);
  const int q = clampi(qidx[p], 0, Q - 1);
  const int nq = min(min(clampi(lens_q[q], 2, S) - 2, mq), S - 3);  // 0 .. S-3
  const int cap = S - 3 - nq;                                       // 0 .. S-3
  const int T = clampi(lens_p[p], 2, L) - 2;                        // 0 .. L-2
  const int a = clampi(win_start[row], 0, max(T - 1, 0));
  const int step = min(stride, cap);  // stride >= 1 (host)
  const int h = (cap - step) >> 1;
  const int nw = min(cap, T - a);  // 0 only when T == 0 or cap == 0
  const bool first = a == 0, last = a + cap >= T;
  const int32_t* qrow = ids_q + (size_t)q * S;
  const int32_t* prow = ids_p + (size_t)p * L;
  int32_t* out = ids + (size_t)row * S;
  int32_t* tout = type_ids + (size_t)row * S;
  const int sep1 = nq + 1, sep2 = nq + nw + 2;  // sep2 <= S-1
  for (int j = lane; j < S; j += 64) {
    // query token j (1..nq) and passage token a + j - sep1 (a+1 .. a+nw <= T): columns clamped into the rows
    const int32_t tq = qrow[min(j, S - 1)];
    const int32_t tp = prow[clampi(a + j - sep1, 0, L - 1)];
    int32_t v = pad;
    v = j < sep2 ? tp : v;
    v = j <= nq ? tq : v;
    v = (j == sep1 || j == sep2) ? sep : v;
    v = j == 0 ? cls : v;
    out[j] = v;
    tout[j] = (j > sep1 && j <= sep2) ? 1 : 0;
  }
  if (lane == 0) {
    lens[row] = nq + nw + 3;
    own[2 * row] = first ? 0 : h;
    own[2 * row + 1] = last ? nw : step + h;
  }
}

__global__ __launch_bounds__(256) void window_best_kernel(const int32_t* __restrict__ span_w,
                                                          const float* __restrict__ score_w,
                                                          const float* __restrict__ null_w,
                                                          const int32_t* __restrict__ start_w,
                                                          const int32_t* __restrict__ wrow, int32_t* __restrict__ span,
                                                          float* __restrict__ score, float* __restrict__ null, int R,
                                                          int P, int n) {
  const int lane = threadIdx.x & 63;
  const int p = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (p >= P) return;  // wave-uniform: the butterflies below run with all 64 lanes
  // offsets are device data: clamped into [0, R], a decreasing pair is an empty range
  const int r0 = clampi(wrow[p], 0, R);
  const int rows = max(clampi(wrow[p + 1], 0, R) - r0, 0);
  const int len = rows * n;  // R * n < 2^31 (host)
  const float ninf = -__builtin_inff();
  float pv = __builtin_inff();  // the previous pick: everything comes after (+inf, -1)
  int pi = -1;
  for (int r = 0; r < n; ++r) {
    float bv = ninf;
    int bi = kNoIdx;
    for (int base = 0; base < len; base += 64) {  // wave-uniform trip count
      const int i = base + lane;
      float x = score_w[min((size_t)r0 * n + min(i, len - 1), (size_t)R * n - 1)];  // R >= 1 (host), len >= 1 here
      x = x != x ? ninf : x;                                                        // a NaN ranks as -inf
      const int id = i < len ? i : kNoIdx;
      if (id != kNoIdx && better(pv, pi, x, id) && better(x, id, bv, bi)) {
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
    // every lane holds the round's pick; (-inf, kNoIdx): the pair is exhausted, and stays so
    if (lane == 0) {
      const bool got = bi != kNoIdx;
      const size_t e = min((size_t)r0 * n + (got ? bi : 0), (size_t)R * n - 1);  // clamped; `got` selects
      const int a = start_w[e / n];
      const int s0 = span_w[2 * e], s1 = span_w[2 * e + 1];
      const bool real = got && s0 >= 0;  // an exhausted slot of a window row stays (-1, -1)
      span[((size_t)p * n + r) * 2] = real ? s0 + a : -1;
      span[((size_t)p * n + r) * 2 + 1] = real ? s1 + a : -1;
      score[(size_t)p * n + r] = bv;
    }
    pv = bv;
    pi = bi;
  }
  if (lane == 0) {
    float m = __builtin_inff();  // no rows: +inf
    for (int w = 0; w < rows; ++w) m = fminf(m, null_w[min(r0 + w, R - 1)]);
    null[p] = m;
  }
}

}  // namespace

void window_assemble(const int32_t* ids_q, const int32_t* lens_q, const int32_t* ids_p, const int32_t* lens_p,
                     const int32_t* qidx, const int32_t* win_pair, const int32_t* win_start, int32_t* ids,
                     int32_t* type_ids, int32_t* lens, int32_t* own, int R, int Pp, int Q, int S, int L, int mq,
                     int stride, int cls, int sep, int pad, hipStream_t stream) {
  ATPU_CHECK(S >= 4 && L >= 2, "window_assemble: S must be >= 4 and L >= 2");
  ATPU_CHECK(Q >= 1 && Pp >= 1 && mq >= 0, "window_assemble: Q and Pp must be >= 1 and max_query_tokens >= 0");
  ATPU_CHECK(stride >= 1, "window_assemble: doc_stride must be >= 1");
  ATPU_CHECK(ids_q && lens_q && ids_p && lens_p && qidx && win_pair && win_start && ids && type_ids && lens && own,
             "window_assemble: null tensor");
  if (R <= 0) return;
  hipLaunchKernelGGL(window_assemble_kernel, dim3((R + 3) / 4), dim3(256), 0, stream, ids_q, lens_q, ids_p, lens_p,
                     qidx, win_pair, win_start, ids, type_ids, lens, own, R, Pp, Q, S, L, mq, stride, cls, sep, pad);
  ATPU_HIP_CHECK(hipGetLastError());
}

void window_best(const int32_t* span_w, const float* score_w, const float* null_w, const int32_t* start_w,
                 const int32_t* wrow, int32_t* span, float* score, float* null, int R, int P, int n,
                 hipStream_t stream) {
  ATPU_CHECK(n >= 1 && n <= 32, "window_best: n must be in [1, 32]");
  ATPU_CHECK(R >= 1 && (long long)R * n < 0x7fffffffLL, "window_best: R must be >= 1 and R * n < 2^31");
  ATPU_CHECK(span_w && score_w && null_w && start_w && wrow && span && score && null, "window_best: null tensor");
  if (P <= 0) return;
  hipLaunchKernelGGL(window_best_kernel, dim3((P + 3) / 4), dim3(256), 0, stream, span_w, score_w, null_w, start_w,
                     wrow, span, score, null, R, P, n);
  ATPU_HIP_CHECK(hipGetLastError());
}

}  // namespace atpu
