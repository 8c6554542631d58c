// Cross-encoder re-ranker front and back end: pair rows from single-segment rows, and the
// per-query top-k of the pair scores.
//
// pair_assemble_kernel ("atpu-pair v1", Python twin: agent_tpu_amd/tokenizer.py pair_rows). The
// frame is the tokenizers': one 64-wide wave per passage row, four rows per workgroup. Position j
// of the output row is a pure function of (j, nq, np): a special id, a token of the query row, a
// token of the passage row, or padding, so a lane reads at most one id of each source row and
// writes ids / type_ids at j, j + 64, ...: coalesced row reads and writes, no LDS, no scan.
// Every data-dependent index is clamp-then-select, as in tokenize_wp.hip: qidx is clamped into
// [0, Q), both lens into [2, S], and the token loads clamp their column into the row and discard
// what a position does not take. No address relies on a lane being inactive.
//
// group_topk_kernel. One wave per query, four queries per workgroup. Round n picks the best
// element that comes after round n-1's pick in the total order (value desc, index asc; better()
// of atpu/topk.h): each lane scans its elements i = lane, lane + 64, ... of the group, the wave
// takes the best of the 64 by the butterfly of sim_topk_merge_kernel. Cost: k * ceil(len / 64)
// 4-byte loads per lane, all L1/L2 hits after the first round: a re-ranker's groups are the
// candidate lists of a search (tens to hundreds of rows), so that is k to a few k loads per
// lane, fewer instructions than keeping k-entry sorted lists per lane (list_insert is k
// compare-swaps per ELEMENT, 64 * k list slots for a 32-row group) and no template over k.
// A group of any length, 0 included, takes the same loop; the list never leaves registers.
#include "atpu/common.h"
#include "atpu/kernels.h"
#include "atpu/topk.h"

namespace atpu {
namespace {

constexpr int kNoIdx = 0x7fffffff;

__device__ __forceinline__ int clampi(int x, int lo, int hi) { return min(max(x, lo), hi); }

__global__ __launch_bounds__(256) void pair_assemble_kernel(const int32_t* __restrict__ ids_q,
                                                            const int32_t* __restrict__ lens_q,
                                                            const int32_t* __restrict__ ids_p,
                                                            const int32_t* __restrict__ lens_p,
                                                            const int32_t* __restrict__ qidx, int32_t* __restrict__ ids,
                                                            int32_t* __restrict__ type_ids, int32_t* __restrict__ lens,
                                                            int P, int Q, int S, int mq, int cls, int sep, int pad) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= P) return;
  // qidx and the lens are device data: clamped before they form an address
  const int q = clampi(qidx[row], 0, Q - 1);
  const int nq = min(min(clampi(lens_q[q], 2, S) - 2, mq), S - 3);  // 0 .. S-3
  const int np = min(clampi(lens_p[row], 2, S) - 2, S - 3 - nq);    // 0 .. S-3-nq
  const int32_t* qrow = ids_q + (size_t)q * S;
  const int32_t* prow = ids_p + (size_t)row * S;
  int32_t* out = ids + (size_t)row * S;
  int32_t* tout = type_ids + (size_t)row * S;
  const int sep1 = nq + 1, sep2 = nq + np + 2;  // sep2 <= S-1
  for (int j = lane; j < S; j += 64) {
    // query token j (1..nq) and passage token j - sep1 (1..np): columns clamped into the row
    const int32_t tq = qrow[min(j, S - 1)];
    const int32_t tp = prow[clampi(j - sep1, 0, S - 1)];
    int32_t v = pad;
    v = j < sep2 ? tp : v;
    v = j <= nq ? tq : v;
    v = (j == sep1 || j == sep2) ? sep : v;
    v = j == 0 ? cls : v;
    out[j] = v;
    tout[j] = (j > sep1 && j <= sep2) ? 1 : 0;
  }
  if (lane == 0) lens[row] = nq + np + 3;
}

__global__ __launch_bounds__(256) void group_topk_kernel(const float* __restrict__ scores,
                                                         const int32_t* __restrict__ goff, int32_t* __restrict__ idx,
                                                         float* __restrict__ val, int P, int Q, int k) {
  const int lane = threadIdx.x & 63;
  const int q = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (q >= Q) return;  // wave-uniform: the butterflies below run with all 64 lanes
  // offsets are device data: clamped into [0, P], a decreasing pair is an empty group
  const int g0 = clampi(goff[q], 0, P);
  const int len = max(clampi(goff[q + 1], 0, P) - g0, 0);
  const float ninf = -__builtin_inff();
  float pv = __builtin_inff();  // the previous pick: everything comes after (+inf, -1)
  int pi = -1;
  for (int n = 0; n < k; ++n) {
    float bv = ninf;
    int bi = kNoIdx;
    for (int base = 0; base < len; base += 64) {  // wave-uniform trip count
      const int i = base + lane;
      float x = scores[min(g0 + min(i, len - 1), P - 1)];  // P >= 1 (host), len >= 1 here
      x = x != x ? ninf : x;                                // a NaN ranks as -inf
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
    // every lane holds the round's pick; (-inf, kNoIdx): the group is exhausted, and stays so
    if (lane == 0) {
      idx[(size_t)q * k + n] = bi == kNoIdx ? -1 : bi;
      val[(size_t)q * k + n] = bv;
    }
    pv = bv;
    pi = bi;
  }
}

}  // namespace

void pair_assemble(const int32_t* ids_q, const int32_t* lens_q, const int32_t* ids_p, const int32_t* lens_p,
                   const int32_t* qidx, int32_t* ids, int32_t* type_ids, int32_t* lens, int P, int Q, int S, int mq,
                   int cls, int sep, int pad, hipStream_t stream) {
  ATPU_CHECK(S >= 4, "pair_assemble: S must be >= 4");
  ATPU_CHECK(Q >= 1 && mq >= 0, "pair_assemble: Q must be >= 1 and max_query_tokens >= 0");
  ATPU_CHECK(ids_q && lens_q && ids_p && lens_p && qidx && ids && type_ids && lens, "pair_assemble: null tensor");
  if (P <= 0) return;
  hipLaunchKernelGGL(pair_assemble_kernel, dim3((P + 3) / 4), dim3(256), 0, stream, ids_q, lens_q, ids_p, lens_p, qidx,
                     ids, type_ids, lens, P, Q, S, mq, cls, sep, pad);
  ATPU_HIP_CHECK(hipGetLastError());
}

void group_topk(const float* scores, const int32_t* goff, int32_t* idx, float* val, int P, int Q, int k,
                hipStream_t stream) {
  ATPU_CHECK(k >= 1 && k <= 32, "group_topk: k must be in [1, 32]");
  ATPU_CHECK(P >= 1, "group_topk: P must be >= 1");
  ATPU_CHECK(scores && goff && idx && val, "group_topk: null tensor");
  if (Q <= 0) return;
  hipLaunchKernelGGL(group_topk_kernel, dim3((Q + 3) / 4), dim3(256), 0, stream, scores, goff, idx, val, P, Q, k);
  ATPU_HIP_CHECK(hipGetLastError());
}

}  // namespace atpu
