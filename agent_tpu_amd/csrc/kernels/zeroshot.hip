// Zero-shot classification front and back end: premise-first pair rows from single-segment rows,
// and the label scores with the full per-text ranking of the NLI logits.
//
// premise_assemble_kernel ("atpu-premise v1", Python twin: agent_tpu_amd/tokenizer.py
// premise_rows). The frame of pair_assemble_kernel (rerank.hip): one 64-wide wave per pair row, four
// rows per workgroup. Here neither segment is "one row per pair": row r takes the text row
// tidx[r] first, cut to the room the hypothesis leaves (HF only_first), and the hypothesis row
// hidx[r] second, kept whole up to mh tokens. Position j of the output row is a pure function of
// (j, nt, nh), so a lane reads at most one id of each source row and writes ids / type_ids at
// j, j + 64, ...: coalesced, no LDS, no scan. Every data-dependent index is clamp-then-select:
// tidx into [0, T), hidx into [0, Hn), both lens into [2, S], the token columns into the row.
//
// nli_rank_kernel. One wave per text (group), four groups per workgroup. A pair's key and score
// come from its two logits (e, c): multi-label, and any group of one, key m = e - c and score
// 1 / (1 + exp(-m)); single-label key e and score exp(e - mx) / sum over the group. The whole
// group is ranked, by counting: element i lands at the number of elements that come before it
// in the total order (key desc, index asc; better() of atpu/topk.h), which is unique, so no sort
// network and no limit on the group's length.
// Where the keys live: nowhere. A wave re-reads the group's 8-byte logit pairs and recomputes
// the keys (one subtraction, two NaN tests), in tiles of 64: per tile of its own elements
// (i = base + lane) it walks the group's tiles (j = jbase + lane, one load per lane), and the 64
// keys of a j tile reach every lane by v_readlane with a constant lane, registers only. Cost per
// lane: ceil(len / 64)^2 8-byte loads, all L1/L2 hits after the first walk (a group of 1000 pairs is
// 8 KB), and len * ceil(len / 64) compare steps of ~4 VALU: 64 steps for a group of up to 64 labels,
// 16 K for 1000. LDS would save the re-reads but bound the group (or need a second path past
// the bound) for a kernel whose groups are label sets of a few to a few hundred.
// Sums: lane l adds exp(key_i - mx) for i = l, l + 64, ... in ascending i, then the fixed
// butterfly of wave_sum: the order depends on the group's length alone, so a text's outputs have
// the same bits whatever shares its launch and wherever its group starts.
#include "atpu/common.h"
#include "atpu/kernels.h"
#include "atpu/topk.h"

namespace atpu {
namespace {

__device__ __forceinline__ int clampi(int x, int lo, int hi) { return min(max(x, lo), hi); }

__global__ __launch_bounds__(256) void premise_assemble_kernel(
    const int32_t* __restrict__ ids_t, const int32_t* __restrict__ lens_t, const int32_t* __restrict__ ids_h,
    const int32_t* __restrict__ lens_h, const int32_t* __restrict__ tidx, const int32_t* __restrict__ hidx,
    int32_t* __restrict__ ids, int32_t* __restrict__ type_ids, int32_t* __restrict__ lens, int P, int T, int Hn, int S,
    int mh, int cls, int sep, int pad) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= P) return;
  // the indices and the lens are device data: clamped before they form an address
  const int t = clampi(tidx[row], 0, T - 1);
  const int h = clampi(hidx[row], 0, Hn - 1);
  const int nh = min(min(clampi(lens_h[h], 2, S) - 2, mh), S - 3);  // 0 .. S-3
  const int nt = min(clampi(lens_t[t], 2, S) - 2, S - 3 - nh);      // 0 .. S-3-nh
  const int32_t* trow = ids_t + (size_t)t * S;
  const int32_t* hrow = ids_h + (size_t)h * S;
  int32_t* out = ids + (size_t)row * S;
  int32_t* tout = type_ids + (size_t)row * S;
  const int sep1 = nt + 1, sep2 = nt + nh + 2;  // sep2 <= S-1
  for (int j = lane; j < S; j += 64) {
    // text token j (1..nt) and hypothesis token j - sep1 (1..nh): columns clamped into the row
    const int32_t tt = trow[min(j, S - 1)];
    const int32_t th = hrow[clampi(j - sep1, 0, S - 1)];
    int32_t v = pad;
    v = j < sep2 ? th : v;
    v = j <= nt ? tt : v;
    v = (j == sep1 || j == sep2) ? sep : v;
    v = j == 0 ? cls : v;
    out[j] = v;
    tout[j] = (j > sep1 && j <= sep2) ? 1 : 0;
  }
  if (lane == 0) lens[row] = nt + nh + 3;
}

// the ranking key of pair i of the group (i clamped into it; the caller discards what it does not
// take): e - c or e; a NaN logit, or a NaN difference (inf - inf), ranks as -inf
__device__ __forceinline__ float nli_key(const float2* __restrict__ pair, int g0, int len, int P, int i, bool multi) {
  const float2 ec = pair[min(g0 + min(i, len - 1), P - 1)];  // P >= 1 (host), len >= 1 at every call
  const float k = multi ? ec.x - ec.y : ec.x;
  return (ec.x != ec.x || ec.y != ec.y || k != k) ? -__builtin_inff() : k;
}

__global__ __launch_bounds__(256) void nli_rank_kernel(const float2* __restrict__ pair, const int32_t* __restrict__ goff,
                                                       int32_t* __restrict__ order, float* __restrict__ score, int P,
                                                       int T, int mode) {
  const int lane = threadIdx.x & 63;
  const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= T) return;  // wave-uniform: the reductions and v_readlane below run with all 64 lanes
  // offsets are device data: clamped into [0, P], a decreasing pair is an empty group
  const int g0 = clampi(goff[t], 0, P);
  const int len = max(clampi(goff[t + 1], 0, P) - g0, 0);
  if (len == 0) return;  // wave-uniform
  const bool multi = mode != 0 || len == 1;  // HF: one candidate label is scored entail-vs-contradiction
  const float ninf = -__builtin_inff();
  float mx = ninf, sum = 0.f;
  if (!multi) {
    for (int base = 0; base < len; base += 64) {  // wave-uniform trip count
      const float k = nli_key(pair, g0, len, P, base + lane, false);
      mx = fmaxf(mx, base + lane < len ? k : ninf);
    }
    mx = wave_max(mx);
    for (int base = 0; base < len; base += 64) {
      const float k = nli_key(pair, g0, len, P, base + lane, false);
      // k == mx: 0 also where both are +inf (inf - inf is NaN)
      sum += base + lane < len ? __expf(k == mx ? 0.f : k - mx) : 0.f;
    }
    sum = wave_sum(sum);
  }
  for (int base = 0; base < len; base += 64) {
    const int i = base + lane;
    const float ki = nli_key(pair, g0, len, P, i, multi);
    int cnt = 0;
    for (int jb = 0; jb < len; jb += 64) {
      // a j past the group: (-inf, j >= len > i) comes before no element
      const float kl = jb + lane < len ? nli_key(pair, g0, len, P, jb + lane, multi) : ninf;
#pragma unroll
      for (int n = 0; n < 64; ++n) {
        const float kj = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(kl), n));
        cnt += better(kj, jb + n, ki, i) ? 1 : 0;
      }
    }
    float s;
    if (multi) {
      s = 1.0f / (1.0f + __expf(-ki));  // -inf: 1 / inf = 0
    } else {
      s = mx == ninf ? 0.f : __expf(ki == mx ? 0.f : ki - mx) / sum;
    }
    if (i < len) {
      const int at = g0 + min(cnt, len - 1);  // cnt < len in a total order; clamped all the same
      order[at] = i;
      score[at] = s;
    }
  }
}

}  // namespace

void premise_assemble(const int32_t* ids_t, const int32_t* lens_t, const int32_t* ids_h, const int32_t* lens_h,
                      const int32_t* tidx, const int32_t* hidx, int32_t* ids, int32_t* type_ids, int32_t* lens, int P,
                      int T, int Hn, int S, int mh, int cls, int sep, int pad, hipStream_t stream) {
  ATPU_CHECK(S >= 4, "premise_assemble: S must be >= 4");
  ATPU_CHECK(T >= 1 && Hn >= 1 && mh >= 0, "premise_assemble: T and Hn must be >= 1 and max_hypothesis_tokens >= 0");
  ATPU_CHECK(ids_t && lens_t && ids_h && lens_h && tidx && hidx && ids && type_ids && lens,
             "premise_assemble: null tensor");
  if (P <= 0) return;
  hipLaunchKernelGGL(premise_assemble_kernel, dim3((P + 3) / 4), dim3(256), 0, stream, ids_t, lens_t, ids_h, lens_h,
                     tidx, hidx, ids, type_ids, lens, P, T, Hn, S, mh, cls, sep, pad);
  ATPU_HIP_CHECK(hipGetLastError());
}

void nli_rank(const float* pair, const int32_t* goff, int32_t* order, float* score, int P, int T, int mode,
              hipStream_t stream) {
  ATPU_CHECK(mode == 0 || mode == 1, "nli_rank: mode must be 0 (single-label) or 1 (multi-label)");
  ATPU_CHECK(P >= 1, "nli_rank: P must be >= 1");
  ATPU_CHECK(pair && goff && order && score, "nli_rank: null tensor");
  ATPU_CHECK((reinterpret_cast<uintptr_t>(pair) & 7) == 0, "nli_rank: pair must be 8-byte aligned");
  if (T <= 0) return;
  hipLaunchKernelGGL(nli_rank_kernel, dim3((T + 3) / 4), dim3(256), 0, stream, reinterpret_cast<const float2*>(pair),
                     goff, order, score, P, T, mode);
  ATPU_HIP_CHECK(hipGetLastError());
}

}  // namespace atpu
