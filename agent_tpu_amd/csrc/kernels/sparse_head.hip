// Learned sparse (SPLADE) term weights: the vocabulary product of every live token of every text,
// reduced per text to its maximum (term_max), then the bias, the positive terms and the best k of
// them (term_select). No [B*S, V] tensor exists: only xmax [B, V] is written.
//
// term_max_kernel<NS>. Vocabulary-stationary, the other way round from vocab_topk: one workgroup
// of 8 waves owns a tile of VT = 16 NS vocabulary entries (NS = 4: 64 entries; NS = 2: 32) and
// loads it ONCE into LDS, so E is read from HBM once per launch; the small t is re-read by every
// workgroup out of L2 / MALL. The LDS image is in fragment order: the 16-byte piece that lane
// (r = lane & 15, g = lane >> 4) feeds as the A operand of MFMA k-chunk kc (32 columns) of
// vocabulary subtile s sits at piece index (s * H/32 + kc) * 64 + lane, so a wave's ds_read_b128
// is one contiguous 1 KiB and conflict free, with no padding (VT * H * 2 bytes: 96 KiB at H = 768,
// 128 KiB at H = 1024, hence hipFuncSetAttribute). Tile rows past V repeat row V - 1 (clamped
// before the address is formed) and are not written.
//
// Split: whole texts to waves, wave w takes texts w, w + 8, ... Nothing is combined across waves:
// no atomics, no LDS traffic after the tile load. A text is walked in steps of two 16-token tiles
// (an A fragment read from LDS serves both: one ds_read_b128 per two MFMAs); a token tile never
// spans two texts, tiles past lens[b] are neither loaded nor multiplied, and the rows of a text's
// last tile past lens[b] re-read row lens[b] - 1 (so no padding row is ever loaded) and are set to
// -inf by select on the accumulator. Tokens are the N dimension of v_mfma_f32_16x16x32_bf16: a
// token's column depends on no other column. Token rows go global -> registers as bf16x8 per lane
// (B operand), 128 columns per stage, double buffered across stages, tiles and texts.
//
// Arithmetic: one fp32 accumulator per (token, vocabulary entry), k-chunks in ascending order:
// the order is a function of H alone, so xmax[b, v] has the same bits whatever B, the text's
// index and its neighbours. The running maximum sits in registers next to the accumulators
// (lane (r, g) holds tokens r mod 16 against entries 16 s + 4 g + e) and is reduced over the 16
// lanes of a row by DPP at the text's end; max is exact in any order. lens[b] <= 0 gives -inf.
//
// term_select_kernel. One workgroup of 1024 threads per text; the row x[v] = xmax[b, v] + bias[v]
// (one fp32 add; adding the bias after the max is exact since fp32 rounding is monotone) is read
// from global memory / L2 on every pass, never assumed to fit LDS. A term's key is the bit
// pattern of x when x > 0 and 0 otherwise (NaN, -inf, zeros and negatives give no term); positive
// floats order as unsigned integers. nnz = the number of keys > 0. When nnz > k a radix select
// (four 8-bit digits from the top, 256-bin histograms in LDS) finds the k-th key T and how many
// entries equal to T the list still takes; otherwise T = 0 and every term is taken. An ordered
// compaction (a block prefix scan per 1024-entry chunk, ascending token) takes every key > T and
// the first remaining slots' worth of keys == T, and a bitonic sort of the at most 1024 entries in
// LDS orders them (x descending, token ascending). Every slot of tok / xs / w is written: (-1, 0,
// 0) past the list; w = log1pf(xs).
//
// Registers (hipcc -O3 for gfx950, packed fp32 ops off): term_max_kernel<4> 139 VGPRs, <2> 106, term_select_kernel 42;
// no AGPRs, no scratch in any of them. Tile choice and timings: docs/PERF_NOTES.md "map_sparse_embed".
#include "atpu/common.h"
#include "atpu/kernels.h"

namespace atpu {
namespace {

constexpr int kTmWaves = 8;
constexpr int kTmStage = 4;      // MFMA k-chunks (of 32 columns) per load stage
constexpr int kSelThreads = 1024;
constexpr int kSelMax = 1024;    // the longest list
constexpr int kNoTok = 0x7fffffff;

struct TokFrag {
  bf16x8 b[2][kTmStage];  // [token tile][k-chunk of the stage]
};

// where a wave is in its walk: text b of length len, tile pair tp, load stage ks
struct TmPos {
  int b, len, tp, ks;
};

__device__ __forceinline__ int tm_len(const int32_t* __restrict__ lens, int b, int S) {
  return min(max(lens[b], 0), S);
}

// the next text of the wave with at least one token (b >= B: the walk is over)
__device__ __forceinline__ void tm_seek(TmPos& p, const int32_t* __restrict__ lens, int B, int S) {
  p.len = 0;
  while (p.b < B) {
    p.len = tm_len(lens, p.b, S);
    if (p.len > 0) break;
    p.b += kTmWaves;
  }
  p.tp = 0;
  p.ks = 0;
}

__device__ __forceinline__ void tm_load(TokFrag& f, const bf16* __restrict__ t, const TmPos& p, int S, int H, int r,
                                        int g) {
  const int KC = H >> 5;
#pragma unroll
  for (int tt = 0; tt < 2; ++tt) {
    const int tok0 = (2 * p.tp + tt) * 16;
    if (tok0 < p.len) {  // wave-uniform: a tile past the text is not loaded
      const int row = min(tok0 + r, p.len - 1);  // the last tile's tail re-reads a live row
      const bf16* src = t + ((size_t)p.b * S + row) * H + p.ks * (32 * kTmStage) + 8 * g;
#pragma unroll
      for (int j = 0; j < kTmStage; ++j)
        if (p.ks * kTmStage + j < KC) f.b[tt][j] = *reinterpret_cast<const bf16x8*>(src + 32 * j);
    }
  }
}

template <int NS>
__global__ __launch_bounds__(kTmWaves* kWave) void term_max_kernel(const bf16* __restrict__ t,
                                                                   const int32_t* __restrict__ lens,
                                                                   const bf16* __restrict__ E,
                                                                   float* __restrict__ xmax, int B, int S, int V,
                                                                   int H) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  bf16x8* tile = reinterpret_cast<bf16x8*>(smem_raw);
  constexpr int VT = 16 * NS;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 15, g = lane >> 4;
  const int v0 = blockIdx.x * VT;
  const int KC = H >> 5, C8 = H >> 3;
  const float ninf = -__builtin_inff();

  // vocabulary tile -> LDS in fragment order; rows past V repeat row V - 1
  for (int i = tid; i < VT * C8; i += kTmWaves * kWave) {
    const int row = i / C8, c8 = i - row * C8;
    const int vr = min(v0 + row, V - 1);
    const int s = row >> 4, rr = row & 15, kc = c8 >> 2, gg = c8 & 3;
    tile[(s * KC + kc) * 64 + gg * 16 + rr] = *reinterpret_cast<const bf16x8*>(E + (size_t)vr * H + 8 * c8);
  }

  // empty texts of this wave: -inf, written before the walk that skips them
  for (int b = wave; b < B; b += kTmWaves)
    if (tm_len(lens, b, S) == 0)
      for (int i = lane; i < VT; i += 64)
        if (v0 + i < V) xmax[(size_t)b * V + v0 + i] = ninf;
  __syncthreads();

  const int KS = (KC + kTmStage - 1) / kTmStage;
  f32x4 acc[2][NS];
  float m[NS][4];
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    acc[0][s] = acc[1][s] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int e = 0; e < 4; ++e) m[s][e] = ninf;
  }

  TmPos p;
  p.b = wave;
  tm_seek(p, lens, B, S);
  TokFrag f0, f1;
  if (p.b < B) tm_load(f0, t, p, S, H, r, g);

  auto stage = [&](const TokFrag& cur, TokFrag& nxt) {
    TmPos n = p;
    const bool last_ks = p.ks + 1 == KS;
    const bool last_tp = (p.tp + 1) * 32 >= p.len;
    if (!last_ks) {
      n.ks = p.ks + 1;
    } else if (!last_tp) {
      n.tp = p.tp + 1;
      n.ks = 0;
    } else {
      n.b = p.b + kTmWaves;
      tm_seek(n, lens, B, S);
    }
    __builtin_amdgcn_sched_barrier(0);
    if (n.b < B) tm_load(nxt, t, n, S, H, r, g);
    __builtin_amdgcn_sched_barrier(0);
    const bool two = (2 * p.tp + 1) * 16 < p.len;  // wave-uniform: the pair's second tile is live
#pragma unroll
    for (int j = 0; j < kTmStage; ++j) {
      const int kc = p.ks * kTmStage + j;
      if (kc < KC) {
        bf16x8 a[NS];
#pragma unroll
        for (int s = 0; s < NS; ++s) a[s] = tile[(s * KC + kc) * 64 + lane];
#pragma unroll
        for (int s = 0; s < NS; ++s) acc[0][s] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[s], cur.b[0][j], acc[0][s], 0, 0, 0);
        if (two) {
#pragma unroll
          for (int s = 0; s < NS; ++s)
            acc[1][s] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[s], cur.b[1][j], acc[1][s], 0, 0, 0);
        }
      }
    }
    if (last_ks) {  // the pair's products are complete: padding tokens to -inf by select, then the maximum
#pragma unroll
      for (int tt = 0; tt < 2; ++tt) {
        const bool live = (2 * p.tp + tt) * 16 + r < p.len;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
#pragma unroll
          for (int e = 0; e < 4; ++e) m[s][e] = fmaxf(m[s][e], live ? acc[tt][s][e] : ninf);
          acc[tt][s] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
      }
      if (last_tp) {  // the text's end: the maximum over the 16 token lanes of a row, then lane r == s writes subtile s
        float out[4] = {ninf, ninf, ninf, ninf};
#pragma unroll
        for (int s = 0; s < NS; ++s)
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            float x = m[s][e];
            x = fmaxf(x, dppf<kDppMirror>(x));
            x = fmaxf(x, dppf<kDppHalfMirror>(x));
            x = fmaxf(x, dppf<kDppXor2>(x));
            x = fmaxf(x, dppf<kDppXor1>(x));
            out[e] = r == s ? x : out[e];
            m[s][e] = ninf;
          }
        if (r < NS) {
          const int v = v0 + 16 * r + 4 * g;
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (v + e < V) xmax[(size_t)p.b * V + v + e] = out[e];
        }
      }
    }
    p = n;
  };
  while (p.b < B) {
    stage(f0, f1);
    if (p.b < B) stage(f1, f0);
  }
}

template <int NS>
void tm_launch(const bf16* t, const int32_t* lens, const bf16* E, float* xmax, int B, int S, int V, int H,
               hipStream_t stream) {
  constexpr int VT = 16 * NS;
  const size_t lds = (size_t)VT * H * sizeof(bf16);
  // up to 128 KiB of dynamic LDS (VT = 64, H = 1024); the attribute is per device
  ATPU_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&term_max_kernel<NS>),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL((term_max_kernel<NS>), dim3((V + VT - 1) / VT), dim3(kTmWaves * kWave), lds, stream, t, lens, E,
                     xmax, B, S, V, H);
  ATPU_HIP_CHECK(hipGetLastError());
}

// ---------------------------------------------------------------------------------- term_select
__device__ __forceinline__ unsigned sel_key(const float* __restrict__ row, const float* __restrict__ bias, int v) {
  const float x = row[v] + bias[v];
  return x > 0.f ? __float_as_uint(x) : 0u;  // NaN compares false: no term
}

// (key descending, token ascending): a goes before b
__device__ __forceinline__ bool sel_before(unsigned ka, int ta, unsigned kb, int tb) {
  return ka > kb || (ka == kb && ta < tb);
}

__global__ __launch_bounds__(kSelThreads) void term_select_kernel(const float* __restrict__ xmax,
                                                                  const float* __restrict__ bias,
                                                                  int32_t* __restrict__ tok, float* __restrict__ xs,
                                                                  float* __restrict__ w, int32_t* __restrict__ nnz,
                                                                  int V, int k) {
  __shared__ unsigned hist[256];
  __shared__ unsigned lkey[kSelMax];
  __shared__ int ltok[kSelMax];
  __shared__ unsigned wtot[kSelThreads / kWave];
  __shared__ unsigned sh_prefix, sh_need, sh_base, sh_cnt;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x;
  const float* row = xmax + (size_t)b * V;

  if (tid == 0) sh_cnt = 0;
  __syncthreads();
  unsigned mine = 0;
  for (int v = tid; v < V; v += kSelThreads) mine += sel_key(row, bias, v) != 0u;
  if (mine) atomicAdd(&sh_cnt, mine);
  __syncthreads();
  const unsigned total = sh_cnt;  // the positive entries before the cut

  // radix select of the k-th key, only when the cut falls inside the positive entries
  unsigned T = 0, need = 0;  // need: how many entries equal to T the list takes
  if (total > (unsigned)k) {
    unsigned prefix = 0;
    need = k;
    for (int shift = 24; shift >= 0; shift -= 8) {
      if (tid < 256) hist[tid] = 0;
      __syncthreads();
      const unsigned himask = shift == 24 ? 0u : ~0u << (shift + 8);
      for (int v = tid; v < V; v += kSelThreads) {
        const unsigned key = sel_key(row, bias, v);
        if ((key & himask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1u);
      }
      __syncthreads();
      if (tid == 0) {  // from the top digit down to the bin that holds the need-th key
        unsigned cum = 0;
        int d = 255;
        for (; d > 0; --d) {
          if (cum + hist[d] >= need) break;
          cum += hist[d];
        }
        sh_prefix = prefix | ((unsigned)d << shift);
        sh_need = need - cum;
      }
      __syncthreads();
      prefix = sh_prefix;
      need = sh_need;
    }
    T = prefix;
  }

  // ordered compaction: keys > T anywhere in the list's head, the first `need` keys == T behind them
  const unsigned above = total > (unsigned)k ? (unsigned)k - need : total;
  if (tid == 0) sh_base = 0;  // low half: keys > T so far; high half: keys == T so far
  __syncthreads();
  for (int c0 = 0; c0 < V; c0 += kSelThreads) {
    const int v = c0 + tid;
    const unsigned key = v < V ? sel_key(row, bias, v) : 0u;
    const bool gt = key > T, eq = T != 0u && key == T;
    unsigned x = (gt ? 1u : 0u) | (eq ? 0x10000u : 0u);  // both counts of a chunk fit 16 bits (<= 1024)
    const unsigned own = x;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned y = __shfl_up(x, o, 64);
      if (lane >= o) x += y;
    }
    if (lane == 63) wtot[wave] = x;
    __syncthreads();
    unsigned off = 0, all = 0;
    for (int i = 0; i < kSelThreads / kWave; ++i) {
      const unsigned c = wtot[i];
      off += i < wave ? c : 0u;
      all += c;
    }
    const unsigned base = sh_base;
    const unsigned excl = x - own + off;
    const unsigned n_gt = (base & 0xffffu) + (excl & 0xffffu), n_eq = (base >> 16) + (excl >> 16);
    if (gt) {  // n_gt < above <= 1024 by construction; the bound check keeps a bad count out of LDS
      if (n_gt < (unsigned)kSelMax) {
        lkey[n_gt] = key;
        ltok[n_gt] = v;
      }
    } else if (eq && n_eq < need && above + n_eq < (unsigned)kSelMax) {
      lkey[above + n_eq] = key;
      ltok[above + n_eq] = v;
    }
    __syncthreads();
    if (tid == 0) {
      const unsigned lo = min((base & 0xffffu) + (all & 0xffffu), 0xffffu);
      const unsigned hi = min((base >> 16) + (all >> 16), 0xffffu);  // saturate: only "< need" is asked of it
      sh_base = lo | (hi << 16);
    }
    __syncthreads();
  }
  const int cnt = (int)min(total, (unsigned)k);

  // bitonic sort of the n = 2^j >= cnt entries, padded with (0, kNoTok), which sort last
  int n = 2;
  while (n < cnt) n <<= 1;
  if (tid >= cnt && tid < n) {
    lkey[tid] = 0u;
    ltok[tid] = kNoTok;
  }
  __syncthreads();
  for (int size = 2; size <= n; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      const int j = tid ^ stride;
      if (tid < n && j > tid) {
        const unsigned ka = lkey[tid], kb = lkey[j];
        const int ta = ltok[tid], tb = ltok[j];
        const bool up = (tid & size) == 0;  // this pair sorts into list order
        if (sel_before(kb, tb, ka, ta) == up) {
          lkey[tid] = kb;
          ltok[tid] = tb;
          lkey[j] = ka;
          ltok[j] = ta;
        }
      }
      __syncthreads();
    }
  }
  for (int i = tid; i < k; i += kSelThreads) {
    const bool got = i < cnt;
    const float x = got ? __uint_as_float(lkey[i]) : 0.f;
    tok[(size_t)b * k + i] = got ? ltok[i] : -1;
    xs[(size_t)b * k + i] = x;
    w[(size_t)b * k + i] = got ? log1pf(x) : 0.f;
  }
  if (tid == 0) nnz[b] = (int)total;
}

}  // namespace

void term_max(const bf16* t, const int32_t* lens, const bf16* E, float* xmax, int B, int S, int V, int H,
              int vocab_tile, hipStream_t stream) {
  ATPU_CHECK(H % 64 == 0 && H >= 64 && H <= 1024, "term_max: H must be a multiple of 64 in [64, 1024]");
  ATPU_CHECK(S >= 1 && S <= 512, "term_max: S must be in [1, 512]");
  ATPU_CHECK(V >= 1 && B >= 1, "term_max: V and B must be >= 1");
  ATPU_CHECK(vocab_tile == 0 || vocab_tile == 32 || vocab_tile == 64, "term_max: vocab_tile must be 0, 32 or 64");
  ATPU_CHECK(t && lens && E && xmax, "term_max: null tensor");
  ATPU_CHECK(((reinterpret_cast<uintptr_t>(t) | reinterpret_cast<uintptr_t>(E)) & 15) == 0 &&
                 ((reinterpret_cast<uintptr_t>(lens) | reinterpret_cast<uintptr_t>(xmax)) & 3) == 0,
             "term_max: t and E must be 16-byte, lens and xmax 4-byte aligned");
  if (vocab_tile == 32) tm_launch<2>(t, lens, E, xmax, B, S, V, H, stream);
  else tm_launch<4>(t, lens, E, xmax, B, S, V, H, stream);
}

void term_select(const float* xmax, const float* bias, int32_t* tok, float* xs, float* w, int32_t* nnz, int B, int V,
                 int k, hipStream_t stream) {
  ATPU_CHECK(k >= 1 && k <= kSelMax, "term_select: k must be in [1, 1024]");
  ATPU_CHECK(V >= 1 && B >= 1, "term_select: V and B must be >= 1");
  ATPU_CHECK(xmax && bias && tok && xs && w && nnz, "term_select: null tensor");
  ATPU_CHECK(((reinterpret_cast<uintptr_t>(xmax) | reinterpret_cast<uintptr_t>(bias) | reinterpret_cast<uintptr_t>(tok) |
               reinterpret_cast<uintptr_t>(xs) | reinterpret_cast<uintptr_t>(w) | reinterpret_cast<uintptr_t>(nnz)) &
              3) == 0,
             "term_select: tensors must be 4-byte aligned");
  hipLaunchKernelGGL(term_select_kernel, dim3(B), dim3(kSelThreads), 0, stream, xmax, bias, tok, xs, w, nnz, V, k);
  ATPU_HIP_CHECK(hipGetLastError());
}

}  // namespace atpu
