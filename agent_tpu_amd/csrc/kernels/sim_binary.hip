// Binary (sign-bit) corpus: a row of D floats is stored as D bits, bit d = x_d > thr_d, in W = D / 32 words
// (bit b of word w = column 32 w + b). A query, packed the same way, is scored by the Hamming distance:
// score(q, r) = D - 2 * popcount(qbits XOR rbits), the dot product of the two +-1 vectors, written as fp32.
// It is an exact integer with |score| <= 1024, larger is better, so sim_topk's (score, row) workspace,
// better() and sim_topk_merge apply unchanged. No table and no gather: xor and v_bcnt on the VALU.
//
// binary_pack_kernel: one workgroup of 4 waves per 64-row block. A wave reads 64 consecutive columns of one
// row in one coalesced 256 B load; __ballot(x > thr) is two words of that row. The block's [W][64] words
// are staged in LDS and written out contiguously: as they lie for the scan layout
// [ceil(n / 64)][W][64] (word (b, w, lane) = bits(64 b + lane, w); the rows past n of the last block are
// zero), or transposed for the row-major [n, W] that the queries use. The comparison is plain: -0.0, +0.0
// and NaN give 0 against a zero threshold.
//
// hamming_scan_kernel<WP, KM>: row-stationary, the other way round from pq.hip. The rows are cut into
// segments of seg_blocks 64-row blocks and every segment into `parts` pieces of bpp blocks; one workgroup of
// 8 waves per (segment, part, tile of at most 32 queries). The tile's words sit in LDS ([32][WP] words, WP
// = W rounded up to a multiple of 8, the padding zero, so a query is WP / 4 broadcast 16-byte reads). A wave
// step loads two 64-row blocks: each lane holds two whole rows in 2 WP <= 64 VGPRs, loaded once as
// contiguous 256 B per word, and the wave loops over the tile's queries with one xor and one
// popcount-accumulate per word and row; every query word serves both rows. The codes are read once per
// query tile, not once per query.
//
// Top-k without per-lane lists: each (wave, query) owns a sorted list of KM >= k entries in LDS
// (8 x 32 x KM x 8 B, 64 KiB at KM = 32). The list's last entry is the bar, one broadcast read per (step,
// query); the lanes whose (score, row) beats it are found by ballot, and only then is the list loaded
// (entry e in lane e) and each such lane inserted in ascending lane order by a wave-cooperative sorted
// insert: lane e recomputes entry e from entries e - 1, e and the candidate. Rows are walked in ascending
// id, so an equal score never beats the bar. At the end the 8 wave lists of a query are merged by 8 lanes
// (k rounds of best head) into ws [nq, items, k], items = segments x parts; every slot is written, also
// for a part without rows (empty entries are (-inf, 0x7fffffff)).
//
// Rows past N and a block past the part are clamped before they form an address and discarded by select.
// Nothing outside the codes' blocks [0, ceil(N / 64)), the query words and ws is touched.
#include "atpu/common.h"
#include "atpu/kernels.h"
#include "atpu/topk.h"

namespace atpu {
namespace {

constexpr int kNoRow = 0x7fffffff;
constexpr int kBinBlock = 64;  // rows of one block of the scan layout
constexpr int kPackWaves = 4, kPackThreads = kPackWaves * kWave;
constexpr int kHamWaves = 8, kHamThreads = kHamWaves * kWave;
constexpr int kHamTile = 32;  // queries of one work item

__global__ __launch_bounds__(kPackThreads) void binary_pack_kernel(const float* __restrict__ x,
                                                                   const float* __restrict__ thr,
                                                                   uint32_t* __restrict__ out, int64_t n, int D,
                                                                   int interleave) {
  __shared__ uint32_t sm[32 * kBinBlock];  // [W][64]
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int W = D >> 5;
  const int64_t r0 = (int64_t)blockIdx.x * kBinBlock;
  for (int c = 0; c < (D >> 6); ++c) {
    const float t = thr[64 * c + lane];
#pragma unroll 4
    for (int j = 0; j < kBinBlock / kPackWaves; ++j) {
      const int r = wave + kPackWaves * j;
      const bool live = r0 + r < n;  // wave-uniform; a row past n reads row n - 1 and packs to zero
      const float xv = x[(size_t)(live ? r0 + r : n - 1) * D + 64 * c + lane];
      const unsigned long long m = __ballot(live && xv > t);
      if (lane < 2) sm[(2 * c + lane) * kBinBlock + r] = (uint32_t)(m >> (32 * lane));
    }
  }
  __syncthreads();
  if (interleave) {
    uint32_t* dst = out + (size_t)blockIdx.x * W * kBinBlock;
    for (int i = tid; i < W * kBinBlock; i += kPackThreads) dst[i] = sm[i];
  } else {
    for (int i = tid; i < W * kBinBlock; i += kPackThreads) {
      const int r = i / W, w = i - r * W;
      if (r0 + r < n) out[(size_t)(r0 + r) * W + w] = sm[w * kBinBlock + r];
    }
  }
}

template <int WP, int KM>
__global__ __launch_bounds__(kHamThreads) void hamming_scan_kernel(const uint32_t* __restrict__ qbits,
                                                                   const uint32_t* __restrict__ codes,
                                                                   float2* __restrict__ ws, int nq, int N, int W, int k,
                                                                   int nblocks, int seg_blocks, int parts, int bpp) {
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];  // the query tile [32][WP], then the lists
  float2* lists = reinterpret_cast<float2*>(smem + kHamTile * WP);  // [kHamWaves][kHamTile][KM]
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int item = blockIdx.x, seg = item / parts, part = item - seg * parts;
  const int q0 = blockIdx.y * kHamTile, nqt = min(kHamTile, nq - q0);
  const int s_lo = seg * seg_blocks, s_hi = min(s_lo + seg_blocks, nblocks);
  const int b_lo = min(s_lo + part * bpp, s_hi), b_hi = min(b_lo + bpp, s_hi);  // may be empty
  const int D = W << 5;

  for (int i = tid; i < kHamTile * WP; i += kHamThreads) {
    const int qi = i / WP, w = i - qi * WP;
    const bool live = qi < nqt && w < W;
    const uint32_t x = qbits[live ? (size_t)(q0 + qi) * W + w : 0];
    smem[i] = live ? x : 0u;
  }
  for (int i = tid; i < kHamWaves * kHamTile * KM; i += kHamThreads)
    lists[i] = float2{-__builtin_inff(), __int_as_float(kNoRow)};
  __syncthreads();

  float2* wl = lists + wave * kHamTile * KM;
  for (int b = b_lo + 2 * wave; b < b_hi; b += 2 * kHamWaves) {
    // two blocks; a second block past the part repeats the part's last block and is discarded
    const uint32_t* p0 = codes + (size_t)b * W * kBinBlock + lane;
    const uint32_t* p1 = codes + (size_t)min(b + 1, b_hi - 1) * W * kBinBlock + lane;
    uint32_t r0[WP], r1[WP];
#pragma unroll
    for (int w = 0; w < WP; ++w) {
      const int wc = min(w, W - 1);
      const uint32_t x0 = p0[wc * kBinBlock], x1 = p1[wc * kBinBlock];
      r0[w] = w < W ? x0 : 0u;
      r1[w] = w < W ? x1 : 0u;
    }
    const int row0 = b * kBinBlock + lane, row1 = row0 + kBinBlock;
    const bool live0 = row0 < N, live1 = b + 1 < b_hi && row1 < N;
    const int id[2] = {live0 ? row0 : kNoRow, live1 ? row1 : kNoRow};
    for (int qi = 0; qi < nqt; ++qi) {
      const u32x4* qw = reinterpret_cast<const u32x4*>(smem + qi * WP);
      int d0 = 0, d1 = 0;
#pragma unroll
      for (int w4 = 0; w4 < WP / 4; ++w4) {
        const u32x4 x = qw[w4];  // one address for the wave: a broadcast
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          d0 += __popc(r0[4 * w4 + e] ^ x[e]);
          d1 += __popc(r1[4 * w4 + e] ^ x[e]);
        }
      }
      const float v[2] = {live0 ? (float)(D - 2 * d0) : -__builtin_inff(),
                          live1 ? (float)(D - 2 * d1) : -__builtin_inff()};
      const float2 bar = wl[qi * KM + KM - 1];
      const float bv = bar.x;
      const int bi = __float_as_int(bar.y);
      if (__ballot(better(v[0], id[0], bv, bi) || better(v[1], id[1], bv, bi)) != 0)
        wave_list_insert<KM, 2>(wl + qi * KM, lane, v, id);  // ascending lane = ascending row
    }
  }
  __syncthreads();

  // 8 lanes per query, one wave list each: k rounds of best head, the owner pops (rows are distinct)
  if (tid < kHamWaves * kHamTile) {
    const int qi = tid >> 3;
    const float2* mine = lists + ((tid & (kHamWaves - 1)) * kHamTile + qi) * KM;
    float2* dst = ws + ((size_t)(q0 + min(qi, nqt - 1)) * gridDim.x + item) * k;
    int pos = 0;
    for (int n = 0; n < k; ++n) {
      const float2 hd = mine[min(pos, KM - 1)];
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
      step(dppf<kDppHalfMirror>(bv), dppi<kDppHalfMirror>(bi));
      step(dppf<kDppXor2>(bv), dppi<kDppXor2>(bi));
      step(dppf<kDppXor1>(bv), dppi<kDppXor1>(bi));
      if (hi == bi && bi != kNoRow) ++pos;
      if ((tid & (kHamWaves - 1)) == 0 && qi < nqt) dst[n] = float2{bv, __int_as_float(bi)};
    }
  }
}

size_t ham_lds_bytes(int WP, int KM) {
  return (size_t)kHamTile * WP * sizeof(uint32_t) + (size_t)kHamWaves * kHamTile * KM * sizeof(float2);
}

template <int WP, int KM>
void ham_launch(const uint32_t* qbits, const uint32_t* codes, float2* ws, int nq, int N, int W, int k, int nblocks,
                int seg_blocks, int parts, int items, hipStream_t stream) {
  const size_t lds = ham_lds_bytes(WP, KM);  // up to 68 KiB (D = 1024, KM = 32); the attribute is per device
  ATPU_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&hamming_scan_kernel<WP, KM>),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  const int bpp = (seg_blocks + parts - 1) / parts;
  hipLaunchKernelGGL((hamming_scan_kernel<WP, KM>), dim3(items, (nq + kHamTile - 1) / kHamTile), dim3(kHamThreads), lds,
                     stream, qbits, codes, ws, nq, N, W, k, nblocks, seg_blocks, parts, bpp);
  ATPU_HIP_CHECK(hipGetLastError());
}

template <int WP>
void ham_dispatch(const uint32_t* qbits, const uint32_t* codes, float2* ws, int nq, int N, int W, int k, int nblocks,
                  int seg_blocks, int parts, int items, hipStream_t stream) {
  if (k <= 8) ham_launch<WP, 8>(qbits, codes, ws, nq, N, W, k, nblocks, seg_blocks, parts, items, stream);
  else if (k <= 16) ham_launch<WP, 16>(qbits, codes, ws, nq, N, W, k, nblocks, seg_blocks, parts, items, stream);
  else ham_launch<WP, 32>(qbits, codes, ws, nq, N, W, k, nblocks, seg_blocks, parts, items, stream);
}

}  // namespace

bool binary_shape_ok(int D) { return D % 64 == 0 && D >= 64 && D <= 1024; }

void binary_pack(const float* x, const float* thr, uint32_t* out, int64_t n, int D, bool interleave,
                 hipStream_t stream) {
  ATPU_CHECK(binary_shape_ok(D), "binary_pack: D must be a multiple of 64 in [64, 1024]");
  ATPU_CHECK(n >= 1 && n <= 2147483647LL - 256, "binary_pack: n must be in [1, 2^31 - 256]");
  ATPU_CHECK(x && thr && out, "binary_pack: null tensor");
  ATPU_CHECK(((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(thr) | reinterpret_cast<uintptr_t>(out)) & 3) ==
                 0, "binary_pack: x, thr and the words must be 4-byte aligned");
  const int64_t nb = (n + kBinBlock - 1) / kBinBlock;
  hipLaunchKernelGGL(binary_pack_kernel, dim3((unsigned)nb), dim3(kPackThreads), 0, stream, x, thr, out, n, D,
                     interleave ? 1 : 0);
  ATPU_HIP_CHECK(hipGetLastError());
}

int hamming_scan_items(int N, int seg_blocks, int parts) {
  const int nblocks = (N + kBinBlock - 1) / kBinBlock;
  return ((nblocks + seg_blocks - 1) / seg_blocks) * parts;
}

void hamming_scan_partial(const uint32_t* qbits, const uint32_t* codes, float* ws, int nq, int N, int D, int k,
                          int seg_blocks, int parts, hipStream_t stream) {
  ATPU_CHECK(nq >= 1 && N >= 1 && N <= 2147483647 - 256, "hamming_scan: nq >= 1 and N in [1, 2^31 - 256]");
  ATPU_CHECK(binary_shape_ok(D), "hamming_scan: D must be a multiple of 64 in [64, 1024]");
  ATPU_CHECK(k >= 1 && k <= 32, "hamming_scan: k must be in [1, 32]");
  const int nblocks = (N + kBinBlock - 1) / kBinBlock;
  ATPU_CHECK(seg_blocks >= 1 && seg_blocks <= nblocks && parts >= 1 && parts <= kSimMaxSplits,
             "hamming_scan: seg_blocks must be in [1, ceil(N / 64)] and parts in [1, 256]");
  const int64_t items = (int64_t)((nblocks + seg_blocks - 1) / seg_blocks) * parts;
  ATPU_CHECK(items <= 2147483647LL && (nq + kHamTile - 1) / kHamTile <= 65535, "hamming_scan: too many workgroups");
  ATPU_CHECK(qbits && codes && ws, "hamming_scan: null tensor");
  ATPU_CHECK(((reinterpret_cast<uintptr_t>(qbits) | reinterpret_cast<uintptr_t>(codes)) & 3) == 0 &&
                 (reinterpret_cast<uintptr_t>(ws) & 7) == 0,
             "hamming_scan: the words must be 4-byte and the workspace 8-byte aligned");
  const int W = D >> 5;
  float2* w = reinterpret_cast<float2*>(ws);
  if (W <= 8) ham_dispatch<8>(qbits, codes, w, nq, N, W, k, nblocks, seg_blocks, parts, (int)items, stream);
  else if (W <= 16) ham_dispatch<16>(qbits, codes, w, nq, N, W, k, nblocks, seg_blocks, parts, (int)items, stream);
  else if (W <= 24) ham_dispatch<24>(qbits, codes, w, nq, N, W, k, nblocks, seg_blocks, parts, (int)items, stream);
  else ham_dispatch<32>(qbits, codes, w, nq, N, W, k, nblocks, seg_blocks, parts, (int)items, stream);
}

}  // namespace atpu
