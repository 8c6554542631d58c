// Inverted index over learned sparse (SPLADE) term weights, and its top-k scan.
//
// Layout. Rows are cut into blocks of kSparseBlockRows = 8192 consecutive rows; inside a block the postings are
// grouped by token. A posting is one 32-bit word: low 16 bits = row - block_base, high 16 bits = the fp16 bits of
// the weight (rounded to nearest even from the fp32 input, once). offsets [nblocks, V + 1] int32 are relative to
// the block's start, block_start [nblocks + 1] int64 is where a block's postings begin. The order of the postings
// of one (block, token) segment is whatever the atomics gave: integer sums make every result independent of it.
//
// Score. For a term shared by query and row, c = rint(double(wq) * double(wd) * 2^32) as int64 (the product is
// exact in fp64, the rint is the only rounding); a row's acc is the integer sum of its c, which has no order;
// score = float(acc) * 2^-32. A row is a hit if acc > 0. A plain int64 CPU computation gives the same bits.
//
// postings_build_kernel<FILL> (postings_count / postings_fill): one wave per row of a block given as CSR. A lane takes one entry
// per step, rounds its weight to fp16 and drops it if that is zero; count adds 1 to counts[token], fill takes
// the slot cursor[token]++ (cursor starts as the exclusive scan of the counts, which the host makes) and writes
// the word with a vector store.
//
// sparse_scan_kernel<KM>: grid (items, nq), 8 waves. A workgroup owns one query and walks the blocks
// b = item, item + items, ...; its top-k lists carry across them. LDS holds kSparseBlockRows int64 accumulators
// (64 KiB). Per block: thread j loads the two offsets of the query's term j (at most 1024 terms) into a segment
// table; segments are cut into chunks of 256 postings and an LDS prefix sum over the chunk counts numbers the
// block's chunks. Waves take chunks round-robin and find a chunk's term by a wave-uniform binary search over
// the prefix, so a token present in every row does not serialise one wave and short segments do not idle seven.
// A lane loads one posting per step (256 B contiguous per wave), forms c and does one 64-bit integer LDS atomic
// add to acc[row]. After a barrier one pass reads every accumulator and writes zero back (the next block starts
// clean); a nonzero one becomes the candidate (score, block_base + row) for the wave's sorted list of KM >= k
// entries in LDS, gated by a ballot against the list's bar (wave_list_insert of atpu/topk.h). After the last
// block the 8 wave lists are merged into ws [nq, items, k]; every slot is written, empty ones hold
// (-inf, 0x7fffffff), and sim_topk_merge reduces the items. No floating-point atomic anywhere.
//
// LDS: 64 KiB accumulators + 2 x 4 KiB segment table + 4 KiB prefix + 8 KM x 8 B lists = 78 KiB at KM = 32, so two
// workgroups share a CU's 160 KiB. The query weight of a chunk's term is one wave-uniform global read.
//
// Every index is clamped before it forms an address and discarded by select: token ids to [0, V), segment
// bounds to the block's postings, the block's postings to [0, total), the row of a word to the block (masked: the block size is a power of two). Nothing
// outside the postings, the offsets, block_start, the query arrays and ws is touched.
#include "atpu/common.h"
#include "atpu/kernels.h"
#include "atpu/topk.h"

namespace atpu {
namespace {

constexpr int kNoRow = 0x7fffffff;
constexpr int kBuildWaves = 4, kBuildThreads = kBuildWaves * kWave;
constexpr int kScanWaves = 8, kScanThreads = kScanWaves * kWave;
constexpr int kChunk = 256;  // postings of one wave's unit of work: 4 steps of 64
constexpr int kMaxTerms = kSparseMaxTerms;
constexpr int kR = kSparseBlockRows;
static_assert(kMaxTerms == 2 * kScanThreads, "two query terms per thread");
static_assert(kR % kScanThreads == 0 && kR <= 65536 && (kR & (kR - 1)) == 0,
              "a row of a block is the low 16 bits of a word, masked to the block: a power of two");

__device__ __forceinline__ uint32_t half_bits(float w) {
  return (uint32_t) __builtin_bit_cast(unsigned short, (_Float16)w);  // round to nearest even
}

template <bool FILL>
__global__ __launch_bounds__(kBuildThreads) void postings_build_kernel(const int64_t* __restrict__ indptr,
                                                                       const int32_t* __restrict__ indices,
                                                                       const float* __restrict__ data,
                                                                       int32_t* __restrict__ slots,
                                                                       uint32_t* __restrict__ out, int rows, int V,
                                                                       int64_t nnz, int cap) {
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r = blockIdx.x * kBuildWaves + wave;
  if (r >= rows) return;  // wave-uniform
  const int64_t lo = max((int64_t)0, min(indptr[r], nnz)), hi = max(lo, min(indptr[r + 1], nnz));
  for (int64_t e0 = lo; e0 < hi; e0 += kWave) {
    const int64_t e = e0 + lane;
    const bool live = e < hi;
    const int tok = indices[live ? e : lo];
    const uint32_t h = half_bits(data[live ? e : lo]);
    if (live && h != 0u && tok >= 0 && tok < V) {
      const int slot = atomicAdd(&slots[tok], 1);
      if (FILL && slot >= 0 && slot < cap) out[slot] = (h << 16) | (uint32_t)r;
    }
  }
}

template <int KM>
__global__ __launch_bounds__(kScanThreads) void sparse_scan_kernel(
    const uint32_t* __restrict__ postings, const int32_t* __restrict__ offsets, const int64_t* __restrict__ block_start,
    const int64_t* __restrict__ q_ptr, const int32_t* __restrict__ q_tok, const float* __restrict__ q_w,
    float2* __restrict__ ws, int V, int nblocks, int64_t total, int64_t nterms, int k) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  long long* acc = reinterpret_cast<long long*>(smem);  // [kR]
  int* seg_lo = reinterpret_cast<int*>(acc + kR);       // [kMaxTerms]
  int* seg_hi = seg_lo + kMaxTerms;                     // [kMaxTerms]
  int* pre = seg_hi + kMaxTerms;                        // [kMaxTerms + 2]: chunks before term j; pre[kMaxTerms] = all
  float2* lists = reinterpret_cast<float2*>(pre + kMaxTerms + 2);  // [kScanWaves][KM]
  __shared__ int wtot[kScanWaves];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int item = blockIdx.x, qi = blockIdx.y;

  const int64_t t0 = max((int64_t)0, min(q_ptr[qi], nterms));
  const int nt = (int)max((int64_t)0, min(min(q_ptr[qi + 1], nterms) - t0, (int64_t)kMaxTerms));
  for (int i = tid; i < kR; i += kScanThreads) acc[i] = 0;
  for (int i = tid; i < kScanWaves * KM; i += kScanThreads) lists[i] = float2{-__builtin_inff(), __int_as_float(kNoRow)};
  int tok[2];
  bool ok[2];
#pragma unroll
  for (int e = 0; e < 2; ++e) {  // the thread's two terms, for every block
    const int j = 2 * tid + e;
    const int t = nt > 0 ? q_tok[t0 + min(j, nt - 1)] : 0;
    ok[e] = j < nt && t >= 0 && t < V;
    tok[e] = ok[e] ? t : 0;
  }
  float2* wl = lists + wave * KM;

  for (int b = item; b < nblocks && nt > 0; b += gridDim.x) {
    const int64_t bs = max((int64_t)0, min(block_start[b], total));
    const int bn = (int)max((int64_t)0, min(min(block_start[b + 1], total) - bs, (int64_t)1 << 23));
    const int32_t* off = offsets + (size_t)b * (V + 1);
    int cnt[2];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int lo = max(0, min(off[tok[e]], bn));
      const int hi = ok[e] ? max(lo, min(off[tok[e] + 1], bn)) : lo;
      seg_lo[2 * tid + e] = lo;
      seg_hi[2 * tid + e] = hi;
      cnt[e] = (hi - lo + kChunk - 1) / kChunk;
    }
    // exclusive prefix of the chunk counts: wave scan, then the 8 wave totals
    const int s = cnt[0] + cnt[1];
    int incl = s;
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
      const int o = __shfl_up(incl, d);
      incl += lane >= d ? o : 0;
    }
    if (lane == kWave - 1) wtot[wave] = incl;
    __syncthreads();  // also: the previous block's drain is over
    int base = 0, T = 0;
#pragma unroll
    for (int w = 0; w < kScanWaves; ++w) {
      const int x = wtot[w];
      base += w < wave ? x : 0;
      T += x;
    }
    pre[2 * tid] = base + incl - s;
    pre[2 * tid + 1] = base + incl - s + cnt[0];
    if (tid == kScanThreads - 1) pre[kMaxTerms] = T;
    T = __builtin_amdgcn_readfirstlane(T);
    __syncthreads();
    if (T == 0) continue;  // workgroup-uniform: the accumulators are still zero

    for (int c = wave; c < T; c += kScanWaves) {
      int lo = 0, hi = kMaxTerms;  // pre[lo] <= c < pre[hi]; a term without chunks is never the answer
#pragma unroll
      for (int it = 0; it < 10; ++it) {
        const int mid = (lo + hi) >> 1;
        const bool le = pre[mid] <= c;  // one address for the wave: a broadcast
        lo = le ? mid : lo;
        hi = le ? hi : mid;
      }
      const int t = __builtin_amdgcn_readfirstlane(lo);
      const int p0 = __builtin_amdgcn_readfirstlane(seg_lo[t] + (c - pre[t]) * kChunk);
      const int p1 = __builtin_amdgcn_readfirstlane(min(p0 + kChunk, seg_hi[t]));  // p0 < p1 <= bn
      const double wq = (double)q_w[t0 + t] * 4294967296.0;  // exact: a power of two
#pragma unroll
      for (int st = 0; st < kChunk / kWave; ++st) {
        const int p = p0 + st * kWave + lane;
        const bool live = p < p1;
        const uint32_t word = postings[bs + (live ? p : p0)];
        const double wd = (double)(float)__builtin_bit_cast(_Float16, (unsigned short)(word >> 16));
        const long long cc = __double2ll_rn(wq * wd);
        if (live)
          atomicAdd(reinterpret_cast<unsigned long long*>(acc + (word & (kR - 1))), (unsigned long long)cc);
      }
    }
    __syncthreads();

    // drain: read and clear, candidates into the wave's list
    const int row0 = b * kR;
    for (int i = tid; i < kR; i += kScanThreads) {
      const long long a = acc[i];
      acc[i] = 0;
      const float v[1] = {a > 0 ? __ll2float_rn(a) * 0x1p-32f : -__builtin_inff()};
      const int id[1] = {a > 0 ? row0 + i : kNoRow};
      const float2 bar = wl[KM - 1];
      if (__ballot(better(v[0], id[0], bar.x, __float_as_int(bar.y))) != 0) wave_list_insert<KM, 1>(wl, lane, v, id);
    }
  }
  __syncthreads();

  // wave 0: 8 lanes, one wave list each; k rounds of best head, the owner pops (rows are distinct)
  if (tid < kWave) {
    const float2* mine = lists + (tid & (kScanWaves - 1)) * KM;
    float2* dst = ws + ((size_t)qi * gridDim.x + item) * k;
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
      if (tid == 0) dst[n] = float2{bv, __int_as_float(bi)};
    }
  }
}

size_t scan_lds_bytes(int KM) {
  return (size_t)kR * sizeof(long long) + (size_t)(3 * kMaxTerms + 2) * sizeof(int) +
         (size_t)kScanWaves * KM * sizeof(float2);
}

template <int KM>
void scan_launch(const uint32_t* postings, const int32_t* offsets, const int64_t* block_start, const int64_t* q_ptr,
                 const int32_t* q_tok, const float* q_w, float2* ws, int nq, int V, int nblocks, int64_t total,
                 int64_t nterms, int k, int items, hipStream_t stream) {
  const size_t lds = scan_lds_bytes(KM);  // above the 64 KiB default; the attribute is per device
  ATPU_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&sparse_scan_kernel<KM>),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL((sparse_scan_kernel<KM>), dim3(items, nq), dim3(kScanThreads), lds, stream, postings, offsets,
                     block_start, q_ptr, q_tok, q_w, ws, V, nblocks, total, nterms, k);
  ATPU_HIP_CHECK(hipGetLastError());
}

void check_block(const char* what, const void* indptr, const void* indices, const void* data, const void* slots, int rows,
                 int V, int64_t nnz) {
  ATPU_CHECK(rows >= 1 && rows <= kR, std::string(what) + ": rows of a block must be in [1, 8192]");
  ATPU_CHECK(V >= 1 && V < 2147483647 && nnz >= 1, std::string(what) + ": V and nnz must be >= 1");
  ATPU_CHECK(indptr && indices && data && slots, std::string(what) + ": null tensor");
  ATPU_CHECK((reinterpret_cast<uintptr_t>(indptr) & 7) == 0 &&
                 ((reinterpret_cast<uintptr_t>(indices) | reinterpret_cast<uintptr_t>(data) |
                   reinterpret_cast<uintptr_t>(slots)) & 3) == 0,
             std::string(what) + ": indptr must be 8-byte, the other tensors 4-byte aligned");
}

}  // namespace

void postings_count(const int64_t* indptr, const int32_t* indices, const float* data, int32_t* counts, int rows, int V,
                    int64_t nnz, hipStream_t stream) {
  check_block("postings_count", indptr, indices, data, counts, rows, V, nnz);
  hipLaunchKernelGGL(postings_build_kernel<false>, dim3((rows + kBuildWaves - 1) / kBuildWaves), dim3(kBuildThreads), 0,
                     stream, indptr, indices, data, counts, static_cast<uint32_t*>(nullptr), rows, V, nnz, 0);
  ATPU_HIP_CHECK(hipGetLastError());
}

void postings_fill(const int64_t* indptr, const int32_t* indices, const float* data, int32_t* cursor, uint32_t* out,
                   int rows, int V, int64_t nnz, int cap, hipStream_t stream) {
  check_block("postings_fill", indptr, indices, data, cursor, rows, V, nnz);
  ATPU_CHECK(out && (reinterpret_cast<uintptr_t>(out) & 3) == 0 && cap >= 1 && cap < (1 << 23),
             "postings_fill: a block holds 1 to 2^23 - 1 postings, 4-byte aligned");
  hipLaunchKernelGGL(postings_build_kernel<true>, dim3((rows + kBuildWaves - 1) / kBuildWaves), dim3(kBuildThreads), 0,
                     stream, indptr, indices, data, cursor, out, rows, V, nnz, cap);
  ATPU_HIP_CHECK(hipGetLastError());
}

void sparse_scan_partial(const uint32_t* postings, const int32_t* offsets, const int64_t* block_start,
                         const int64_t* q_ptr, const int32_t* q_tok, const float* q_w, float* ws, int nq, int N, int V,
                         int64_t total, int64_t nterms, int k, int items, hipStream_t stream) {
  ATPU_CHECK(nq >= 1 && nq <= 65535 && N >= 1 && N <= 2147483647 - 256,
             "sparse_scan: nq in [1, 65535] and N in [1, 2^31 - 256]");
  ATPU_CHECK(V >= 1 && V < 2147483647 && total >= 1 && nterms >= 1, "sparse_scan: V, postings and query terms >= 1");
  ATPU_CHECK(k >= 1 && k <= 32, "sparse_scan: k must be in [1, 32]");
  const int nblocks = (N + kR - 1) / kR;
  ATPU_CHECK(items >= 1 && items <= kSimMaxSplits && items <= nblocks,
             "sparse_scan: items must be in [1, min(256, ceil(N / 8192))]");
  ATPU_CHECK(postings && offsets && block_start && q_ptr && q_tok && q_w && ws, "sparse_scan: null tensor");
  ATPU_CHECK(((reinterpret_cast<uintptr_t>(postings) | reinterpret_cast<uintptr_t>(offsets) |
               reinterpret_cast<uintptr_t>(q_tok) | reinterpret_cast<uintptr_t>(q_w)) & 3) == 0 &&
                 ((reinterpret_cast<uintptr_t>(block_start) | reinterpret_cast<uintptr_t>(q_ptr) |
                   reinterpret_cast<uintptr_t>(ws)) & 7) == 0,
             "sparse_scan: 32-bit tensors must be 4-byte, 64-bit tensors and the workspace 8-byte aligned");
  float2* w = reinterpret_cast<float2*>(ws);
  if (k <= 8)
    scan_launch<8>(postings, offsets, block_start, q_ptr, q_tok, q_w, w, nq, V, nblocks, total, nterms, k, items, stream);
  else if (k <= 16)
    scan_launch<16>(postings, offsets, block_start, q_ptr, q_tok, q_w, w, nq, V, nblocks, total, nterms, k, items, stream);
  else
    scan_launch<32>(postings, offsets, block_start, q_ptr, q_tok, q_w, w, nq, V, nblocks, total, nterms, k, items, stream);
}

}  // namespace atpu
