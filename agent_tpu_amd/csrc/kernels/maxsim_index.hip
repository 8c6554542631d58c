// MaxSim against a resident token-vector index: the passage-stationary twin of maxsim.hip.
//   score(q, p) = sum_{i < len_q} max_{j < len_p} <Q[q, i], tok[off[p] + j]>,
// exact fp32 on v_mfma_f32_16x16x4_f32. The index is tok [T, P], the live unit token vectors of all
// passages back to back (fp16 or fp32, no padding rows), and off [N + 1] int64.
//
// maxsim_index_kernel<F16>: one workgroup of up to four waves owns a work item, passage pidx[m] (m itself
// without pidx). The passage's tokens go from HBM into LDS once, as stored, and every query that wants
// the item is scored against them: in the all form the queries blockIdx.y * 32 .. + 31 of [0, Qn)
// (out [Qn, M], query-major), in the list form the entries e in [qoff[m], qoff[m + 1]) with query
// qsel[e] (out [E]). Wave w takes the item's queries w, w + nw, ...: a query belongs to one wave, so after
// the passage is on chip there is no barrier and no exchange between waves.
//
// A wave walks its query's tokens i < len_q in tiles of 16. The tile is the B operand, read from
// global memory (a few KiB per query, L2-resident) once per k chunk; the passage's 16-row tiles are the
// A operand, read from LDS, one accumulator (4 registers) per row tile, up to 8 of them in flight: in
// the C/D layout col = lane & 15 is the query token and row = (lane >> 4) * 4 + reg the passage token.
// The max over the passage tokens is taken on the accumulator registers by select (row < len), the four
// lane groups meet by xor16 / xor32, and the wave adds the 16 maxima in increasing token index by
// readlane: ((m0 + m1) + m2) + ... in fp32, maxsim.hip's sum.
//
// k order of one dot product, a function of P and the storage dtype alone, one accumulator per
// (query token, passage token):
//   fp32: maxsim.hip's. Chunks of 16 columns ascending; lane (r = lane & 15, g = lane >> 4) holds
//         row r's columns 16 ch + 4 g .. + 3 and MFMA j of the chunk takes element j. An fp32 index has
//         the bits of ops.maxsim on the padded tensors.
//   fp16: sim_topk_f16.hip's. Chunks of 32 columns ascending; the lane holds the 16 bytes of columns
//         32 cp + 8 g .. + 7, widened to fp32 in registers (exact), and MFMA j = 0 .. 7 takes element j.
//
// LDS image: the rows as stored, row stride P * sizeof(elem) + 16 bytes. Of the 16 lanes that a
// ds_read_b128 serves together (8 rows of one g and the 8 other rows of the next g) two can meet on
// one 16-byte slot with this stride: at most one extra LDS cycle per read, against the 128 to 256 MFMA
// cycles that a read feeds, so the image is not permuted.
//
// On-chip capacity: mi_tile_rows(P) rows, a multiple of 16 that fits 96 KiB, at most 128 (P = 1024
// fp32: 16 rows; P = 128 fp16: 128). A longer passage is walked in tiles of that many tokens: the
// running max of every token of the wave's query is carried in LDS (rmax [wave][S]) from tile to tile
// (max is order-free; every accumulator starts at +0.0, so no dot product is -0.0 and +-0 ties do not
// exist). Such a passage is fetched once per group of nw queries; one that fits, once per workgroup.
//
// Device data is clamped before it forms an address (rerank.hip's rule): pidx into [0, N), qsel into
// [0, Qn), qoff into [0, E] and monotone, lens_q into [1, S], the passage's start into [0, T), its length
// off[p + 1] - off[p] into [1, T - start]. Rows that a 16-row tile holds past the passage's end are
// rows min(row, T - 1) of tok (a neighbour's, with no padding in the index) and query rows past S
// repeat row S - 1: their dot products are discarded by select, never multiplied by 0, and an MFMA
// output depends on its own A row and B column only, so NaN there reaches no score. Nothing outside
// the given tensors is read. A score is a function of its own query rows, passage rows and lengths.
#include "atpu/common.h"
#include "atpu/kernels.h"

namespace atpu {
namespace {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef const __attribute__((address_space(1))) float* mi_gfloat;  // a global pointer across a call: global_load, not flat
typedef const __attribute__((address_space(1))) f32x4* mi_gf32x4;

constexpr int kMiThreads = 256;
constexpr int kMiMaxTiles = 8;            // 16-row tiles of one on-chip passage tile
constexpr int kMiQChunk = 32;             // queries of one workgroup in the all form
constexpr int kMiLdsBudget = 96 * 1024;   // bytes of passage rows on chip

__host__ __device__ inline int mi_row_bytes(int P, bool f16) { return P * (f16 ? 2 : 4) + 16; }

int mi_tile_rows(int P, bool f16) {
  const int rows = (kMiLdsBudget / mi_row_bytes(P, f16)) & ~15;
  return rows < 16 ? 16 : (rows > 16 * kMiMaxTiles ? 16 * kMiMaxTiles : rows);
}

__device__ __forceinline__ int mi_clamp(int x, int lo, int hi) { return min(max(x, lo), hi); }
__device__ __forceinline__ long long mi_clampl(long long x, long long lo, long long hi) {
  return x < lo ? lo : (x > hi ? hi : x);
}

// The lane's max over the live rows of NT on-chip row tiles for query token (lane & 15) of the tile at
// qrow (the lane's own query row, + 4 g floats for fp32, + 8 g for fp16). A call, not inlined: with the
// eight forms inlined into one kernel the scalar registers spill (65 of them); as calls nothing does.
template <bool F16, int NT>
__device__ __noinline__ float mi_tile_max(const unsigned char* __restrict__ lds, int rb, mi_gfloat qrow, int P, int rows,
                                          int r, int g) {
  f32x4 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  if (F16) {
    const unsigned char* a0 = lds + r * rb + 16 * g;
    for (int cp = 0; cp < (P >> 5); ++cp) {
      const f32x4 b0 = *(mi_gf32x4)(qrow + 32 * cp);
      const f32x4 b1 = *(mi_gf32x4)(qrow + 32 * cp + 4);
      f16x8 a[NT];
#pragma unroll
      for (int t = 0; t < NT; ++t) a[t] = *reinterpret_cast<const f16x8*>(a0 + t * 16 * rb + 64 * cp);
#pragma unroll
      for (int j = 0; j < 8; ++j)
#pragma unroll
        for (int t = 0; t < NT; ++t)
          acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32((float)a[t][j], j < 4 ? b0[j & 3] : b1[j & 3], acc[t], 0, 0, 0);
    }
  } else {
    const unsigned char* a0 = lds + r * rb + 16 * g;
    for (int ch = 0; ch < (P >> 4); ++ch) {
      const f32x4 b = *(mi_gf32x4)(qrow + 16 * ch);
      f32x4 a[NT];
#pragma unroll
      for (int t = 0; t < NT; ++t) a[t] = *reinterpret_cast<const f32x4*>(a0 + t * 16 * rb + 64 * ch);
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t][j], b[j], acc[t], 0, 0, 0);
    }
  }
  float m = -__builtin_inff();
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int e = 0; e < 4; ++e) m = fmaxf(m, t * 16 + g * 4 + e < rows ? acc[t][e] : -__builtin_inff());
  return m;
}

template <bool F16>
__global__ __launch_bounds__(kMiThreads) void maxsim_index_kernel(
    const float* __restrict__ qv, const int32_t* __restrict__ lens_q, const unsigned char* __restrict__ tok,
    const int64_t* __restrict__ off, const int32_t* __restrict__ pidx, const int32_t* __restrict__ qoff,
    const int32_t* __restrict__ qsel, float* __restrict__ out, int Qn, int S, int P, long long T, int N, int M, int E,
    int TR) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nw = blockDim.x >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int m = blockIdx.x;
  const int rb = mi_row_bytes(P, F16);
  const int esz = F16 ? 2 : 4;
  float* rmax = reinterpret_cast<float*>(smem + (size_t)TR * rb) + wave * S;  // this wave's [S]
  const bool list = qoff != nullptr;

  // device data: clamped before it forms an address
  const int pi = pidx ? mi_clamp(pidx[m], 0, N - 1) : m;
  const long long o0 = off[pi], o1 = off[pi + 1];
  const long long start = mi_clampl(o0, 0, T - 1);
  const long long len = mi_clampl((long long)((unsigned long long)o1 - (unsigned long long)o0), 1, T - start);
  int lo, hi;
  if (list) {
    lo = mi_clamp(qoff[m], 0, E);
    hi = mi_clamp(qoff[m + 1], lo, E);
  } else {
    lo = blockIdx.y * kMiQChunk;
    hi = min(Qn, lo + kMiQChunk);
  }
  if (lo >= hi) return;  // uniform over the workgroup: an empty item does nothing
  const bool multi = len > TR;
  const int pieces = (P * esz) >> 4;  // 16-byte pieces of a row

  for (int base = lo; base < hi; base += nw) {  // uniform
    const int u = base + wave;
    const bool have = u < hi;  // wave-uniform
    int qi = 0, lq = 1;
    if (have) {
      qi = list ? mi_clamp(qsel[u], 0, Qn - 1) : u;
      lq = mi_clamp(lens_q[qi], 1, S);
    }
    const float* q = qv + (size_t)qi * S * P + (F16 ? 8 : 4) * g;
    float sum = 0.f;
    for (long long t0 = 0; t0 < len; t0 += TR) {  // uniform
      const int rows = (int)(len - t0 < TR ? len - t0 : TR);
      const int nt = (rows + 15) >> 4;
      if (multi || base == lo) {
        if (multi && !(base == lo && t0 == 0)) __syncthreads();  // every read of the previous tile is done
        for (int i = tid; i < nt * 16 * pieces; i += blockDim.x) {
          const int row = i / pieces, c = i - row * pieces;
          const long long gr = min(start + t0 + row, T - 1);  // past the passage: a row of tok, discarded by select
          *reinterpret_cast<f32x4*>(smem + row * rb + c * 16) =
              *reinterpret_cast<const f32x4*>(tok + ((size_t)gr * P) * esz + c * 16);
        }
        __syncthreads();
      }
      if (!have) continue;
      const bool first = t0 == 0, last = t0 + TR >= len;
      for (int i0 = 0; i0 < lq; i0 += 16) {
        const int ti = min(i0 + r, S - 1);  // query rows past S repeat the last row; tokens >= len_q are not added
        const mi_gfloat qrow = (mi_gfloat)(q + (size_t)ti * P);
        float mm;
        switch (nt) {
          case 1: mm = mi_tile_max<F16, 1>(smem, rb, qrow, P, rows, r, g); break;
          case 2: mm = mi_tile_max<F16, 2>(smem, rb, qrow, P, rows, r, g); break;
          case 3: mm = mi_tile_max<F16, 3>(smem, rb, qrow, P, rows, r, g); break;
          case 4: mm = mi_tile_max<F16, 4>(smem, rb, qrow, P, rows, r, g); break;
          case 5: mm = mi_tile_max<F16, 5>(smem, rb, qrow, P, rows, r, g); break;
          case 6: mm = mi_tile_max<F16, 6>(smem, rb, qrow, P, rows, r, g); break;
          case 7: mm = mi_tile_max<F16, 7>(smem, rb, qrow, P, rows, r, g); break;
          default: mm = mi_tile_max<F16, 8>(smem, rb, qrow, P, rows, r, g); break;
        }
        mm = fmaxf(mm, xor16f(mm));
        mm = fmaxf(mm, xor32f(mm));
        if (!first) mm = fmaxf(mm, rmax[ti]);  // written before the barriers of this tile's load
        if (!last) {
          if (g == 0 && i0 + r < S) rmax[ti] = mm;
        } else {
          const int cnt = min(16, lq - i0);
#pragma unroll
          for (int i = 0; i < 16; ++i)  // increasing token index, left to right
            if (i < cnt) sum += __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, mm), i));
        }
      }
      if (last && lane == 0) out[list ? (size_t)u : (size_t)qi * M + m] = sum;
    }
  }
}

}  // namespace

void maxsim_index(const float* qv, const int32_t* lens_q, const void* tok, const int64_t* off, const int32_t* pidx,
                  const int32_t* qoff, const int32_t* qsel, float* out, int Qn, int S, int P, int64_t T, int N, int M, int E,
                  int is_f16, hipStream_t stream) {
  ATPU_CHECK(P % 64 == 0 && P >= 64 && P <= 1024, "maxsim_index: P must be a multiple of 64 in [64, 1024]");
  ATPU_CHECK(S >= 1 && Qn >= 1 && N >= 1 && T >= 1 && M >= 0 && E >= 0,
             "maxsim_index: S, Qn, N and T must be >= 1");
  ATPU_CHECK((qoff == nullptr) == (qsel == nullptr) || E == 0, "maxsim_index: qoff and qsel come together");
  ATPU_CHECK(pidx || M == N, "maxsim_index: without pidx M must be N");
  if (M == 0) return;
  ATPU_CHECK(qv && lens_q && tok && off && out, "maxsim_index: null tensor");
  ATPU_CHECK(((reinterpret_cast<uintptr_t>(qv) | reinterpret_cast<uintptr_t>(tok)) & 15) == 0,
             "maxsim_index: qv and tok must be 16-byte aligned");
  const bool f16 = is_f16 != 0, list = qoff != nullptr;
  const int TR = mi_tile_rows(P, f16);
  const int nw = list ? 4 : (Qn < 4 ? Qn : 4);
  const size_t lds = (size_t)TR * mi_row_bytes(P, f16) + (size_t)nw * S * sizeof(float);
  ATPU_CHECK(lds <= 160 * 1024, "maxsim_index: S too large for the running-max rows");
  const dim3 grid(M, list ? 1 : (Qn + kMiQChunk - 1) / kMiQChunk);
  // up to 96 KiB of passage rows; the attribute is per device
  if (f16) {
    ATPU_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&maxsim_index_kernel<true>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL((maxsim_index_kernel<true>), grid, dim3(64 * nw), lds, stream, qv, lens_q,
                       static_cast<const unsigned char*>(tok), off, pidx, qoff, qsel, out, Qn, S, P, (long long)T, N, M, E,
                       TR);
  } else {
    ATPU_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&maxsim_index_kernel<false>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL((maxsim_index_kernel<false>), grid, dim3(64 * nw), lds, stream, qv, lens_q,
                       static_cast<const unsigned char*>(tok), off, pidx, qoff, qsel, out, Qn, S, P, (long long)T, N, M, E,
                       TR);
  }
  ATPU_HIP_CHECK(hipGetLastError());
}

}  // namespace atpu
