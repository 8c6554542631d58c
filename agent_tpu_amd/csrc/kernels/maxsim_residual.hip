// MaxSim against a residual-compressed token-vector index (ColBERTv2's stored form), and its encoder.
// A token is the id of its nearest centroid and b = 1, 2 or 4 bits per dimension:
//   v[d] = centroids[cid][d] + weights[code[d]]          one fp32 add, no renormalisation,
// code[d] in byte d * b / 8 of the token's P * b / 8 code bytes at bits (d * b) % 8 .. + b - 1, low bits first.
//
// maxsim_index_rc_kernel<B>: the twin of maxsim_index_kernel<false> (maxsim_index.hip). The grid, the
// wave-per-query split, the multi-tile walk with rmax, the fp32 LDS image with its row stride, the MFMA walk
// (mi_tile_max<false, NT>) and the summation are that kernel's, so a score has the bits of maxsim_index on
// the decoded fp32 rows. Only the stage that fills the image differs: the passage is decompressed while it
// is brought on chip, once per workgroup (once per group of nw queries for a passage longer than the
// tile), and the decoded rows never exist in HBM.
//
// The fill, two steps with a barrier between them.
//   A. stage: the tile's code bytes go from HBM into LDS as stored, in 8-byte loads (P * b / 8 is a
//      multiple of 8). Consecutive threads take consecutive 8-byte words of consecutive rows, and the rows
//      of a passage are consecutive in the file: one contiguous stream, every byte read once. The first
//      threads also stage the tile's centroid ids, clamped into [0, K), and the 2^b bucket weights.
//   B. decode: thread i takes 16-byte piece c = i % (P / 4) of row i / (P / 4), the mapping of the
//      uncompressed kernel's copy loop. It reads the row's id and the piece's 4 b code bits from LDS (one
//      aligned 32-bit word, shifted), the centroid's piece c from global memory, adds the four weights
//      looked up in LDS and writes the piece into the image. Consecutive threads read consecutive 16 bytes
//      of a centroid row (P / 4 >= 16 threads per row: whole 256-byte runs of the table, which at K <= 4096
//      stays in L2) and write consecutive 16 bytes of the image, the conflict-free ds_write_b128 pattern.
//      The 16 weights sit in 16 different banks and equal indices broadcast, so the lookups do not
//      conflict either. Mapping a thread to a code word instead (4 pieces at b = 2) would stride both the
//      centroid reads and the image writes by 64 bytes; staging the codes costs at most 12 KiB of LDS and
//      one barrier per tile and keeps all three streams contiguous.
//
// LDS: the image [TR rows, stride 4 P + 16] and rmax [nw][S] where the uncompressed kernel has them, then
// the staged codes [TR][P b / 8], the ids [TR] and the weights [16].
//
// Device data is clamped before it forms an address, as in maxsim_index.hip; in addition cid into [0, K).
// Rows that a 16-row tile holds past the passage's end repeat row min(row, T - 1) (codes and id) and are
// discarded by select. Nothing outside the given tensors is read.
//
// residual_encode_kernel<B>: thread i takes the 4 dimensions 4 (i % (P / 4)) .. + 3 of row i / (P / 4): one
// 16-byte load of x and one of the row's centroid (id clamped), r = x - c in one fp32 subtraction, the code
// the number of cutoffs strictly below r. The 8 / b lanes that share a 32-bit code word shift their 4 b
// bits into place and meet by xor shuffles; the first of them stores the word. P / 4 is a multiple of 16,
// so a word's lanes are in one row and one wave.
#include "atpu/common.h"
#include "atpu/kernels.h"
#include "atpu/maxsim_tile.h"

namespace atpu {
namespace {

typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

__host__ __device__ inline int rc_code_bytes(int P, int b) { return P * b >> 3; }
// rmax [nw][S] rounded up to 16 bytes: the staged codes behind it are stored in 8-byte pieces
__host__ __device__ inline size_t rc_rmax_bytes(int nw, int S) { return ((size_t)nw * S * sizeof(float) + 15) & ~(size_t)15; }

template <int B>
__global__ __launch_bounds__(kMiThreads) void maxsim_index_rc_kernel(
    const float* __restrict__ qv, const int32_t* __restrict__ lens_q, const unsigned char* __restrict__ codes,
    const int32_t* __restrict__ cid, const float* __restrict__ cent, const float* __restrict__ weights,
    const int64_t* __restrict__ off, const int32_t* __restrict__ pidx, const int32_t* __restrict__ qoff,
    const int32_t* __restrict__ qsel, float* __restrict__ out, int Qn, int S, int P, long long T, int K, int N, int M,
    int E, int TR) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nw = blockDim.x >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int m = blockIdx.x;
  const int rb = mi_row_bytes(P, false);
  const int cb = rc_code_bytes(P, B);
  float* rmax = reinterpret_cast<float*>(smem + (size_t)TR * rb) + wave * S;  // this wave's [S]
  unsigned char* scode = smem + (size_t)TR * rb + rc_rmax_bytes(nw, S);  // [TR][cb], 16-byte aligned
  int* scid = reinterpret_cast<int*>(scode + (size_t)TR * cb);                     // [TR]
  float* sw = reinterpret_cast<float*>(scid + TR);                                 // [16]
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
  const int pieces = P >> 2;  // 16-byte pieces of a decoded row
  const int words = cb >> 3;  // 8-byte words of a row's codes
  if (tid < (1 << B)) sw[tid] = weights[tid];  // visible after the first fill's barrier

  for (int base = lo; base < hi; base += nw) {  // uniform
    const int u = base + wave;
    const bool have = u < hi;  // wave-uniform
    int qi = 0, lq = 1;
    if (have) {
      qi = list ? mi_clamp(qsel[u], 0, Qn - 1) : u;
      lq = mi_clamp(lens_q[qi], 1, S);
    }
    const float* q = qv + (size_t)qi * S * P + 4 * g;
    float sum = 0.f;
    for (long long t0 = 0; t0 < len; t0 += TR) {  // uniform
      const int rows = (int)(len - t0 < TR ? len - t0 : TR);
      const int nt = (rows + 15) >> 4;
      if (multi || base == lo) {
        if (multi && !(base == lo && t0 == 0)) __syncthreads();  // every read of the previous tile is done
        // A: the codes as stored, the clamped ids
        for (int i = tid; i < nt * 16 * words; i += blockDim.x) {
          const int row = i / words, w = i - row * words;
          const long long gr = min(start + t0 + row, T - 1);  // past the passage: a row of the index, discarded by select
          *reinterpret_cast<u32x2*>(scode + row * cb + w * 8) =
              *reinterpret_cast<const u32x2*>(codes + (size_t)gr * cb + w * 8);
        }
        for (int row = tid; row < nt * 16; row += blockDim.x)
          scid[row] = mi_clamp(cid[min(start + t0 + row, T - 1)], 0, K - 1);
        __syncthreads();
        // B: centroid piece + bucket weights -> the fp32 image
        for (int i = tid; i < nt * 16 * pieces; i += blockDim.x) {
          const int row = i / pieces, c = i - row * pieces;
          const f32x4 ce = *reinterpret_cast<const f32x4*>(cent + (size_t)scid[row] * P + 4 * c);
          const int bit = 4 * B * c;  // of the row's codes; 4 B bits never straddle a 32-bit word
          const unsigned bits = *reinterpret_cast<const unsigned*>(scode + row * cb + ((bit >> 5) << 2)) >> (bit & 31);
          f32x4 v;
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = ce[e] + sw[(bits >> (B * e)) & ((1u << B) - 1)];
          *reinterpret_cast<f32x4*>(smem + row * rb + c * 16) = v;
        }
        __syncthreads();
      }
      if (!have) continue;
      const bool first = t0 == 0, last = t0 + TR >= len;
      for (int i0 = 0; i0 < lq; i0 += 16) {
        const int ti = min(i0 + r, S - 1);  // query rows past S repeat the last row; tokens >= len_q are not added
        const mi_gfloat qrow = (mi_gfloat)(q + (size_t)ti * P);
        float mm = mi_tiles_max<false>(nt, smem, rb, qrow, P, rows, r, g);
        mm = fmaxf(mm, xor16f(mm));
        mm = fmaxf(mm, xor32f(mm));
        if (!first) mm = fmaxf(mm, rmax[ti]);  // written before the barriers of this tile's fill
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

template <int B>
__global__ __launch_bounds__(256) void residual_encode_kernel(
    const float* __restrict__ x, const int32_t* __restrict__ cid, const float* __restrict__ cent,
    const float* __restrict__ cutoffs, unsigned* __restrict__ codes, long long total, int P, int K) {
  constexpr int kCut = (1 << B) - 1;
  constexpr int kLanes = 8 / B;  // lanes of one 32-bit code word
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;  // 16-byte piece of x
  const int pieces = P >> 2;
  unsigned word = 0;
  if (i < total) {  // total is a multiple of 16: the lanes of a word are in or out together
    const long long row = i / pieces;
    const int c = (int)(i - row * pieces);
    const f32x4 xv = *reinterpret_cast<const f32x4*>(x + (size_t)i * 4);
    const f32x4 ce = *reinterpret_cast<const f32x4*>(cent + (size_t)mi_clamp(cid[row], 0, K - 1) * P + 4 * c);
    float cut[kCut];
#pragma unroll
    for (int k = 0; k < kCut; ++k) cut[k] = cutoffs[k];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float res = xv[e] - ce[e];
      unsigned code = 0;
#pragma unroll
      for (int k = 0; k < kCut; ++k) code += res > cut[k] ? 1u : 0u;
      word |= code << (B * e);
    }
    word <<= 4 * B * (int)(i & (kLanes - 1));
  }
#pragma unroll
  for (int o = 1; o < kLanes; o <<= 1) word |= (unsigned)__shfl_xor((int)word, o, 64);
  if (i < total && (i & (kLanes - 1)) == 0) codes[i / kLanes] = word;
}

template <int B>
void launch_rc(const float* qv, const int32_t* lens_q, const void* codes, const int32_t* cid, const float* cent,
               const float* weights, const int64_t* off, const int32_t* pidx, const int32_t* qoff, const int32_t* qsel,
               float* out, int Qn, int S, int P, long long T, int K, int N, int M, int E, int TR, int nw, size_t lds,
               dim3 grid, hipStream_t stream) {
  // up to 96 KiB of decoded rows; the attribute is per device
  ATPU_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&maxsim_index_rc_kernel<B>),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL((maxsim_index_rc_kernel<B>), grid, dim3(64 * nw), lds, stream, qv, lens_q,
                     static_cast<const unsigned char*>(codes), cid, cent, weights, off, pidx, qoff, qsel, out, Qn, S, P, T,
                     K, N, M, E, TR);
}

}  // namespace

void maxsim_index_rc(const float* qv, const int32_t* lens_q, const void* codes, const int32_t* cid, const float* centroids,
                     const float* weights, const int64_t* off, const int32_t* pidx, const int32_t* qoff,
                     const int32_t* qsel, float* out, int Qn, int S, int P, int64_t T, int K, int bits, int N, int M, int E,
                     hipStream_t stream) {
  ATPU_CHECK(P % 64 == 0 && P >= 64 && P <= 1024, "maxsim_index_rc: P must be a multiple of 64 in [64, 1024]");
  ATPU_CHECK(bits == 1 || bits == 2 || bits == 4, "maxsim_index_rc: bits must be 1, 2 or 4");
  ATPU_CHECK(K >= 1 && K <= 4096, "maxsim_index_rc: K must be in [1, 4096]");
  ATPU_CHECK(S >= 1 && Qn >= 1 && N >= 1 && T >= 1 && M >= 0 && E >= 0,
             "maxsim_index_rc: S, Qn, N and T must be >= 1");
  ATPU_CHECK((qoff == nullptr) == (qsel == nullptr) || E == 0, "maxsim_index_rc: qoff and qsel come together");
  ATPU_CHECK(pidx || M == N, "maxsim_index_rc: without pidx M must be N");
  if (M == 0) return;
  ATPU_CHECK(qv && lens_q && codes && cid && centroids && weights && off && out, "maxsim_index_rc: null tensor");
  ATPU_CHECK(((reinterpret_cast<uintptr_t>(qv) | reinterpret_cast<uintptr_t>(codes) | reinterpret_cast<uintptr_t>(centroids)) & 15) == 0,
             "maxsim_index_rc: qv, codes and centroids must be 16-byte aligned");
  const bool list = qoff != nullptr;
  const int TR = mi_tile_rows(P, false);
  const int nw = list ? 4 : (Qn < 4 ? Qn : 4);
  const size_t lds = (size_t)TR * mi_row_bytes(P, false) + rc_rmax_bytes(nw, S) +
                     (size_t)TR * rc_code_bytes(P, bits) + (size_t)TR * sizeof(int) + 16 * sizeof(float);
  ATPU_CHECK(lds <= 160 * 1024, "maxsim_index_rc: S too large for the running-max rows");
  const dim3 grid(M, list ? 1 : (Qn + kMiQChunk - 1) / kMiQChunk);
#define ATPU_RC(B)                                                                                                  \
  launch_rc<B>(qv, lens_q, codes, cid, centroids, weights, off, pidx, qoff, qsel, out, Qn, S, P, (long long)T, K, N, M, \
               E, TR, nw, lds, grid, stream)
  if (bits == 1) ATPU_RC(1);
  else if (bits == 2) ATPU_RC(2);
  else ATPU_RC(4);
#undef ATPU_RC
  ATPU_HIP_CHECK(hipGetLastError());
}

void residual_encode(const float* x, const int32_t* cid, const float* centroids, const float* cutoffs, void* codes,
                     int64_t T, int P, int K, int bits, hipStream_t stream) {
  ATPU_CHECK(P % 64 == 0 && P >= 64 && P <= 1024, "residual_encode: P must be a multiple of 64 in [64, 1024]");
  ATPU_CHECK(bits == 1 || bits == 2 || bits == 4, "residual_encode: bits must be 1, 2 or 4");
  ATPU_CHECK(K >= 1 && K <= 4096 && T >= 0, "residual_encode: K must be in [1, 4096] and T >= 0");
  if (T == 0) return;
  ATPU_CHECK(x && cid && centroids && cutoffs && codes, "residual_encode: null tensor");
  ATPU_CHECK(((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(centroids) | reinterpret_cast<uintptr_t>(codes)) & 15) == 0,
             "residual_encode: x, centroids and codes must be 16-byte aligned");
  const long long total = (long long)T * (P >> 2);
  const long long blocks = (total + 255) / 256;
  ATPU_CHECK(blocks <= 0x7fffffffLL, "residual_encode: too many rows for one launch");
  const dim3 grid((unsigned)blocks);
  unsigned* out = static_cast<unsigned*>(codes);
  if (bits == 1)
    hipLaunchKernelGGL((residual_encode_kernel<1>), grid, dim3(256), 0, stream, x, cid, centroids, cutoffs, out, total, P, K);
  else if (bits == 2)
    hipLaunchKernelGGL((residual_encode_kernel<2>), grid, dim3(256), 0, stream, x, cid, centroids, cutoffs, out, total, P, K);
  else
    hipLaunchKernelGGL((residual_encode_kernel<4>), grid, dim3(256), 0, stream, x, cid, centroids, cutoffs, out, total, P, K);
  ATPU_HIP_CHECK(hipGetLastError());
}

}  // namespace atpu
