// Lloyd's k-means on the device: the assignment step (a similarity GEMM with an arg-max epilogue), the
// centroid update (an order-free segmented sum keyed by label) and the centroid finalize.
//
// kmeans_assign_kernel<QH, NW>: persistent workgroups of NW waves walk tiles of QT = 16 QH rows of
// x [N, D]. The row tile sits in LDS (row stride D + 4 floats, as the query tile of sim_topk.hip) and is
// the B operand of v_mfma_f32_16x16x4_f32; the waves stream the centroids c [K, D], which stay in L2,
// as the A operand in steps of 32 centroids (wave w takes steps w, w + NW, ...). The column order of
// one dot product is sim_topk's (chunks of 16 columns, j-major inside a chunk, four chunks per load
// step: see the header of sim_topk.hip), a function of D alone, and every (row, centroid) score is one
// fp32 accumulator, so a row's score has the same bits as sim_topk's whatever N, K, the tile, the wave
// or the launch shape. The optional bias is one fp32 add on the finished accumulator.
//
// Each lane keeps ONE best (score, centroid) per row slot in the total order of better() (score desc,
// centroid asc, +0.0 == -0.0). At the end of a tile the 4 lane groups meet by two permlane swaps and
// the NW waves through a small LDS array; QT threads write label and best and count the rows whose
// label differs from prev_labels (one integer atomic per workgroup at the end: order-free).
//
// Rows past N and centroids past K are clamped into range and their scores discarded by select, never
// multiplied by 0: nothing outside x[0:N], c[0:K], bias[0:K], prev_labels[0:N] is read.
//
// Order-free sums: a value v enters a sum as the int64 rint(v * 2^s) (ties to even). v is fp32 and the
// scale a power of two, so the product is exact in fp64 and the only rounding is the rint. Integer
// addition is associative: the totals have the same bits in any order, chunking or rank split, which
// is why integer atomics are deterministic here (and only here).
//
// kmeans_update: (1) label histogram (integer atomics), (2) one-workgroup exclusive scan, (3) row ids
// scattered into label order through per-label cursors (the order inside a label is arbitrary and
// does not matter), (4) workgroup (label, slice) sums chunks of the label's rows in int64 registers, a
// float4 column per thread, and adds them to sums [K, D] with one 64-bit integer atomic per column.
// One pass over x.
//
// kmeans_finalize: one thread per centroid, fp64 with explicit single-rounding operations in ascending
// column order (no contraction), so the PyTorch twin reproduces the bits.
#include "atpu/common.h"
#include "atpu/kernels.h"
#include "atpu/topk.h"

namespace atpu {
namespace {

constexpr int kKmStepRows = 32;  // centroids per wave step: two 16-row MFMA tiles
constexpr int kKmStep = 64;      // columns per load step
constexpr int kKmPad = 4;        // floats of padding per LDS row
constexpr int kKmNone = 0x7fffffff;
constexpr int kKmThreads = 256;  // update / scan / fixed_sum workgroups
constexpr int kKmChunk = 64;     // rows of one label that a workgroup sums before it flushes

struct KmFrag {
  f32x4 a[2][4];  // [centroid tile][chunk]
};

__device__ __forceinline__ void km_load(KmFrag& f, const float* __restrict__ c, int D, int K, int row0, int r, int g,
                                        int kb) {
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int row = min(row0 + t * 16 + r, K - 1);  // clamp, the score is discarded by select
    const float* p = c + (size_t)row * D + kb + 4 * g;
#pragma unroll
    for (int ch = 0; ch < 4; ++ch) f.a[t][ch] = *reinterpret_cast<const f32x4*>(p + 16 * ch);
  }
}

template <int QH, int NW>
__global__ __launch_bounds__(NW * kWave) void kmeans_assign_kernel(const float* __restrict__ x,
                                                                    const float* __restrict__ c,
                                                                    const float* __restrict__ bias,
                                                                    const int32_t* __restrict__ prev,
                                                                    int32_t* __restrict__ labels,
                                                                    float* __restrict__ best,
                                                                    unsigned long long* __restrict__ changed, int N,
                                                                    int K, int D, int ntiles) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int QT = 16 * QH;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int ldq = D + kKmPad;
  float2* red = reinterpret_cast<float2*>(smem + QT * ldq);  // [NW][QT]
  const int c4 = D >> 2;
  const int nsteps = (K + kKmStepRows - 1) / kKmStepRows;
  const int KS = D / kKmStep;
  const float* qb = smem + r * ldq + 4 * g;
  int nchanged = 0;  // thread 0's running count

  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int q0 = tile * QT;
    // row tile -> LDS (slots past N repeat the last row); the previous tile's MFMAs are behind the
    // barrier that precedes its epilogue
    for (int i = tid; i < QT * c4; i += NW * kWave) {
      const int qi = i / c4, cc = i - qi * c4;
      const int qr = min(q0 + qi, N - 1);
      *reinterpret_cast<f32x4*>(smem + qi * ldq + cc * 4) = *reinterpret_cast<const f32x4*>(x + (size_t)qr * D + cc * 4);
    }
    __syncthreads();

    float bv[QH];
    int bi[QH];
#pragma unroll
    for (int h = 0; h < QH; ++h) {
      bv[h] = -__builtin_inff();
      bi[h] = kKmNone;
    }
    KmFrag f0, f1;
    int s = wave, ks = 0;
    f32x4 acc[2][QH];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int h = 0; h < QH; ++h) acc[t][h] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (s < nsteps) km_load(f0, c, D, K, s * kKmStepRows, r, g, 0);
    auto stage = [&](const KmFrag& cur, KmFrag& nxt) {
      const bool last = ks + 1 == KS;
      const int ns = last ? s + NW : s, nks = last ? 0 : ks + 1;
      km_load(nxt, c, D, K, ns * kKmStepRows, r, g, nks * kKmStep);  // clamped into c[0:K] past the end
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int ch = 0; ch < 4; ++ch) {
        f32x4 b[QH];
#pragma unroll
        for (int h = 0; h < QH; ++h)
          b[h] = *reinterpret_cast<const f32x4*>(qb + h * 16 * ldq + ks * kKmStep + 16 * ch);
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int h = 0; h < QH; ++h)
              acc[t][h] = __builtin_amdgcn_mfma_f32_16x16x4f32(cur.a[t][ch][j], b[h][j], acc[t][h], 0, 0, 0);
      }
      if (last) {  // the centroids' scores are complete
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int row = s * kKmStepRows + t * 16 + g * 4 + e;
            const bool live = row < K;
            const float bb = bias != nullptr ? bias[min(row, K - 1)] : 0.f;
#pragma unroll
            for (int h = 0; h < QH; ++h) {
              const float sc = bias != nullptr ? acc[t][h][e] + bb : acc[t][h][e];
              const float v = live ? sc : -__builtin_inff();
              const int id = live ? row : kKmNone;
              const bool sw = better(v, id, bv[h], bi[h]);
              bv[h] = sw ? v : bv[h];
              bi[h] = sw ? id : bi[h];
            }
          }
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int h = 0; h < QH; ++h) acc[t][h] = f32x4{0.f, 0.f, 0.f, 0.f};
      }
      s = ns;
      ks = nks;
    };
    while (s < nsteps) {
      stage(f0, f1);
      if (s < nsteps) stage(f1, f0);
    }

    // the 4 lane groups of a row slot (lanes r, r + 16, r + 32, r + 48), then the NW waves through LDS
#pragma unroll
    for (int h = 0; h < QH; ++h) {
      auto step = [&](float ov, int oi) {
        const bool sw = better(ov, oi, bv[h], bi[h]);
        bv[h] = sw ? ov : bv[h];
        bi[h] = sw ? oi : bi[h];
      };
      step(xor16f(bv[h]), xor16i(bi[h]));
      step(xor32f(bv[h]), xor32i(bi[h]));
      if (g == 0) red[wave * QT + h * 16 + r] = float2{bv[h], __int_as_float(bi[h])};
    }
    __syncthreads();  // also: every wave is done with the row tile
    if (wave == 0) {
      const int qi = min(lane, QT - 1);
      float v = red[qi].x;
      int id = __float_as_int(red[qi].y);
#pragma unroll
      for (int w = 1; w < NW; ++w) {
        const float2 o = red[w * QT + qi];
        const bool sw = better(o.x, __float_as_int(o.y), v, id);
        v = sw ? o.x : v;
        id = sw ? __float_as_int(o.y) : id;
      }
      const bool mine = lane < QT && q0 + lane < N;
      bool diff = false;
      if (mine) {
        labels[q0 + lane] = id;
        best[q0 + lane] = v;
        diff = prev[q0 + lane] != id;
      }
      nchanged += __popcll(__ballot(diff));
    }
    // wave 0 reads `red` before it reaches the next tile's barrier; the others write it after that barrier
  }
  if (tid == 0 && nchanged != 0) atomicAdd(changed, (unsigned long long)nchanged);
}

template <int QH, int NW>
void km_assign_launch(const float* x, const float* c, const float* bias, const int32_t* prev, int32_t* labels,
                      float* best, unsigned long long* changed, int N, int K, int D, int max_wgs,
                      hipStream_t stream) {
  constexpr int QT = 16 * QH;
  const size_t lds = (size_t)QT * (D + kKmPad) * sizeof(float) + (size_t)NW * QT * sizeof(float2);
  ATPU_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&kmeans_assign_kernel<QH, NW>),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  const int ntiles = (int)(((long long)N + QT - 1) / QT);
  const int grid = ntiles < max_wgs ? ntiles : max_wgs;
  hipLaunchKernelGGL((kmeans_assign_kernel<QH, NW>), dim3(grid), dim3(NW * kWave), lds, stream, x, c, bias, prev,
                     labels, best, changed, N, K, D, ntiles);
  ATPU_HIP_CHECK(hipGetLastError());
}

// ------------------------------------------------------------------------------------------ fixed-point sums
__device__ __forceinline__ long long km_fixed(float v, double scale) { return __double2ll_rn((double)v * scale); }

__device__ __forceinline__ long long wave_sum_i64(long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ __launch_bounds__(kKmThreads) void fixed_sum_kernel(const float* __restrict__ v, long long n, double scale,
                                                               unsigned long long* __restrict__ out) {
  long long acc = 0;
  for (long long i = (long long)blockIdx.x * kKmThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kKmThreads)
    acc += km_fixed(v[i], scale);
  acc = wave_sum_i64(acc);
  if ((threadIdx.x & 63) == 0 && acc != 0) atomicAdd(out, (unsigned long long)acc);
}

__global__ __launch_bounds__(kKmThreads) void km_hist_kernel(const int32_t* __restrict__ labels, int N, int K,
                                                             unsigned long long* __restrict__ counts) {
  for (long long i = (long long)blockIdx.x * kKmThreads + threadIdx.x; i < N; i += (long long)gridDim.x * kKmThreads) {
    const int l = labels[i];
    if (l >= 0 && l < K) atomicAdd(counts + l, 1ull);  // a label outside [0, K) leaves its row out
  }
}

// one workgroup: offsets[k] = sum of counts[0:k]; cursors start at the offsets
__global__ __launch_bounds__(kKmThreads) void km_scan_kernel(const unsigned long long* __restrict__ counts, int K,
                                                             int* __restrict__ offsets, int* __restrict__ cursors) {
  __shared__ int part[kKmThreads];
  const int tid = threadIdx.x;
  const int per = (K + kKmThreads - 1) / kKmThreads;
  const int lo = min(tid * per, K), hi = min(lo + per, K);
  int sum = 0;
  for (int k = lo; k < hi; ++k) sum += (int)counts[k];
  part[tid] = sum;
  __syncthreads();
  if (tid == 0) {
    int run = 0;
    for (int t = 0; t < kKmThreads; ++t) {
      const int v = part[t];
      part[t] = run;
      run += v;
    }
  }
  __syncthreads();
  int run = part[tid];
  for (int k = lo; k < hi; ++k) {
    offsets[k] = run;
    cursors[k] = run;
    run += (int)counts[k];
  }
}

__global__ __launch_bounds__(kKmThreads) void km_scatter_kernel(const int32_t* __restrict__ labels, int N, int K,
                                                                int* __restrict__ cursors, int* __restrict__ perm) {
  for (long long i = (long long)blockIdx.x * kKmThreads + threadIdx.x; i < N; i += (long long)gridDim.x * kKmThreads) {
    const int l = labels[i];
    if (l >= 0 && l < K) perm[atomicAdd(cursors + l, 1)] = (int)i;  // slot < offsets[l] + counts[l] <= N
  }
}

// workgroup (label k, slice sl of S): the label's rows perm[offsets[k] + m], m in chunks sl, sl + S, ...
// of kKmChunk rows. Thread (rg, cq): float4 column cq of the rows rg, rg + RP, ... of a chunk.
__global__ __launch_bounds__(kKmThreads) void km_reduce_kernel(const float* __restrict__ x,
                                                               const int* __restrict__ perm,
                                                               const int* __restrict__ offsets,
                                                               const unsigned long long* __restrict__ counts, int D,
                                                               int S, double scale,
                                                               unsigned long long* __restrict__ sums) {
  const int k = blockIdx.x / S, sl = blockIdx.x - k * S;
  const int cnt = (int)counts[k];
  if (sl * kKmChunk >= cnt) return;
  const int c4 = D >> 2;            // <= 256
  const int RP = kKmThreads / c4;  // rows in parallel (1 for D > 512)
  const int tid = threadIdx.x;
  const int rg = tid / c4, cq = tid - rg * c4;
  if (rg >= RP) return;
  const int* members = perm + offsets[k];
  long long a0 = 0, a1 = 0, a2 = 0, a3 = 0;
  for (int base = sl * kKmChunk; base < cnt; base += S * kKmChunk) {
    const int end = min(base + kKmChunk, cnt);
    int m = base + rg;
    for (; m + 3 * RP < end; m += 4 * RP) {  // four rows in flight
      f32x4 v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = *reinterpret_cast<const f32x4*>(x + (size_t)members[m + u * RP] * D + cq * 4);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        a0 += km_fixed(v[u][0], scale);
        a1 += km_fixed(v[u][1], scale);
        a2 += km_fixed(v[u][2], scale);
        a3 += km_fixed(v[u][3], scale);
      }
    }
    for (; m < end; m += RP) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(x + (size_t)members[m] * D + cq * 4);
      a0 += km_fixed(v[0], scale);
      a1 += km_fixed(v[1], scale);
      a2 += km_fixed(v[2], scale);
      a3 += km_fixed(v[3], scale);
    }
  }
  unsigned long long* dst = sums + (size_t)k * D + cq * 4;
  if (a0 != 0) atomicAdd(dst + 0, (unsigned long long)a0);
  if (a1 != 0) atomicAdd(dst + 1, (unsigned long long)a1);
  if (a2 != 0) atomicAdd(dst + 2, (unsigned long long)a2);
  if (a3 != 0) atomicAdd(dst + 3, (unsigned long long)a3);
}

// ------------------------------------------------------------------------------------------------ finalize
__global__ __launch_bounds__(kKmThreads) void km_finalize_kernel(const long long* __restrict__ sums,
                                                                 const long long* __restrict__ counts,
                                                                 const float* __restrict__ c_old,
                                                                 float* __restrict__ c_new, float* __restrict__ bias,
                                                                 int K, int D, double scale, int cosine) {
#pragma clang fp contract(off)  // every fp64 operation below rounds once, as the PyTorch twin's
  const int k = blockIdx.x * kKmThreads + threadIdx.x;
  if (k >= K) return;
  const long long cnt = counts[k];
  const float* old = c_old + (size_t)k * D;
  float* out = c_new + (size_t)k * D;
  if (cnt > 0) {
    const double den = (double)cnt * scale;  // exact: a power-of-two scale
    double ss = 0.0;
    for (int d = 0; d < D; ++d) {
      const float m = (float)((double)sums[(size_t)k * D + d] / den);
      out[d] = m;
      const double sq = (double)m * (double)m;
      ss = ss + sq;
    }
    if (cosine) {
      const double nrm = fmax(__dsqrt_rn(ss), 1e-12);
      for (int d = 0; d < D; ++d) out[d] = (float)((double)out[d] / nrm);
    }
  } else {  // an empty cluster keeps its centroid
    for (int d = 0; d < D; ++d) out[d] = old[d];
  }
  if (bias != nullptr) {
    double ss = 0.0;
    for (int d = 0; d < D; ++d) {
      const double sq = (double)out[d] * (double)out[d];
      ss = ss + sq;
    }
    bias[k] = (float)(-0.5 * ss);
  }
}

int km_cus() {
  int dev = 0, cus = 0;
  ATPU_HIP_CHECK(hipGetDevice(&dev));
  ATPU_HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
  return cus > 0 ? cus : 1;
}

int km_grid(long long n, int cus) {
  const long long want = (n + kKmThreads - 1) / kKmThreads;
  const long long cap = (long long)cus * 8;
  return (int)(want < 1 ? 1 : (want < cap ? want : cap));
}

}  // namespace

bool kmeans_shape_ok(int D, int K) { return D % 64 == 0 && D >= 64 && D <= 1024 && K >= 1 && K <= kKmeansMaxK; }

void kmeans_assign(const float* x, const float* c, const float* bias, const int32_t* prev_labels, int32_t* labels,
                   float* best, int64_t* changed, int N, int K, int D, int max_wgs, hipStream_t stream) {
  ATPU_CHECK(kmeans_shape_ok(D, K), "kmeans_assign: D must be a multiple of 64 in [64, 1024] and K in [1, 4096]");
  ATPU_CHECK(N >= 1 && N <= 2147483647 - 256, "kmeans_assign: N must be in [1, 2^31 - 256]");
  ATPU_CHECK(x && c && prev_labels && labels && best && changed, "kmeans_assign: null tensor");
  ATPU_CHECK(((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(c)) & 15) == 0 &&
                 (reinterpret_cast<uintptr_t>(changed) & 7) == 0,
             "kmeans_assign: x and c must be 16-byte and the changed count 8-byte aligned");
  ATPU_CHECK(max_wgs >= 0, "kmeans_assign: max_wgs must be >= 0 (0: one round of the device)");
  ATPU_HIP_CHECK(hipMemsetAsync(changed, 0, sizeof(int64_t), stream));
  unsigned long long* ch = reinterpret_cast<unsigned long long*>(changed);
  // few centroids: 16-row tiles (49 KiB at D = 768), three workgroups of four waves per CU overlap their
  // tile loads with each other's MFMAs; otherwise 32-row tiles, one workgroup of eight waves per CU, so
  // every centroid fragment read from L2 serves 32 rows
  if (K <= 64) {
    km_assign_launch<1, 4>(x, c, bias, prev_labels, labels, best, ch, N, K, D, max_wgs ? max_wgs : 3 * km_cus(), stream);
  } else {
    km_assign_launch<2, 8>(x, c, bias, prev_labels, labels, best, ch, N, K, D, max_wgs ? max_wgs : km_cus(), stream);
  }
}

void fixed_sum(const float* v, int64_t n, int shift, int64_t* out, hipStream_t stream) {
  ATPU_CHECK(n >= 0 && out && (v || n == 0), "fixed_sum: null tensor");
  ATPU_CHECK(shift >= -1000 && shift <= 1000, "fixed_sum: shift must be in [-1000, 1000]");
  ATPU_HIP_CHECK(hipMemsetAsync(out, 0, sizeof(int64_t), stream));
  if (n == 0) return;
  hipLaunchKernelGGL(fixed_sum_kernel, dim3(km_grid(n, km_cus())), dim3(kKmThreads), 0, stream, v, (long long)n,
                     ldexp(1.0, shift), reinterpret_cast<unsigned long long*>(out));
  ATPU_HIP_CHECK(hipGetLastError());
}

size_t kmeans_update_ws_bytes(int N, int K) { return ((size_t)N + 2 * (size_t)K) * sizeof(int32_t); }

void kmeans_update(const float* x, const int32_t* labels, int shift, int64_t* sums, int64_t* counts, int32_t* ws,
                   int N, int K, int D, hipStream_t stream) {
  ATPU_CHECK(kmeans_shape_ok(D, K), "kmeans_update: D must be a multiple of 64 in [64, 1024] and K in [1, 4096]");
  ATPU_CHECK(N >= 1 && N <= 2147483647 - 256, "kmeans_update: N must be in [1, 2^31 - 256]");
  ATPU_CHECK(shift >= -1000 && shift <= 1000, "kmeans_update: shift must be in [-1000, 1000]");
  ATPU_CHECK(x && labels && sums && counts && ws, "kmeans_update: null tensor");
  ATPU_CHECK((reinterpret_cast<uintptr_t>(x) & 15) == 0 && ((reinterpret_cast<uintptr_t>(sums) |
                                                             reinterpret_cast<uintptr_t>(counts)) & 7) == 0,
             "kmeans_update: x must be 16-byte, sums and counts 8-byte aligned");
  // ws: perm [N], offsets [K], cursors [K]
  int* perm = ws;
  int* offsets = ws + N;
  int* cursors = offsets + K;
  ATPU_HIP_CHECK(hipMemsetAsync(sums, 0, (size_t)K * D * sizeof(int64_t), stream));
  ATPU_HIP_CHECK(hipMemsetAsync(counts, 0, (size_t)K * sizeof(int64_t), stream));
  const int cus = km_cus();
  unsigned long long* ucounts = reinterpret_cast<unsigned long long*>(counts);
  hipLaunchKernelGGL(km_hist_kernel, dim3(km_grid(N, cus)), dim3(kKmThreads), 0, stream, labels, N, K, ucounts);
  hipLaunchKernelGGL(km_scan_kernel, dim3(1), dim3(kKmThreads), 0, stream, ucounts, K, offsets, cursors);
  hipLaunchKernelGGL(km_scatter_kernel, dim3(km_grid(N, cus)), dim3(kKmThreads), 0, stream, labels, N, K, cursors, perm);
  // slices per label: about two chunks' worth of workgroups per chunk of rows, so one label holding every
  // row still spreads over the device
  long long S = (2ll * N + (long long)K * kKmChunk - 1) / ((long long)K * kKmChunk);
  S = S < 1 ? 1 : (S > 4096 ? 4096 : S);
  hipLaunchKernelGGL(km_reduce_kernel, dim3((unsigned)(K * S)), dim3(kKmThreads), 0, stream, x, perm, offsets, ucounts,
                     D, (int)S, ldexp(1.0, shift), reinterpret_cast<unsigned long long*>(sums));
  ATPU_HIP_CHECK(hipGetLastError());
}

void kmeans_finalize(const int64_t* sums, const int64_t* counts, const float* c_old, float* c_new, float* bias, int K,
                     int D, int shift, int cosine, hipStream_t stream) {
  ATPU_CHECK(K >= 1 && K <= kKmeansMaxK && D >= 1, "kmeans_finalize: K must be in [1, 4096]");
  ATPU_CHECK(shift >= -1000 && shift <= 1000, "kmeans_finalize: shift must be in [-1000, 1000]");
  ATPU_CHECK(sums && counts && c_old && c_new, "kmeans_finalize: null tensor");
  hipLaunchKernelGGL(km_finalize_kernel, dim3((K + kKmThreads - 1) / kKmThreads), dim3(kKmThreads), 0, stream,
                     reinterpret_cast<const long long*>(sums), reinterpret_cast<const long long*>(counts), c_old, c_new,
                     bias, K, D, ldexp(1.0, shift), cosine);
  ATPU_HIP_CHECK(hipGetLastError());
}

}  // namespace atpu
