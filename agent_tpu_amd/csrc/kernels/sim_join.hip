// Near-duplicate detection on the device: a similarity self-join with a threshold (the third epilogue of
// the exact fp32 similarity GEMM, after sim_topk's top-k and kmeans_assign's arg-max) and the connected
// components of the pairs it emits.
//
// sim_join_kernel<QH, NW>: persistent workgroups of NW waves walk work items (column panel, row tile).
// A row tile is QT = 16 QH rows of x [Nx, D] in LDS (row stride D + 4 floats), the B operand of
// v_mfma_f32_16x16x4_f32; a column panel is PS steps of 32 rows of y [Ny, D], streamed as the A operand
// with the two-buffer prefetch of kmeans_assign_kernel (wave w takes the panel's steps w, w + NW, ...).
// The column order of one dot product is sim_topk's (see the header of sim_topk.hip), a function of D
// alone, and every (row, column) score is one fp32 accumulator: a pair's score has the bits that
// sim_topk(x[i:i+1], y, ...) reports for row j, whatever the tile, wave, panel, grid, Nx or Ny.
//
// Ids: row i of x is I = x_base + i, row j of y is J = y_base + j. A pair is emitted when I < J and
// score >= threshold (an fp32 compare), so the lower id is always the x-side operand and a row never
// pairs with itself. The steps of a panel whose largest id is <= the tile's smallest id are not
// computed (the live steps of a tile are a suffix); the steps that the diagonal crosses are masked by
// I < J. Rows past Nx and columns past Ny are clamped into range and their scores discarded by select:
// nothing outside x[0:Nx] and y[0:Ny] is read.
//
// Walk: item = panel * ntiles + tile, workgroup b takes items b, b + grid, ..., so the workgroups that
// are resident together read the same column panel while every one of them holds a different row tile.
// PS = 256 steps (8192 rows: 24 MiB at D = 768) is past an XCD's 4 MiB L2 and inside the 256 MiB
// Infinity Cache; measured at N = 2^18, panels of 1024 rows (inside L2) reach 110 TF/s of triangle
// flops, 8192 to 65536 rows 119, one panel of all rows 114 (docs/PERF_NOTES.md): every item reloads its
// row tile and restarts the prefetch, which costs more than the L2 misses of a larger panel. The dead
// tiles of a panel (the whole panel at or below the tile's diagonal) are a suffix of its tiles and are
// jumped over.
//
// Emission: a lane owns 8 QH scores of a finished step. One wave-uniform ballot says whether any lane
// has a hit; without one nothing more happens (the common case). Otherwise the 8 QH slots are ranked
// by ballot + mbcnt, lane 0 reserves the wave's slots with ONE 64-bit atomicAdd on count, and the lanes
// whose slot is < cap store (I, J, score) with plain vector stores. count ends as the true total also
// beyond cap; nothing is written at or past cap. The order of the list is arbitrary.
//
// cc_min_labels: labels[v] = the smallest id in v's connected component. parent[v] <= v always holds.
// One round hooks every edge (atomicMin of the smaller parent into the parent slot of the larger one)
// and then compresses every node to its root; the host repeats rounds until a round's hooks change
// nothing. At that fixed point parent is constant on every edge, hence on every component, and a
// component's smallest member can only point at itself: the result is unique, so the races between
// hooks do not show in it. Parents only decrease, so the rounds end.
#include "atpu/common.h"
#include "atpu/kernels.h"

namespace atpu {
namespace {

constexpr int kSjStepRows = 32;  // rows of y per wave step: two 16-row MFMA tiles
constexpr int kSjStep = 64;      // columns per load step
constexpr int kSjPad = 4;        // floats of padding per LDS row
constexpr int kSjPanelSteps = 256;  // steps of a column panel (8192 rows)
constexpr int kCcThreads = 256;

struct SjFrag {
  f32x4 a[2][4];  // [y tile][chunk]
};

__device__ __forceinline__ void sj_load(SjFrag& f, const float* __restrict__ y, int D, int Ny, int row0, int r, int g,
                                        int kb) {
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int row = min(row0 + t * 16 + r, Ny - 1);  // clamp, the score is discarded by select
    const float* p = y + (size_t)row * D + kb + 4 * g;
#pragma unroll
    for (int ch = 0; ch < 4; ++ch) f.a[t][ch] = *reinterpret_cast<const f32x4*>(p + 16 * ch);
  }
}

__device__ __forceinline__ int sj_rank(unsigned long long m) {
  return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
}

template <int QH, int NW>
__global__ __launch_bounds__(NW * kWave) void sim_join_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                               float thr, int Nx, int Ny, int D, int x_base,
                                                               int y_base, int ntiles, int npanels, int PS,
                                                               int32_t* __restrict__ pairs, float* __restrict__ scores,
                                                               unsigned long long* __restrict__ count,
                                                               unsigned long long cap) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int QT = 16 * QH;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int ldq = D + kSjPad;
  const int c4 = D >> 2;
  const int nsteps = (Ny + kSjStepRows - 1) / kSjStepRows;
  const int KS = D / kSjStep;
  const float* qb = smem + r * ldq + 4 * g;
  const long long nitems = (long long)npanels * ntiles;
  bool loaded = false;

  for (long long item = blockIdx.x; item < nitems; item += gridDim.x) {
    const int panel = (int)(item / ntiles), tile = (int)(item - (long long)panel * ntiles);
    const int q0 = tile * QT;
    // live steps of the tile: y_base + 32 s + 31 > x_base + q0
    const long long d = (long long)x_base + q0 - y_base;
    const int s_min = d < 0 ? 0 : (int)min((d + 1) >> 5, (long long)nsteps);
    const int s_lo = max(panel * PS, s_min), s_hi = min((panel + 1) * PS, nsteps);
    if (s_lo >= s_hi) {  // so are the panel's later tiles: on to this workgroup's first item of the next panel
      const long long nxt = (long long)(panel + 1) * ntiles;
      item += (nxt - item + gridDim.x - 1) / gridDim.x * gridDim.x - gridDim.x;
      continue;
    }
    if (loaded) __syncthreads();  // every wave is done with the previous row tile
    for (int i = tid; i < QT * c4; i += NW * kWave) {
      const int qi = i / c4, cc = i - qi * c4;
      const int qr = min(q0 + qi, Nx - 1);  // slots past Nx repeat the last row
      *reinterpret_cast<f32x4*>(smem + qi * ldq + cc * 4) = *reinterpret_cast<const f32x4*>(x + (size_t)qr * D + cc * 4);
    }
    __syncthreads();
    loaded = true;

    SjFrag f0, f1;
    int s = s_lo + wave, ks = 0;
    f32x4 acc[2][QH];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int h = 0; h < QH; ++h) acc[t][h] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (s < s_hi) sj_load(f0, y, D, Ny, s * kSjStepRows, r, g, 0);
    auto stage = [&](const SjFrag& cur, SjFrag& nxt) {
      const bool last = ks + 1 == KS;
      const int ns = last ? s + NW : s, nks = last ? 0 : ks + 1;
      sj_load(nxt, y, D, Ny, ns * kSjStepRows, r, g, nks * kSjStep);  // clamped into y[0:Ny] past the end
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int ch = 0; ch < 4; ++ch) {
        f32x4 b[QH];
#pragma unroll
        for (int h = 0; h < QH; ++h)
          b[h] = *reinterpret_cast<const f32x4*>(qb + h * 16 * ldq + ks * kSjStep + 16 * ch);
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int h = 0; h < QH; ++h)
              acc[t][h] = __builtin_amdgcn_mfma_f32_16x16x4f32(cur.a[t][ch][j], b[h][j], acc[t][h], 0, 0, 0);
      }
      if (last) {  // the step's scores are complete: the threshold filter
        unsigned bits = 0;  // slot (t, e, h) -> bit (t * 4 + e) * QH + h
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int col = s * kSjStepRows + t * 16 + g * 4 + e;
            const long long J = (long long)y_base + col;
#pragma unroll
            for (int h = 0; h < QH; ++h) {
              const int row = q0 + h * 16 + r;
              const bool live = col < Ny && row < Nx && (long long)x_base + row < J;
              const bool hit = live && acc[t][h][e] >= thr;
              bits |= (hit ? 1u : 0u) << ((t * 4 + e) * QH + h);
            }
          }
        if (__ballot(bits != 0) != 0) {
          int total = 0;
#pragma unroll
          for (int k = 0; k < 8 * QH; ++k) total += __popcll(__ballot((bits >> k) & 1u));
          unsigned long long base = 0;
          if (lane == 0) base = atomicAdd(count, (unsigned long long)total);
          base = __shfl(base, 0, 64);
          int run = 0;
#pragma unroll
          for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
              for (int h = 0; h < QH; ++h) {
                const int k = (t * 4 + e) * QH + h;
                const bool hit = (bits >> k) & 1u;
                const unsigned long long m = __ballot(hit);
                const unsigned long long slot = base + (unsigned long long)(run + sj_rank(m));
                if (hit && slot < cap) {
                  pairs[2 * slot] = x_base + q0 + h * 16 + r;
                  pairs[2 * slot + 1] = y_base + s * kSjStepRows + t * 16 + g * 4 + e;
                  scores[slot] = acc[t][h][e];
                }
                run += __popcll(m);
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
    while (s < s_hi) {
      stage(f0, f1);
      if (s < s_hi) stage(f1, f0);
    }
  }
}

int sj_cus() {
  int dev = 0, cus = 0;
  ATPU_HIP_CHECK(hipGetDevice(&dev));
  ATPU_HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
  return cus > 0 ? cus : 1;
}

// ------------------------------------------------------------------------------------ connected components
__global__ __launch_bounds__(kCcThreads) void cc_init_kernel(int32_t* __restrict__ parent, int N) {
  for (long long v = (long long)blockIdx.x * kCcThreads + threadIdx.x; v < N; v += (long long)gridDim.x * kCcThreads)
    parent[v] = (int32_t)v;
}

// every parent value is a root here (the previous round compressed); hooks touch root slots only
__global__ __launch_bounds__(kCcThreads) void cc_hook_kernel(const int32_t* __restrict__ pairs, long long E, int N,
                                                             int32_t* __restrict__ parent, int32_t* __restrict__ changed) {
  for (long long i = (long long)blockIdx.x * kCcThreads + threadIdx.x; i < E; i += (long long)gridDim.x * kCcThreads) {
    const int u = pairs[2 * i], v = pairs[2 * i + 1];
    if ((unsigned)u >= (unsigned)N || (unsigned)v >= (unsigned)N) continue;  // the wrapper refuses such a list
    const int pu = parent[u], pv = parent[v];
    if (pu == pv) continue;
    const int hi = max(pu, pv), lo = min(pu, pv);
    if (atomicMin(parent + hi, lo) > lo) *changed = 1;
  }
}

__global__ __launch_bounds__(kCcThreads) void cc_compress_kernel(int32_t* __restrict__ parent, int N) {
  for (long long v = (long long)blockIdx.x * kCcThreads + threadIdx.x; v < N; v += (long long)gridDim.x * kCcThreads) {
    const int p0 = parent[v];
    int p = p0;
    for (;;) {  // parent[p] < p unless p is a root: at most N steps
      const int pp = parent[p];
      if (pp == p) break;
      p = pp;
    }
    if (p != p0) parent[v] = p;
  }
}

int cc_grid(long long n, int cus) {
  const long long want = (n + kCcThreads - 1) / kCcThreads;
  const long long cap = (long long)cus * 8;
  return (int)(want < 1 ? 1 : (want < cap ? want : cap));
}

}  // namespace

bool sim_join_ok(int D) { return D % 64 == 0 && D >= 64 && D <= 1024; }

void sim_join(const float* x, const float* y, float threshold, int Nx, int Ny, int D, int x_base, int y_base,
              int32_t* pairs, float* scores, int64_t* count, int64_t cap, int max_wgs, int panel_steps,
              hipStream_t stream) {
  constexpr int kMaxId = 2147483647 - 256;
  ATPU_CHECK(sim_join_ok(D), "sim_join: D must be a multiple of 64 in [64, 1024]");
  ATPU_CHECK(Nx >= 1 && Ny >= 1 && x_base >= 0 && y_base >= 0 && Nx <= kMaxId - x_base && Ny <= kMaxId - y_base,
             "sim_join: Nx, Ny >= 1 and every id x_base + i, y_base + j in [0, 2^31 - 256)");
  ATPU_CHECK(cap >= 0 && count && x && y && (cap == 0 || (pairs && scores)), "sim_join: null tensor");
  ATPU_CHECK(((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & 15) == 0 &&
                 (reinterpret_cast<uintptr_t>(count) & 7) == 0,
             "sim_join: x and y must be 16-byte and the count 8-byte aligned");
  ATPU_CHECK(max_wgs >= 0 && panel_steps >= 0, "sim_join: max_wgs and panel_steps must be >= 0 (0: the default)");
  ATPU_HIP_CHECK(hipMemsetAsync(count, 0, sizeof(int64_t), stream));
  constexpr int QH = 2, NW = 8, QT = 16 * QH;
  const int PS = panel_steps ? panel_steps : kSjPanelSteps;
  const int nsteps = (Ny + kSjStepRows - 1) / kSjStepRows;
  const int ntiles = (Nx + QT - 1) / QT, npanels = (nsteps + PS - 1) / PS;
  const long long nitems = (long long)ntiles * npanels;
  const long long want = max_wgs ? max_wgs : sj_cus();
  const int grid = (int)(nitems < want ? nitems : want);
  const size_t lds = (size_t)QT * (D + kSjPad) * sizeof(float);  // 128.5 KiB at D = 1024
  ATPU_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&sim_join_kernel<QH, NW>),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL((sim_join_kernel<QH, NW>), dim3(grid), dim3(NW * kWave), lds, stream, x, y, threshold, Nx, Ny, D,
                     x_base, y_base, ntiles, npanels, PS, pairs, scores, reinterpret_cast<unsigned long long*>(count),
                     (unsigned long long)cap);
  ATPU_HIP_CHECK(hipGetLastError());
}

void cc_init(int32_t* parent, int N, hipStream_t stream) {
  ATPU_CHECK(N >= 1 && parent, "cc_min_labels: N must be >= 1");
  hipLaunchKernelGGL(cc_init_kernel, dim3(cc_grid(N, sj_cus())), dim3(kCcThreads), 0, stream, parent, N);
  ATPU_HIP_CHECK(hipGetLastError());
}

void cc_round(const int32_t* pairs, int64_t E, int32_t* parent, int N, int32_t* changed, hipStream_t stream) {
  ATPU_CHECK(N >= 1 && E >= 1 && pairs && parent && changed, "cc_min_labels: null tensor");
  const int cus = sj_cus();
  ATPU_HIP_CHECK(hipMemsetAsync(changed, 0, sizeof(int32_t), stream));
  hipLaunchKernelGGL(cc_hook_kernel, dim3(cc_grid(E, cus)), dim3(kCcThreads), 0, stream, pairs, (long long)E, N, parent,
                     changed);
  hipLaunchKernelGGL(cc_compress_kernel, dim3(cc_grid(N, cus)), dim3(kCcThreads), 0, stream, parent, N);
  ATPU_HIP_CHECK(hipGetLastError());
}

}  // namespace atpu
