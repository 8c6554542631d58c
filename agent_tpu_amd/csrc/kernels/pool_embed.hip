// Sentence embedding from the encoder's last hidden rows: masked mean (or the [CLS] row), the
// last LayerNorm applied to the POOLED vector instead of to every row, optional L2 normalisation.
//
// On the LayerNorm-folded encoder the last layer leaves raw rows g_j (pre-LN sums) and their
// statistics fin = (rstd_j, rstd_j * mu_j). The mean commutes with that LayerNorm:
//   mean_{j<len} LN(g_j)[n] = gamma[n] * (sum_j rstd_j g_j[n] - sum_j rstd_j mu_j) / len + beta[n]
// so the kernel reads every real token row once, never a padding row, and no [B*S, H] tensor
// is written. Without fin the rows are already normalised: out = sum_j x_j / len. Mode cls is
// the same algebra over row 0 alone (len = 1).
//
// One workgroup (512 threads) per sequence. The real rows of a sequence are contiguous, so it
// is streamed as a flat run of 16-B chunks: with C = H / 8 chunks per row, R = 512 / C whole
// rows are in flight per pass and thread t = r * C + c always holds column chunk c (768
// columns: C = 96, R = 5, 480 threads busy; a wave's 64 loads are 1 KiB contiguous whatever C
// is). Four passes are loaded before the first is consumed (4 x 16 B in flight per lane).
// fp32 accumulators, rows in increasing j per thread; the R partial rows meet in LDS and are
// summed in fixed order, the norm by a wave reduction and a fixed-order sum over the 8 waves:
// no atomics, a sequence's bits do not depend on the batch or on the run.
//
// Rows >= len: the row index is clamped to len - 1 (a row the encoder computed) and the loaded
// value is discarded by select, never multiplied by 0: whatever padding rows hold, NaN included,
// contributes nothing. len is clamped to [1, S].
#include "atpu/common.h"
#include "atpu/kernels.h"

namespace atpu {
namespace {

constexpr int kPoolThreads = 512;
constexpr int kPoolUnroll = 4;

template <bool FIN>
__global__ __launch_bounds__(kPoolThreads) void pool_embed_kernel(const bf16* __restrict__ x,
                                                                  const float* __restrict__ fin,
                                                                  const float* __restrict__ gamma,
                                                                  const float* __restrict__ beta,
                                                                  const int32_t* __restrict__ lens,
                                                                  float* __restrict__ out, int S, int H, int R,
                                                                  int cls, int normalize) {
  __shared__ __attribute__((aligned(16))) float part[kPoolThreads * 8];  // [R][H] partial sums
  __shared__ float s2part[64];                                            // [R] partial sum of rstd * mu
  __shared__ float red[kPoolThreads / kWave];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int C = H >> 3;
  const int len = cls ? 1 : min(max(lens[b], 1), S);
  const int r = tid / C, c = tid - r * C;
  float acc[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) acc[e] = 0.f;
  float s2 = 0.f;
  if (r < R) {
    const bf16* xb = x + (size_t)b * S * H + c * 8;
    const float* fb = FIN ? fin + (size_t)b * S * 2 : nullptr;
    for (int j0 = r; j0 < len; j0 += kPoolUnroll * R) {
      u32x4 v[kPoolUnroll];
      float2 f[kPoolUnroll];
#pragma unroll
      for (int u = 0; u < kPoolUnroll; ++u) {
        const int jc = min(j0 + u * R, len - 1);  // clamp, then select below
        v[u] = *reinterpret_cast<const u32x4*>(xb + (size_t)jc * H);
        if (FIN) f[u] = *reinterpret_cast<const float2*>(fb + jc * 2);
      }
#pragma unroll
      for (int u = 0; u < kPoolUnroll; ++u) {
        const bool live = j0 + u * R < len;
        const float w = FIN ? f[u].x : 1.f;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float lo = __uint_as_float(v[u][e] << 16), hi = __uint_as_float(v[u][e] & 0xffff0000u);
          const float a0 = FIN ? fmaf(w, lo, acc[2 * e]) : acc[2 * e] + lo;
          const float a1 = FIN ? fmaf(w, hi, acc[2 * e + 1]) : acc[2 * e + 1] + hi;
          acc[2 * e] = live ? a0 : acc[2 * e];
          acc[2 * e + 1] = live ? a1 : acc[2 * e + 1];
        }
        if (FIN) s2 = live ? s2 + f[u].y : s2;
      }
    }
    float* pr = part + r * H + c * 8;
    *reinterpret_cast<f32x4*>(pr) = f32x4{acc[0], acc[1], acc[2], acc[3]};
    *reinterpret_cast<f32x4*>(pr + 4) = f32x4{acc[4], acc[5], acc[6], acc[7]};
    if (c == 0) s2part[r] = s2;
  }
  __syncthreads();
  // column n = tid, tid + 512: the R partial rows in fixed order, then the pooled LayerNorm
  float ev[2] = {0.f, 0.f};
  float ss = 0.f;
  const float cnt = (float)len;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int n = tid + i * kPoolThreads;
    if (n < H) {
      float a = 0.f, m = 0.f;
      for (int q = 0; q < R; ++q) a += part[q * H + n];
      if (FIN) {
        for (int q = 0; q < R; ++q) m += s2part[q];
        ev[i] = gamma[n] * (a - m) / cnt + beta[n];
      } else {
        ev[i] = a / cnt;
      }
      ss = fmaf(ev[i], ev[i], ss);
    }
  }
  float den = 1.f;
  if (normalize) {  // wave-uniform: every lane of every wave takes part in the reductions
    ss = wave_sum(ss);
    if ((tid & (kWave - 1)) == 0) red[tid / kWave] = ss;
    __syncthreads();
    float t = 0.f;
#pragma unroll
    for (int wv = 0; wv < kPoolThreads / kWave; ++wv) t += red[wv];
    den = fmaxf(sqrtf(t), 1e-12f);  // F.normalize: e / max(||e||, eps)
  }
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int n = tid + i * kPoolThreads;
    if (n < H) out[(size_t)b * H + n] = normalize ? ev[i] / den : ev[i];
  }
}

}  // namespace

void pool_embed(const bf16* x, const float* fin, const float* gamma, const float* beta, const int32_t* lens,
                float* out, int B, int S, int H, int mode, int normalize, hipStream_t stream) {
  ATPU_CHECK(B > 0 && S >= 1 && S <= 512, "pool_embed: S must be in [1, 512]");
  ATPU_CHECK(H % 64 == 0 && H >= 64 && H <= 1024, "pool_embed: H must be a multiple of 64 in [64, 1024]");
  ATPU_CHECK(mode == kPoolMean || mode == kPoolCls, "pool_embed: mode must be mean (0) or cls (1)");
  ATPU_CHECK(x && lens && out, "pool_embed: null tensor");
  ATPU_CHECK(!fin || (gamma && beta), "pool_embed: fin needs gamma and beta");
  ATPU_CHECK(((reinterpret_cast<uintptr_t>(x) & 15) | (reinterpret_cast<uintptr_t>(fin) & 7) |
              (reinterpret_cast<uintptr_t>(out) & 3)) == 0, "pool_embed: x must be 16-byte and fin 8-byte aligned");
  const int R = kPoolThreads / (H / 8);  // whole rows per pass: 4 (H = 1024) .. 64 (H = 64)
  const int cls = mode == kPoolCls, nrm = normalize != 0;
  if (fin)
    hipLaunchKernelGGL((pool_embed_kernel<true>), dim3(B), dim3(kPoolThreads), 0, stream, x, fin, gamma, beta, lens,
                       out, S, H, R, cls, nrm);
  else
    hipLaunchKernelGGL((pool_embed_kernel<false>), dim3(B), dim3(kPoolThreads), 0, stream, x, fin, gamma, beta, lens,
                       out, S, H, R, cls, nrm);
  ATPU_HIP_CHECK(hipGetLastError());
}

}  // namespace atpu
