// INT8 (W8A8) GEMM on the i8 MFMA, with the row quantiser that feeds it.
//
//   q[r,k]   = clamp(rint(x[r,k] * (127 / amax_r)), -127, 127),  scale[r] = amax_r / 127
//   acc[m,n] = sum_k Aq[m,k] * Wq[n,k]                            (int32, exact for K <= 2^17)
//   C[m,n]   = bf16( act(float(acc) * a_scale[m] * b_scale[n] + bias[n]) + R[m,n] )
//
// Symmetric, 127 levels, no zero points; every scale operation is one IEEE fp32 operation
// (no contraction), so the PyTorch twins in ops/linear_i8.py reproduce q and scale bit for bit
// and the raw accumulators exactly.
//
// Structure: the 128x128 bf16 kernel of gemm_bf16.hip with one byte per element. A staged row
// is still 128 B (now 128 k values = two v_mfma_i32_16x16x64_i8 steps), so the glds staging, the
// XOR swizzle on the 16-B chunk and the swapped MFMA operands (each lane owns 4 consecutive
// output columns of one row) carry over unchanged. One kernel family for every M and no
// split-K: a row's result does not depend on the batch it is launched in.
#include "atpu/common.h"
#include "atpu/kernels.h"
#include "atpu/ln_row.h"
#include "atpu/quant_i8.h"

namespace atpu {
namespace {

typedef int i32x4 __attribute__((ext_vector_type(4)));

constexpr int kTile = 128;      // output tile (rows and columns) of a workgroup
constexpr int kRowBytes = 128;  // K bytes (= int8 values) per staged row
constexpr int kMaxK = 1 << 17;  // 2^17 * 127^2 < 2^31: the int32 accumulator cannot overflow

__device__ __forceinline__ int swz(int row, int chunk) { return chunk ^ ((row >> 1) & 7); }

// ------------------------------------------------------------------ row quantiser
// one wave per row; NC 16-byte chunks (8 bf16) per lane stay in registers between the amax
// pass and the quantise pass, longer rows re-read the rest
template <int NC>
__global__ __launch_bounds__(256) void quantize_rows_i8_kernel(const bf16* __restrict__ x, int ldx,
                                                               int8_t* __restrict__ q, int ldq,
                                                               float* __restrict__ scale, int rows, int K) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (row >= rows) return;  // wave-uniform
  const bf16* xr = x + (size_t)row * ldx;
  int8_t* qr = q + (size_t)row * ldq;
  const int nch = K / 8;
  bf16x8 v[NC];
  float amax = 0.f;
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    // clamped chunk, unconditional load: a repeated chunk leaves the maximum unchanged
    const int ic = min(lane + 64 * c, nch - 1);
    v[c] = *reinterpret_cast<const bf16x8*>(xr + ic * 8);
    amax = absmax_bf16x8(v[c], amax);
  }
  for (int ic = lane + 64 * NC; ic < nch; ic += 64)
    amax = absmax_bf16x8(*reinterpret_cast<const bf16x8*>(xr + ic * 8), amax);
  amax = wave_max(amax);
  const float2 si = quant_scale_inv(amax);
  if (lane == 0) scale[row] = si.x;
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const int ic = lane + 64 * c;
    if (ic < nch) *reinterpret_cast<u32x2*>(qr + ic * 8) = quant_pack8(v[c], si.y);
  }
  for (int ic = lane + 64 * NC; ic < nch; ic += 64)
    *reinterpret_cast<u32x2*>(qr + ic * 8) = quant_pack8(*reinterpret_cast<const bf16x8*>(xr + ic * 8), si.y);
}

// layernorm_hw_kernel (norm_embed.hip) with the quantised row as a second output
template <int NG>
__global__ __launch_bounds__(256) void layernorm_quant_i8_kernel(const bf16* __restrict__ x,
                                                                 const bf16* __restrict__ res,
                                                                 const float* __restrict__ gamma,
                                                                 const float* __restrict__ beta,
                                                                 bf16* __restrict__ out, int8_t* __restrict__ q,
                                                                 float* __restrict__ scale, int rows, float eps) {
  const int hl = threadIdx.x & 31;
  const int row = blockIdx.x * 8 + (threadIdx.x >> 5);
  const bool live = row < rows;
  const int r = live ? row : rows - 1;  // dead half-waves read a valid row, never store
  constexpr int N = NG * 256;
  ln_hw_row<NG, true, true>(x + (size_t)r * N, res ? res + (size_t)r * N : nullptr, gamma, beta, out + (size_t)r * N,
                            live, eps, hl, q + (size_t)r * N, scale + r);
}

// ------------------------------------------------------------------ GEMM
// 256 threads, 4 waves as 2x2, 64x64 per wave (16 accumulators of 4 int32). RAW: write the
// int32 accumulators to acc_out and nothing else.
template <int EPI, bool RAW>
__global__ __launch_bounds__(256, 2) void gemm_i8_kernel(const int8_t* __restrict__ A, int lda,
                                                         const float* __restrict__ a_scale,
                                                         const int8_t* __restrict__ Bt, int ldb,
                                                         const float* __restrict__ b_scale, bf16* __restrict__ C,
                                                         int ldc, const float* __restrict__ bias,
                                                         const bf16* __restrict__ R, int ldr, int M, int N, int K,
                                                         int32_t* __restrict__ acc_out, int ldacc) {
  constexpr int NW = 4, TM = 4, TN = 4;
  constexpr int A_BYTES = kTile * kRowBytes;
  constexpr int STAGE_BYTES = 2 * A_BYTES;
  __shared__ __attribute__((aligned(16))) char lds[2 * STAGE_BYTES];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ntn = (N + kTile - 1) / kTile;
  const int ntm = (M + kTile - 1) / kTile;
  const int tile = xcd_remap(blockIdx.x, ntm * ntn);
  const int m0 = (tile / ntn) * kTile;
  const int n0 = (tile % ntn) * kTile;

  // ---- per-lane staging sources: wave-instruction i covers staged rows [(i*NW+wave)*8, +8);
  // rows past the edge are clamped (their products are never stored), and so is the k offset
  // of the half stage a K % 128 == 64 problem ends with (its second half is never multiplied)
  const int srow = lane >> 3, spos = lane & 7;
  const int8_t* a_src[kTile / 8 / NW];
  const int8_t* b_src[kTile / 8 / NW];
  int schunk[kTile / 8 / NW];
#pragma unroll
  for (int i = 0; i < kTile / 8 / NW; ++i) {
    const int r = (i * NW + wave) * 8 + srow;
    a_src[i] = A + (size_t)min(m0 + r, M - 1) * lda;
    b_src[i] = Bt + (size_t)min(n0 + r, N - 1) * ldb;
    schunk[i] = swz(r, spos) * 16;
  }
  auto stage = [&](int kt, int buf) {
    char* base = lds + buf * STAGE_BYTES;
#pragma unroll
    for (int i = 0; i < kTile / 8 / NW; ++i) {
      const int koff = min(kt * kRowBytes + schunk[i], K - 16);
      glds16(a_src[i] + koff, base + (i * NW + wave) * 8 * kRowBytes);
      glds16(b_src[i] + koff, base + A_BYTES + (i * NW + wave) * 8 * kRowBytes);
    }
  };

  const int wm = wave >> 1, wn = wave & 1;
  const int arow0 = wm * 64, brow0 = wn * 64;
  i32x4 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = i32x4{0, 0, 0, 0};

  // both operands take the 16 bytes at k = 64 ks + 16 (lane >> 4) of row lane & 15
  const int frow = lane & 15, fchunk = lane >> 4;
  auto compute = [&](int buf, int ksteps) {
    const char* base = lds + buf * STAGE_BYTES;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      if (ks < ksteps) {
        i32x4 af[TM], bfg[TN];
#pragma unroll
        for (int i = 0; i < TM; ++i) {
          const int r = arow0 + i * 16 + frow;
          af[i] = *reinterpret_cast<const i32x4*>(base + r * kRowBytes + swz(r, ks * 4 + fchunk) * 16);
        }
#pragma unroll
        for (int j = 0; j < TN; ++j) {
          const int r = brow0 + j * 16 + frow;
          bfg[j] = *reinterpret_cast<const i32x4*>(base + A_BYTES + r * kRowBytes + swz(r, ks * 4 + fchunk) * 16);
        }
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(bfg[j], af[i], acc[i][j], 0, 0, 0);
      }
    }
  };

  const int nk = (K + kRowBytes - 1) / kRowBytes;
  stage(0, 0);
  wait_vmcnt0();
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const int cur = kt & 1;
    if (kt + 1 < nk) stage(kt + 1, cur ^ 1);
    compute(cur, min(2, (K - kt * kRowBytes) / 64));
    wait_vmcnt0();
    __syncthreads();
  }

  // ---- epilogue: lane owns C[m][n..n+3] of each (i, j) fragment. Indices are clamped and the
  // loads unconditional; only the stores are predicated.
#pragma unroll
  for (int i = 0; i < TM; ++i) {
    const int m = m0 + arow0 + i * 16 + frow;
    const size_t mc = min(m, M - 1);
    float as = 1.f;
    if constexpr (!RAW) as = a_scale[mc];
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int n = n0 + brow0 + j * 16 + fchunk * 4;
      const int nc = min(n, N - 4);
      const bool live = m < M && n < N;
      if constexpr (RAW) {
        if (live) *reinterpret_cast<i32x4*>(acc_out + mc * ldacc + nc) = acc[i][j];
      } else {
#pragma clang fp contract(off)
        const f32x4 ws = *reinterpret_cast<const f32x4*>(b_scale + nc);
        f32x4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = static_cast<float>(acc[i][j][e]) * as * ws[e];
        if constexpr (EPI & kEpiBias) v += *reinterpret_cast<const f32x4*>(bias + nc);
        if constexpr (EPI & kEpiGelu) {
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = gelu_poly1(v[e]);
        }
        if constexpr (EPI & kEpiResidual) {
          const bf16x4 r = *reinterpret_cast<const bf16x4*>(R + mc * ldr + nc);
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] += bf2f(r[e]);
        }
        bf16x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = f2bf(v[e]);
        if (live) *reinterpret_cast<bf16x4*>(C + mc * ldc + nc) = o;
      }
    }
  }
}

template <int EPI, bool RAW>
void launch_gemm_i8(const GemmI8Args& g, hipStream_t stream) {
  const int blocks = ((g.M + kTile - 1) / kTile) * ((g.N + kTile - 1) / kTile);
  hipLaunchKernelGGL((gemm_i8_kernel<EPI, RAW>), dim3(blocks), dim3(256), 0, stream, g.A, g.lda, g.a_scale, g.Bt,
                     g.ldb, g.b_scale, g.C, g.ldc, g.bias, g.R, g.ldr, g.M, g.N, g.K, g.acc_out, g.ldacc);
}

bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace

bool gemm_i8_ok(int M, int N, int K) {
  return M >= 1 && N >= 16 && N % 16 == 0 && K >= 64 && K % 64 == 0 && K <= kMaxK &&
         ((int64_t)M + kTile - 1) / kTile * (((int64_t)N + kTile - 1) / kTile) < (1ll << 31);
}

void quantize_rows_i8(const bf16* x, int ldx, int8_t* q, int ldq, float* scale, int rows, int K,
                      hipStream_t stream) {
  ATPU_CHECK(rows > 0 && K > 0 && K % 16 == 0, "quantize_rows_i8: K must be a positive multiple of 16");
  ATPU_CHECK(x && q && scale, "quantize_rows_i8: null operand");
  ATPU_CHECK(ldx >= K && ldx % 8 == 0 && ldq >= K && ldq % 8 == 0 && aligned(x, 16) && aligned(q, 8),
             "quantize_rows_i8: rows must keep 16-B (x) / 8-B (q) alignment");
  const dim3 grid((rows + 3) / 4), block(256);
  if (K <= 1024)
    hipLaunchKernelGGL((quantize_rows_i8_kernel<2>), grid, block, 0, stream, x, ldx, q, ldq, scale, rows, K);
  else if (K <= 3072)
    hipLaunchKernelGGL((quantize_rows_i8_kernel<6>), grid, block, 0, stream, x, ldx, q, ldq, scale, rows, K);
  else
    hipLaunchKernelGGL((quantize_rows_i8_kernel<8>), grid, block, 0, stream, x, ldx, q, ldq, scale, rows, K);
  ATPU_HIP_CHECK(hipGetLastError());
}

void layernorm_quant_i8(const bf16* x, const bf16* res, const float* gamma, const float* beta, bf16* out, int8_t* q,
                        float* scale, int rows, int N, float eps, hipStream_t stream) {
  ATPU_CHECK(N % 256 == 0 && N <= 2048, "row width must be a multiple of 256, <= 2048");
  ATPU_CHECK(x && gamma && beta && out && q && scale, "layernorm_quant_i8: null operand");
  if (rows <= 0) return;
  const dim3 grid((rows + 7) / 8), block(256);
#define ATPU_LNQ(NG_) \
  case NG_: hipLaunchKernelGGL(layernorm_quant_i8_kernel<NG_>, grid, block, 0, stream, x, res, gamma, beta, out, q, scale, rows, eps); break
  switch (N / 256) {
    ATPU_LNQ(1);
    ATPU_LNQ(2);
    ATPU_LNQ(3);
    ATPU_LNQ(4);
    ATPU_LNQ(6);
    ATPU_LNQ(8);
    default: throw std::invalid_argument("atpu: unsupported row width " + std::to_string(N));
  }
#undef ATPU_LNQ
  ATPU_HIP_CHECK(hipGetLastError());
}

void gemm_i8(const GemmI8Args& g, hipStream_t stream) {
  ATPU_CHECK(gemm_i8_ok(g.M, g.N, g.K), "gemm_i8: needs M >= 1, N % 16 == 0, K % 64 == 0, K <= 2^17");
  ATPU_CHECK(g.A && g.Bt && g.lda >= g.K && g.ldb >= g.K && g.lda % 16 == 0 && g.ldb % 16 == 0 &&
                 aligned(g.A, 16) && aligned(g.Bt, 16),
             "gemm_i8: operands must keep 16-B rows");
  if (g.acc_out) {
    ATPU_CHECK(g.ldacc >= g.N && g.ldacc % 4 == 0 && aligned(g.acc_out, 16), "gemm_i8: acc_out must keep 16-B rows");
    launch_gemm_i8<0, true>(g, stream);
    ATPU_HIP_CHECK(hipGetLastError());
    return;
  }
  ATPU_CHECK(g.a_scale && g.b_scale && aligned(g.b_scale, 16), "gemm_i8: scales missing (b_scale 16-B aligned)");
  ATPU_CHECK(g.C && g.ldc >= g.N && g.ldc % 4 == 0 && aligned(g.C, 8), "gemm_i8: C must keep 8-B rows");
  ATPU_CHECK(!(g.epi & kEpiBias) || (g.bias && aligned(g.bias, 16)), "gemm_i8: bias epilogue without (aligned) bias");
  ATPU_CHECK(!(g.epi & kEpiResidual) || (g.R && g.ldr >= g.N && g.ldr % 4 == 0 && aligned(g.R, 8)),
             "gemm_i8: residual epilogue without R (8-B rows)");
  switch (g.epi) {  // the encoder's epilogues: QKV (bias), FFN1 (bias, GELU), out-projection / FFN2 (bias, residual)
    case 0: launch_gemm_i8<0, false>(g, stream); break;
    case kEpiBias: launch_gemm_i8<kEpiBias, false>(g, stream); break;
    case kEpiBias | kEpiGelu: launch_gemm_i8<kEpiBias | kEpiGelu, false>(g, stream); break;
    case kEpiBias | kEpiResidual: launch_gemm_i8<kEpiBias | kEpiResidual, false>(g, stream); break;
    default: ATPU_CHECK(false, "gemm_i8: epilogue must be none, Bias, Bias|Gelu or Bias|Residual");
  }
  ATPU_HIP_CHECK(hipGetLastError());
}

}  // namespace atpu
