// Timing-only builds of the persistent 256x256 GEMM (the DBG template bits of gemm256s_kernel:
// results WRONG). The library carries no entry point that dispatches them; tools/gemm_ablate.py
// compiles this file, which includes the kernel source, into a library of its own and times a
// DBG build against the production instantiation of the same compile.
#include "../agent_tpu_amd/csrc/kernels/gemm_bf16.hip"

namespace atpu {
namespace {

template <int E, int L, int DBG>
void ablate_launch(const GemmArgs& g, hipStream_t s) {
  const int tiles = (g.M / 256) * (g.N / 256);
  int nb = std::min(tiles, num_cus());
  if (nb >= 8) nb &= ~7;
  const LnFold lf{g.in_fin, g.colsum, g.res_fin, g.gamma, g.part_out};
  hipLaunchKernelGGL((gemm256s_kernel<E, DBG, true, true, L>), dim3(nb), dim3(512), 0, s, g.A, g.lda, g.Bt, g.ldb, g.C,
                     g.ldc, g.bias, g.R, g.ldr, g.M, g.N, g.K, lf);
}

}  // namespace
}  // namespace atpu

// which: 0 = InNorm + GELU (FFN1), A and C in image order; 1 = ResNorm + StatsOut with residual
// (out-proj, FFN2), A, C and R in image order. dbg: 0 (production) or 512 (no LDS transposes).
// Returns 0, or -1 for an unknown (which, dbg) / shape, or the HIP error of the launch.
extern "C" __attribute__((visibility("default"))) int atpu_gemm_ablate(
    int which, int dbg, const void* A, const void* Bt, void* C, const float* bias, const void* R, int M, int N, int K,
    const float* in_fin, const float* colsum, const float* res_fin, const float* gamma, float* part_out, void* stream) {
  using namespace atpu;
  if (M % 256 || N % 256 || K % 256 || K < 256) return -1;
  GemmArgs g;
  g.A = static_cast<const bf16*>(A);
  g.lda = K;
  g.Bt = static_cast<const bf16*>(Bt);
  g.ldb = K;
  g.C = static_cast<bf16*>(C);
  g.ldc = N;
  g.bias = bias;
  g.R = static_cast<const bf16*>(R);
  g.ldr = N;
  g.M = M;
  g.N = N;
  g.K = K;
  g.in_fin = in_fin;
  g.colsum = colsum;
  g.res_fin = res_fin;
  g.gamma = gamma;
  g.part_out = part_out;
  hipStream_t s = static_cast<hipStream_t>(stream);
  constexpr int kFfn1 = kEpiBias | kEpiInNorm | kEpiGelu;
  constexpr int kRes = kEpiBias | kEpiResidual | kEpiResNorm | kEpiStatsOut;
  if (which == 0 && dbg == 0) ablate_launch<kFfn1, kLayA | kLayC, 0>(g, s);
  else if (which == 0 && dbg == 512) ablate_launch<kFfn1, kLayA | kLayC, 512>(g, s);
  else if (which == 1 && dbg == 0) ablate_launch<kRes, kLayA | kLayC | kLayR, 0>(g, s);
  else if (which == 1 && dbg == 512) ablate_launch<kRes, kLayA | kLayC | kLayR, 512>(g, s);
  else return -1;
  return static_cast<int>(hipGetLastError());
}
