// Rows with mask tokens ("atpu-fill v1", Python twin: agent_tpu_amd/tokenizer.py fill_rows).
//
// The host splits a text at every literal mask token; the m + 1 pieces are tokenized as ordinary
// single-segment rows [CLS] piece [SEP] (ids_s [Ns, S], lens_s [Ns]); the segments of row b are
// segoff[b] .. segoff[b+1] - 1. fill_assemble_kernel builds
//
//     [CLS] seg_0 [MASK] seg_1 [MASK] ... seg_m [SEP] [PAD]...
//
// from the pieces without their own [CLS] / [SEP]: the concatenation c = seg_0 MASK seg_1 ... seg_m
// of T tokens is cut to its first kept = min(T, S - 2), row position j holds c[j - 1], [SEP] sits at
// kept + 1 and lens = kept + 2. pos [B, M]: the row position of mask j, -1 where the row has fewer
// masks or the mask fell at or beyond position S - 1. All type_ids are 0 (not written).
//
// The frame of pair_assemble_kernel (rerank.hip): one 64-wide wave per row, four rows per workgroup;
// position j is a pure function of (j, the segments' lengths), a lane walks the row's segments (at
// most M + 1 <= 17) and reads at most one id of each; no LDS, no scan. Every index from device data
// is clamp-then-select: segoff into [0, Ns] (a decreasing pair is an empty range, more than M + 1
// segments are cut to M + 1), the segment index into [0, Ns - 1], lens_s into [2, S], and the token
// loads clamp their column into the row and discard what a position does not take.
#include "atpu/common.h"
#include "atpu/kernels.h"

namespace atpu {
namespace {

__device__ __forceinline__ int clampi(int x, int lo, int hi) { return min(max(x, lo), hi); }

__global__ __launch_bounds__(256) void fill_assemble_kernel(const int32_t* __restrict__ ids_s,
                                                            const int32_t* __restrict__ lens_s,
                                                            const int32_t* __restrict__ segoff,
                                                            int32_t* __restrict__ ids, int32_t* __restrict__ lens,
                                                            int32_t* __restrict__ pos, int B, int Ns, int S, int M,
                                                            int cls, int sep, int pad, int mask) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= B) return;
  const int s0 = clampi(segoff[row], 0, Ns);
  const int nseg = clampi(clampi(segoff[row + 1], 0, Ns) - s0, 0, M + 1);
  // T and the masks' positions: every lane walks the same <= 17 lengths
  int T = 0, mypos = -1;
  for (int i = 0; i < nseg; ++i) {
    const int n = clampi(lens_s[min(s0 + i, Ns - 1)], 2, S) - 2;
    T += n;
    if (i + 1 < nseg) {         // mask i follows segment i: concatenation index T, row position T + 1
      mypos = (lane == i && T < S - 2) ? T + 1 : mypos;
      T += 1;
    }
  }
  const int kept = min(T, S - 2);
  int32_t* out = ids + (size_t)row * S;
  for (int j = lane; j < S; j += 64) {
    const int c = j - 1;
    int32_t v = pad;
    int run = 0;
    for (int i = 0; i < nseg; ++i) {
      const int s = min(s0 + i, Ns - 1);
      const int n = clampi(lens_s[s], 2, S) - 2;
      const int32_t tok = ids_s[(size_t)s * S + clampi(1 + c - run, 0, S - 1)];
      v = (c >= run && c < run + n) ? tok : v;
      v = (c == run + n && i + 1 < nseg) ? mask : v;
      run += n + 1;
    }
    v = j > kept ? pad : v;
    v = j == kept + 1 ? sep : v;
    v = j == 0 ? cls : v;
    out[j] = v;
  }
  if (lane == 0) lens[row] = kept + 2;
  if (lane < M) pos[(size_t)row * M + lane] = mypos;
}

}  // namespace

void fill_assemble(const int32_t* ids_s, const int32_t* lens_s, const int32_t* segoff, int32_t* ids, int32_t* lens,
                   int32_t* pos, int B, int Ns, int S, int M, int cls, int sep, int pad, int mask,
                   hipStream_t stream) {
  ATPU_CHECK(S >= 3, "fill_assemble: S must be >= 3");
  ATPU_CHECK(M >= 1 && M <= 16, "fill_assemble: M must be in [1, 16]");
  if (B <= 0) return;
  ATPU_CHECK(Ns >= 1, "fill_assemble: Ns must be >= 1");
  ATPU_CHECK(ids_s && lens_s && segoff && ids && lens && pos, "fill_assemble: null tensor");
  hipLaunchKernelGGL(fill_assemble_kernel, dim3((B + 3) / 4), dim3(256), 0, stream, ids_s, lens_s, segoff, ids, lens,
                     pos, B, Ns, S, M, cls, sep, pad, mask);
  ATPU_HIP_CHECK(hipGetLastError());
}

}  // namespace atpu
