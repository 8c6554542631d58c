// [CLS] attention of the last BERT layer with the K / V projection re-associated away
// (ops/cls_attend.py has the algebra): per sequence, the 128 raw hidden rows g_j (pre-LN sums,
// statistics (rstd, rstd*mu) in fin) are the keys AND the values,
//   s_hj = rstd_j (U_h . g_j) - rstd_j mu_j sum(U_h),   p_h = softmax_{j < len} s_h,
//   Z_h  = sum_j (p_hj rstd_j) g_j - (sum_j p_hj rstd_j mu_j) . 1
// with one projected query U_h [H] per head. One workgroup (8 waves) per sequence; the heads
// are the 16 columns of a v_mfma_f32_16x16x32_bf16 tile (columns >= heads repeat the last
// head and are never stored).
//
// g of one sequence is 128 x H bf16 (192 KiB at H = 768): it does not fit the 160 KiB LDS.
// It is staged by LDS-DMA as 64-column chunks, one chunk = a [128][128 B] image (asw swizzle:
// conflict-free for the row reads of pass 1 and the transposed reads of pass 2) in a ring of
// 9 buffers (144 KiB):
//   pass 1 (scores): wave w stages and reads ONLY key rows 16w..16w+15 of every chunk, so the
//     pass needs no barrier: counted vmcnt waits, 2 MFMAs per chunk (+2 with a ones operand
//     that sum U_h), chunk c + 9 staged into chunk c's buffer as soon as c is read. The 16 x 16
//     fp32 score blocks meet in LDS.
//   pass 2 (context): every wave redoes the softmax of all 128 keys for its lanes' heads
//     (32 scores per lane, registers), then the 16-column tiles of the chunks are dealt
//     round-robin to the waves (2 chunks per step), chunks still resident first. The
//     NCH - 9 chunks pass 1 overwrote (3 of 12 at H = 768, 7 of 16 at H = 1024) are read again
//     from L2 / MALL into buffers pass 2 has finished with: 25 % (44 %) more L2 traffic, no
//     more HBM traffic, issued 3+ steps ahead of their use.
// P.rstd is rounded to bf16 (the MFMA operand) and the mu term is summed with the same rounded
// weights; the row sum l_h is the fp32 sum of the unrounded exponentials. The context leaves
// through LDS as whole 16-B chunks of the sequence's contiguous [heads * H] output. No atomics;
// every reduction has a fixed order, so a sequence's bits do not depend on the batch.
//
// B = 1024, H = 768: 240 MB of traffic (floor ~40 us at 6 TB/s), measured 69.8 us (docs/PERF_NOTES.md).
//
// Keys >= len: the staged row index is clamped to len - 1 (a valid row: nothing is computed
// from rows the encoder only padded), the score is then replaced by -1e30 and the weight by 0.
// len is clamped to [1, 128] (the tokenizer never gives less than 2: [CLS] [SEP]).
#include "atpu/common.h"
#include "atpu/kernels.h"
#include "atpu/lds_ops.h"

#include <type_traits>
#include <utility>

namespace atpu {
namespace {

constexpr int kCBufs = 9;                        // chunk images in LDS
constexpr int kScStride = 132;                   // floats per head row of the score block (128 + pad)
constexpr int kScOff = kCBufs * kAttnImg;
constexpr int kCLds = kScOff + 16 * kScStride * 4;
static_assert(kCLds <= 160 * 1024, "LDS budget");

template <class F, int... Is>
__device__ __forceinline__ void static_for_impl(F&& f, std::integer_sequence<int, Is...>) {
  (f(std::integral_constant<int, Is>{}), ...);
}
template <int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
  static_for_impl(f, std::make_integer_sequence<int, N>{});
}

// 16-B global load the compiler's wait-count pass does not see (offset OFF bytes from p)
template <int OFF, class T>
__device__ __forceinline__ void gload16(T& dst, const void* p) {
  static_assert(sizeof(T) == 16 && OFF >= 0 && OFF < 4096, "gload16");
  asm volatile("global_load_dwordx4 %0, %1, off offset:%2" : "=&v"(dst) : "v"(p), "n"(OFF) : "memory");
}

// NCH = H / 64 chunks
template <int NCH>
__global__ __launch_bounds__(512, 1) void cls_attend_kernel(const bf16* __restrict__ g, const float* __restrict__ fin,
                                                            const bf16* __restrict__ U,
                                                            const int32_t* __restrict__ lens, bf16* __restrict__ Z,
                                                            int heads) {
  constexpr int H = NCH * 64;
  constexpr int kEv = NCH > kCBufs ? NCH - kCBufs : 0;  // chunks pass 1 overwrites, pass 2 re-reads
  constexpr int kSteps = NCH / 2;                       // pass 2: two chunks (8 column tiles) per step
  constexpr int kZStride = H * 2 + 16;                  // bytes per head row of the staged output
  static_assert(NCH % 2 == 0 && kEv + 2 <= kCBufs && 16 * kZStride <= kScOff, "chunk ring");
  __shared__ __attribute__((aligned(16))) char lds[kCLds];
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fr = lane & 15, fc = lane >> 4;
  const int b = blockIdx.x;
  const int len = min(max(lens[b], 1), 128);
  const bf16* gb = g + (size_t)b * 128 * H;

  // ---- registers first (oldest in the vmcnt order): statistics of the lane's 32 keys
  // (16 kt + 4 fc + e, the MFMA output rows it holds) and the queries U [head fr][8 fc ..].
  // Loaded by inline asm: a load the compiler tracks makes it drain the whole LDS-DMA stream
  // (vmcnt(0)) at the value's first use. The counted wait of chunk 0 retires them (in-order
  // return); the registers pass through the waits that precede their first use.
  f32x4 fv[8][2];
  {
    const float* fb = fin + (size_t)b * 256 + fc * 8;
    static_for<8>([&](auto kk) {
      constexpr int kt = decltype(kk)::value;
      gload16<kt * 128>(fv[kt][0], fb);
      gload16<kt * 128 + 16>(fv[kt][1], fb);
    });
  }
  bf16x8 uf[NCH][2];
  {
    // columns fr >= heads of the tile repeat the last head (index clamped): computed, never stored
    const bf16* ub = U + ((size_t)b * heads + min(fr, heads - 1)) * H + fc * 8;
    static_for<NCH>([&](auto cc) {
      constexpr int c = decltype(cc)::value;
      gload16<c * 128>(uf[c][0], ub);
      gload16<c * 128 + 64>(uf[c][1], ub);
    });
  }
  __builtin_amdgcn_sched_barrier(0);

  // ---- staging: the wave's 16 key rows of chunk c -> image buf (2 x 1 KiB LDS-DMA)
  const char* srow[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int r = w * 16 + i * 8 + (lane >> 3);
    srow[i] = reinterpret_cast<const char*>(gb + (size_t)min(r, len - 1) * H + asw(r, lane & 7) * 8);
  }
  auto stage = [&](int c, int buf) {
#pragma unroll
    for (int i = 0; i < 2; ++i) glds16(srow[i] + c * 128, lds + buf * kAttnImg + (w * 16 + i * 8) * 128);
  };
  static_for<(NCH < kCBufs ? NCH : kCBufs)>([&](auto cc) { stage(cc.value, cc.value); });

  // ---- pass 1: raw scores of key rows 16w.. (lane: keys 16w + 4fc + e, head fr), sum(U_h)
  bf16x8 ones;
#pragma unroll
  for (int e = 0; e < 8; ++e) ones[e] = (bf16)1.0f;
  f32x4 sacc = {0.f, 0.f, 0.f, 0.f}, usum = {0.f, 0.f, 0.f, 0.f};
  {
    const int r1 = w * 16 + fr;
    const char* rd = lds + r1 * 128;
    const int sl0 = asw(r1, fc) * 16, sl1 = asw(r1, 4 + fc) * 16;
    static_for<NCH>([&](auto cc) {
      constexpr int c = decltype(cc)::value;
      constexpr int staged = NCH < kCBufs + c ? NCH : kCBufs + c;  // chunks issued so far
      asm volatile("s_waitcnt vmcnt(%2)" : "+v"(uf[c][0]), "+v"(uf[c][1]) : "n"(2 * (staged - c - 1)) : "memory");
      const char* img = rd + (c % kCBufs) * kAttnImg;
      bf16x8 g0 = ds_read128(img + sl0);
      bf16x8 g1 = ds_read128(img + sl1);
      lgkm_wait<0>(g0, g1);
      sacc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(g0, uf[c][0], sacc, 0, 0, 0);
      sacc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(g1, uf[c][1], sacc, 0, 0, 0);
      usum = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones, uf[c][0], usum, 0, 0, 0);
      usum = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones, uf[c][1], usum, 0, 0, 0);
      if constexpr (c + kCBufs < NCH) stage(c + kCBufs, c % kCBufs);
    });
  }
  float* sc = reinterpret_cast<float*>(lds + kScOff) + fr * kScStride + fc * 4;
  *reinterpret_cast<f32x4*>(sc + w * 16) = sacc;
  // every wave's DMA has landed and its score block is written (fv: loaded long ago, first used below)
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier"
               : "+v"(fv[0][0]), "+v"(fv[0][1]), "+v"(fv[1][0]), "+v"(fv[1][1]), "+v"(fv[2][0]), "+v"(fv[2][1]),
                 "+v"(fv[3][0]), "+v"(fv[3][1]), "+v"(fv[4][0]), "+v"(fv[4][1]), "+v"(fv[5][0]), "+v"(fv[5][1]),
                 "+v"(fv[6][0]), "+v"(fv[6][1]), "+v"(fv[7][0]), "+v"(fv[7][1])::"memory");

  // ---- softmax over the 128 keys of head fr (this lane: keys 16 kt + 4 fc + e)
  bf16x8 pf[4];  // P.rstd in bf16, B operand of key step ks (keys 32 ks + {4fc + e, 16 + 4fc + e})
  float inv, csum;
  {
    const float su = usum[0];
    float x[8][4];
    float mx = -1e30f;
#pragma unroll
    for (int kt = 0; kt < 8; ++kt) {
      const f32x4 s4 = *reinterpret_cast<const f32x4*>(sc + kt * 16);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float rstd = fv[kt][e >> 1][(e & 1) * 2], rm = fv[kt][e >> 1][(e & 1) * 2 + 1];
        const float v = fmaf(rstd, s4[e], -rm * su);
        x[kt][e] = kt * 16 + fc * 4 + e < len ? v : -1e30f;
        mx = fmaxf(mx, x[kt][e]);
      }
    }
    constexpr float kLog2e = 1.4426950408889634f;
    const float moff = lane_rows_max(mx) * kLog2e;
    float l = 0.f, cs = 0.f;
#pragma unroll
    for (int kt = 0; kt < 8; ++kt)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const bool live = kt * 16 + fc * 4 + e < len;
        const float rstd = fv[kt][e >> 1][(e & 1) * 2], rm = fv[kt][e >> 1][(e & 1) * 2 + 1];
        const float ex = __builtin_amdgcn_exp2f(fmaf(x[kt][e], kLog2e, -moff));  // 0 for masked keys
        l += ex;
        const bf16 wb = f2bf(live ? ex * rstd : 0.f);
        cs += live ? bf2f(wb) * (rm * __builtin_amdgcn_rcpf(rstd)) : 0.f;  // weight x mu
        pf[kt >> 1][(kt & 1) * 4 + e] = wb;
      }
    inv = 1.f / lane_rows_sum(l);  // l >= 1: the row maximum contributes exp2(0)
    csum = lane_rows_sum(cs);
  }

  // ---- pass 2: Z tile (16 columns x 16 heads) = g^T (transposed reads) . P, all 128 keys
  const int half = w >> 2, dt = w & 3;
  f32x4 o[kSteps];
  {
    const int tq = (lane >> 2) & 3, tp = lane & 3;
    const int k0 = fc * 4 + tq;  // (k0 + 32 ks (+ 16)) & 7 == k0 & 7
    const char* vrow = lds + k0 * 128 + (tp & 1) * 8 + asw(k0, dt * 2 + (tp >> 1)) * 16;
    static_for<kSteps>([&](auto ss) {
      constexpr int s = decltype(ss)::value;
      // position p of the order holds chunk (kEv + p) % NCH: resident chunks first. An
      // overwritten chunk e < kEv comes back into the buffer of position e.
      constexpr int c0 = (kEv + 2 * s) % NCH, c1 = (kEv + 2 * s + 1) % NCH;
      constexpr int b0 = (c0 >= kEv ? c0 : kEv + c0) % kCBufs, b1 = (c1 >= kEv ? c1 : kEv + c1) % kCBufs;
      if constexpr (kEv > 0 && 2 * s + 1 >= NCH - kEv)  // a re-read chunk: every wave's rows have landed
        asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
      const char* img = vrow + (half ? b1 : b0) * kAttnImg;
      bf16x4 vl[4], vh[4];
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        vl[ks] = tr16(img + ks * 32 * 128);
        vh[ks] = tr16(img + (ks * 32 + 16) * 128);
      }
      asm volatile("s_waitcnt lgkmcnt(0)"
                   : "+v"(vl[0]), "+v"(vl[1]), "+v"(vl[2]), "+v"(vl[3]), "+v"(vh[0]), "+v"(vh[1]), "+v"(vh[2]),
                     "+v"(vh[3])::"memory");
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        bf16x8 vf;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          vf[e] = vl[ks][e];
          vf[4 + e] = vh[ks][e];
        }
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf[ks], acc, 0, 0, 0);
      }
      o[s] = acc;
      if constexpr (2 * s < kEv) {
        // positions 2s, 2s + 1 are read by all waves: their buffers take chunks 2s (, 2s + 1) again
        asm volatile("s_barrier" ::: "memory");
        stage(2 * s, b0);
        if constexpr (2 * s + 1 < kEv) stage(2 * s + 1, b1);
      }
    });
  }
  // ---- output through LDS (the images are dead): [16][H] bf16, padded rows
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
  static_for<kSteps>([&](auto ss) {
    constexpr int s = decltype(ss)::value;
    constexpr int c0 = (kEv + 2 * s) % NCH, c1 = (kEv + 2 * s + 1) % NCH;
    const int col = (half ? c1 : c0) * 64 + dt * 16 + fc * 4;  // lane: columns col..col+3 of head fr
    typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
    *reinterpret_cast<u32x2*>(lds + fr * kZStride + col * 2) =
        u32x2{pack_bf16x2((o[s][0] - csum) * inv, (o[s][1] - csum) * inv),
              pack_bf16x2((o[s][2] - csum) * inv, (o[s][3] - csum) * inv)};
  });
  __syncthreads();
  bf16* zb = Z + (size_t)b * heads * H;
  for (int idx = tid; idx < heads * (H / 8); idx += 512) {
    const int h = idx / (H / 8), n8 = idx % (H / 8);
    *reinterpret_cast<u32x4*>(zb + h * H + n8 * 8) = *reinterpret_cast<const u32x4*>(lds + h * kZStride + n8 * 16);
  }
}

}  // namespace

void cls_attend(const bf16* g, const float* fin, const bf16* U, const int32_t* lens, bf16* Z, int B, int S, int H,
                int heads, hipStream_t stream) {
  ATPU_CHECK(B > 0 && S == 128, "cls_attend: sequences of exactly 128 tokens");
  ATPU_CHECK(H % 256 == 0 && H >= 256 && H <= 1024, "cls_attend: H must be 256, 512, 768 or 1024");
  ATPU_CHECK(heads >= 1 && heads <= 16 && heads * 64 == H, "cls_attend: at most 16 heads of 64");
  ATPU_CHECK(g && fin && U && lens && Z, "cls_attend: null tensor");
  ATPU_CHECK(((reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(fin) | reinterpret_cast<uintptr_t>(U) |
               reinterpret_cast<uintptr_t>(Z)) & 15) == 0, "cls_attend: tensors must be 16-byte aligned");
#define ATPU_CLS(N) \
  hipLaunchKernelGGL((cls_attend_kernel<N>), dim3(B), dim3(512), 0, stream, g, fin, U, lens, Z, heads)
  switch (H / 64) {
    case 4: ATPU_CLS(4); break;
    case 8: ATPU_CLS(8); break;
    case 12: ATPU_CLS(12); break;
    default: ATPU_CLS(16); break;
  }
#undef ATPU_CLS
  ATPU_HIP_CHECK(hipGetLastError());
}

}  // namespace atpu
