// Masked multi-head attention for 32-wide heads (MiniLM-class BERT encoders: hidden 384 =
// 12 heads of 32). Same math as attention_fwd_kernel (attention.hip): bf16 in, fp32 scores and
// online softmax, keys k >= lens[b] masked, bf16 out; not causal, no bias.
//
//   O[b,q,h,:] = softmax_k( scale * Q[b,q,h]·K[b,k,h] ) · V[b,k,h,:]
//
// Work split: HEAD PAIRS. Two adjacent heads' K (or V) columns are 64 contiguous bf16 = 128 B
// per key row, exactly the row image the D = 64 kernel stages by LDS-DMA (8 lanes x 16 B per
// row, 8 rows per wave instruction). One workgroup of 8 waves serves one (batch item, head
// pair, block of 128 queries): it stages both heads' K and V chunks of 128 keys (16 KiB +
// 16 KiB), waves 0-3 compute the even head and waves 4-7 the odd head. A wave owns 32 queries
// = two 16-query MFMA column tiles, so every K fragment and every transposed V fragment read
// from LDS feeds two MFMAs (the D = 64 tile reads one fragment per MFMA).
//  * S^T = K·Q^T: D = 32 is the K-depth of ONE v_mfma_f32_16x16x32_bf16, so a 16x16 score tile
//    is one MFMA with no d-loop. Keys sit in the accumulator rows and the query on the lane:
//    row max / row sum are in-register plus the lane_rows_* permlane swaps, and P^T is already
//    the B operand of O^T = V^T·P^T.
//  * PV: two d-tiles per head, V gathered by ds_read_b64_tr_b16 from the row-major image.
//  * Key tiles and 32-key PV steps that lie wholly past len are skipped (wave-uniform).
//  * O leaves through LDS (the K half, free after the last chunk): the two heads' 64-B halves
//    are joined so each store instruction writes whole 128-B rows of a head pair.
//  * An odd head count leaves a last pair with one head: the staging then fetches the even
//    head's 64 B twice instead of the columns past H*32, waves 4-7 skip the compute, and only
//    the even half of the O rows is stored.
//
// LDS bank analysis (64 banks x 4 B: a 256-B bank row is two 128-B key rows; rows r and r+1
// differ in which 128-B half they occupy, rows r and r+2 alias). Both swizzles XOR the 16-B
// chunk index (3 bits) with bits of the row; XOR with a fixed value is a bijection of the 8
// chunk positions whatever the base chunk is, which is why the argument survives a wave
// reading only its head's 64-B half (chunks hsel*4 .. hsel*4+3) of every row:
//  * K, ds_read_b128: a 16-lane phase (fixed fg) reads chunk hsel*4+fg of 16 consecutive rows
//    at position chunk ^ ((row>>1)&7). The 8 row pairs get 8 distinct positions and the two
//    rows of a pair the two halves of the bank row: 16 distinct 16-B slots, conflict-free.
//    (Swizzling only inside a head's half, chunk ^ ((row>>1)&3), would alias rows r and r+8.)
//  * V, ds_read_b64_tr_b16: a 32-lane half reads a 32-B chunk pair (one d-tile) of 8
//    consecutive rows at pair position pair ^ ((row>>1)&3): 4 row pairs -> 4 distinct 32-B
//    positions x 2 halves of the bank row = 8 distinct 32-B groups, conflict-free.
//  * O staging uses the K swizzle: the 8-B writes of a 32-lane half cover 16 rows x 16 B and
//    the 16-B reads of a 16-lane phase 2 rows x 128 B, both 256 distinct bytes of a bank row.
// Because the XOR reaches bit 2 of the chunk index the two heads' halves interleave in LDS;
// nothing relies on them being apart (the one-head pair only redirects its global reads).
#include "atpu/common.h"
#include "atpu/kernels.h"

#include <algorithm>

namespace atpu {
namespace {

constexpr int kD = 32;
constexpr int kKC = 128;         // keys per chunk
constexpr int kQB = 128;         // queries per workgroup (of each head of the pair)
constexpr int kRowB = 2 * kD * 2;  // 128 B: one key row of a head pair
constexpr int kLdsK = kKC * kRowB;  // 16 KiB
constexpr int kLdsV = kKC * kRowB;  // 16 KiB
constexpr int kWaves = 8;
constexpr int kThreads = kWaves * 64;
constexpr float kLog2e = 1.4426950408889634f;

__device__ __forceinline__ int kswz(int row, int chunk) { return chunk ^ ((row >> 1) & 7); }
__device__ __forceinline__ int vswz(int row, int chunk) { return chunk ^ (((row >> 1) & 3) << 1); }

typedef short v4s __attribute__((vector_size(8)));
// ds_read_b64_tr_b16: per 16-lane group, lane 4q+p addresses row q, elements 4p..4p+3 of a
// 4x16 block; lane i gets column i of the 4 rows (row q -> elem q)
__device__ __forceinline__ bf16x4 lds_read_tr16(const char* p) {
  const v4s r = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) v4s*)(p));
  return __builtin_bit_cast(bf16x4, r);
}

// SINGLE: the whole key range is one chunk (Skv <= 128): no running max / rescale.
template <bool SINGLE>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(4))) void attention_d32_kernel(
    const bf16* __restrict__ Q, int ldq, const bf16* __restrict__ Kp, int ldk, const bf16* __restrict__ V, int ldv,
    bf16* __restrict__ O, int ldo, const int32_t* __restrict__ lens, int Sq, int Skv, int H, int nq, int npairs,
    float scale_log2) {
  __shared__ __attribute__((aligned(16))) char lds[kLdsK + kLdsV];
  char* ldsK = lds;
  char* ldsV = lds + kLdsK;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int qblk = blockIdx.x % nq, pair = (blockIdx.x / nq) % npairs, b = blockIdx.x / (nq * npairs);
  const int len = lens ? min(lens[b], Skv) : Skv;
  const int fr = lane & 15, fg = lane >> 4;
  const int hsel = wave >> 2, h = pair * 2 + hsel;
  const bool has_odd = pair * 2 + 1 < H;
  const int qw = qblk * kQB + (wave & 3) * 32;  // this wave's 32 queries
  const bool active = h < H && qw < Sq;         // wave-uniform; idle waves still stage and meet the barriers

  const bf16* Kb = Kp + (size_t)b * Skv * ldk + pair * (2 * kD);
  const bf16* Vb = V + (size_t)b * Skv * ldv + pair * (2 * kD);

  // ---- Q fragments: 2 query tiles x 16 queries, the whole head row (d = fg*8 .. +7) ----
  bf16x8 qf[2];
#pragma unroll
  for (int qt = 0; qt < 2; ++qt) {
#pragma unroll
    for (int e = 0; e < 8; ++e) qf[qt][e] = (bf16)0.f;
    if (active) {
      const int q = min(qw + qt * 16 + fr, Sq - 1);
      qf[qt] = *reinterpret_cast<const bf16x8*>(Q + ((size_t)b * Sq + q) * ldq + h * kD + fg * 8);
    }
  }

  float m_run[2] = {-1e30f, -1e30f}, l_run[2] = {0.f, 0.f};
  f32x4 o[2][2];  // O^T tiles [query tile][d-tile]
#pragma unroll
  for (int qt = 0; qt < 2; ++qt)
#pragma unroll
    for (int dt = 0; dt < 2; ++dt) o[qt][dt] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int kc = 0; kc < len; kc += kKC) {
    __syncthreads();  // previous chunk fully consumed
    // ---- stage the pair's K and V chunks: 16 pieces of 8 rows each (2 per wave), row-major
    // 128-B images; LDS position spos of row r receives global chunk swz(r, spos) ----
    {
      const int srow = lane >> 3, spos = lane & 7;
#pragma unroll
      for (int i = 0; i < 16 / kWaves; ++i) {
        const int piece = i * kWaves + wave;
        const int r = piece * 8 + srow;
        const int key = min(kc + r, Skv - 1);
        int ck = kswz(r, spos), cv = vswz(r, spos);
        if (!has_odd) {  // one-head pair: never read the columns past H*32
          ck &= 3;
          cv &= 3;
        }
        // 32-bit lane offsets from the item's base (host check: Skv * ld < 2^31)
        glds16(Kb + (unsigned)key * (unsigned)ldk + ck * 8, ldsK + piece * 8 * kRowB);
        glds16(Vb + (unsigned)key * (unsigned)ldv + cv * 8, ldsV + piece * 8 * kRowB);
      }
    }
    wait_vmcnt0();
    __syncthreads();

    if (active) {
      const int klive = len - kc;  // > 0; keys of this chunk below klive are live
      // ---- S^T = K·Q^T: s[qt][kt] holds keys kt*16 + fg*4 + r, query qt*16 + fr ----
      f32x4 s[2][8];
#pragma unroll
      for (int kt = 0; kt < 8; ++kt) {
        s[0][kt] = f32x4{0.f, 0.f, 0.f, 0.f};
        s[1][kt] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (kt * 16 < klive) {
          const int r = kt * 16 + fr;
          const bf16x8 kf = *reinterpret_cast<const bf16x8*>(ldsK + r * kRowB + kswz(r, hsel * 4 + fg) * 16);
          s[0][kt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[0], s[0][kt], 0, 0, 0);
          s[1][kt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[1], s[1][kt], 0, 0, 0);
        }
      }

      // ---- scale, mask, softmax in the exp2 domain (per query column) ----
      const bool tail = klive < kKC;
#pragma unroll
      for (int qt = 0; qt < 2; ++qt) {
        float cmax = -1e30f;
#pragma unroll
        for (int kt = 0; kt < 8; ++kt)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            float x = s[qt][kt][r] * scale_log2;
            if (tail) x = kt * 16 + fg * 4 + r >= klive ? -1e30f : x;
            s[qt][kt][r] = x;
            cmax = fmaxf(cmax, x);
          }
        cmax = lane_rows_max(cmax);  // l, l^16, l^32, l^48 by permlane swaps
        const float m_new = SINGLE ? cmax : fmaxf(m_run[qt], cmax);
        float psum = 0.f;
#pragma unroll
        for (int kt = 0; kt < 8; ++kt)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float x = s[qt][kt][r];
            float p = __builtin_amdgcn_exp2f(x - m_new);
            if (tail) p = x <= -1e29f ? 0.f : p;
            s[qt][kt][r] = p;
            psum += p;
          }
        psum = lane_rows_sum(psum);
        if constexpr (SINGLE) {
          l_run[qt] = psum;
        } else {
          const float alpha = __builtin_amdgcn_exp2f(m_run[qt] - m_new);
          l_run[qt] = l_run[qt] * alpha + psum;
          m_run[qt] = m_new;
          o[qt][0] *= alpha;
          o[qt][1] *= alpha;
        }
      }

      // ---- O^T += V^T · P^T over the live 32-key steps ----
      const int tq = fr >> 2, tp = fr & 3;  // transposed-read lane roles
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        if (ks * 32 < klive) {
          bf16x8 pf[2];
#pragma unroll
          for (int qt = 0; qt < 2; ++qt)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              pf[qt][e] = f2bf(s[qt][2 * ks][e]);
              pf[qt][4 + e] = f2bf(s[qt][2 * ks + 1][e]);
            }
#pragma unroll
          for (int dt = 0; dt < 2; ++dt) {
            const int klo = ks * 32 + fg * 4 + tq, khi = klo + 16;
            const int c = hsel * 4 + dt * 2 + (tp >> 1);
            const bf16x4 lo = lds_read_tr16(ldsV + klo * kRowB + vswz(klo, c) * 16 + (tp & 1) * 8);
            const bf16x4 hi = lds_read_tr16(ldsV + khi * kRowB + vswz(khi, c) * 16 + (tp & 1) * 8);
            bf16x8 vf;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              vf[e] = lo[e];
              vf[4 + e] = hi[e];
            }
            o[0][dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf[0], o[0][dt], 0, 0, 0);
            o[1][dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf[1], o[1][dt], 0, 0, 0);
          }
        }
      }
    }
    if constexpr (SINGLE) break;
  }

  // ---- normalise into the K half of LDS: row = query of the block, the pair's 128-B row with
  // 16-B chunks at kswz positions; lane holds O[q][dt*16 + fg*4 + 0..3] ----
  __syncthreads();  // every wave is done with the last chunk
  if (active) {
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) {
      const float inv = l_run[qt] > 0.f ? 1.f / l_run[qt] : 0.f;
      const int row = (wave & 3) * 32 + qt * 16 + fr;
#pragma unroll
      for (int dt = 0; dt < 2; ++dt) {
        bf16x4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = f2bf(o[qt][dt][e] * inv);
        const int ch = hsel * 4 + dt * 2 + (fg >> 1);
        *reinterpret_cast<bf16x4*>(ldsK + row * kRowB + kswz(row, ch) * 16 + (fg & 1) * 8) = v;
      }
    }
  }
  __syncthreads();
  // ---- store whole pair rows: wave w owns rows w*16 .. +15, 8 rows x 128 B per instruction.
  // Rows >= Sq (never written above when their wave was idle) and the missing odd head's half
  // are not stored ----
  {
    const int lr = lane >> 3, lc = lane & 7;
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) {
      const int row = wave * 16 + hh * 8 + lr;
      const int q = qblk * kQB + row;
      if (q < Sq && (lc < 4 || has_odd)) {
        const u32x4 val = *reinterpret_cast<const u32x4*>(ldsK + row * kRowB + kswz(row, lc) * 16);
        *reinterpret_cast<u32x4*>(O + ((size_t)b * Sq + q) * ldo + pair * (2 * kD) + lc * 8) = val;
      }
    }
  }
}

}  // namespace

void attention_d32_fwd_strided(const bf16* q, int ldq, const bf16* k, int ldk, const bf16* v, int ldv, bf16* out,
                               int ldo, const int32_t* lens, int B, int Sq, int Skv, int H, float scale,
                               hipStream_t stream) {
  ATPU_CHECK(B > 0 && Sq > 0 && Skv > 0 && H > 0, "attention: empty problem");
  ATPU_CHECK(ldq % 8 == 0 && ldk % 8 == 0 && ldv % 8 == 0 && ldo % 8 == 0, "attention: head dim 32 needs 16-B row strides");
  ATPU_CHECK(((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(k) | reinterpret_cast<uintptr_t>(v) |
               reinterpret_cast<uintptr_t>(out)) & 15) == 0,
             "attention: head dim 32 needs 16-B aligned q, k, v, out");
  ATPU_CHECK(ldq >= H * kD && ldk >= H * kD && ldv >= H * kD && ldo >= H * kD, "attention: rows narrower than H*32");
  ATPU_CHECK((long long)Skv * std::max(ldk, ldv) < (1LL << 31), "attention: one item's K / V rows must span < 2^31 elements");
  const int nq = (Sq + kQB - 1) / kQB, npairs = (H + 1) / 2;
  const long long nb = (long long)nq * npairs * B;
  ATPU_CHECK(nb < (1LL << 31), "attention: grid too large");
  const float sl2 = scale * kLog2e;
  // (a) packed BERT layout (q | k | v column blocks of one [rows, 3*H*32] tensor), one key chunk;
  // (b) anything else: 128-key chunks with the online softmax
  const bool packed = k == q + H * kD && v == k + H * kD && ldk == ldq && ldv == ldq;
  if (packed && Sq == Skv && Skv <= kKC)
    hipLaunchKernelGGL(attention_d32_kernel<true>, dim3((unsigned)nb), dim3(kThreads), 0, stream, q, ldq, k, ldk, v,
                       ldv, out, ldo, lens, Sq, Skv, H, nq, npairs, sl2);
  else
    hipLaunchKernelGGL(attention_d32_kernel<false>, dim3((unsigned)nb), dim3(kThreads), 0, stream, q, ldq, k, ldk, v,
                       ldv, out, ldo, lens, Sq, Skv, H, nq, npairs, sl2);
  ATPU_HIP_CHECK(hipGetLastError());
}

}  // namespace atpu
