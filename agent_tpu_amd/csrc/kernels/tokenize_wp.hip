// Batched GPU WordPiece tokenizer (K1 for models with a vocabulary): packed UTF-8 rows -> ids.
//
// Spec ("atpu-wordpiece v1", Python twin: agent_tpu_amd/tokenizer.py WordPieceVocab, host twin:
// runtime/wordpiece.cpp; the matching rules and the table layout are shared code, atpu/wordpiece.h):
//   byte classes as in tokenize.hip (separators, one-byte punctuation words, word bytes);
//   each word is matched greedily, longest entry first, on bytes (ASCII A-Z folded when the
//   vocabulary is uncased); a continuation piece matches the "##" entries; a position that matches
//   nothing, or a word of more than 100 characters, makes the whole word one [UNK];
//   ids = [CLS] + first S-2 tokens + [SEP] + [PAD]...; len = n + 2.
//
// The frame is tokenize.hip's: one 64-wide wave per row, four rows per workgroup, the row staged
// into LDS by aligned 16-byte loads, 64 bytes classified per step, word starts against the left
// neighbour and word lengths from the ballot pair of two chunks (a walk for words of 64+ bytes).
// What differs is the work at a word start: the lane runs the greedy loop (one forward pass per
// piece, FNV grown a byte per candidate end, probing the open-addressed table in global memory --
// a 30,522-entry table is ~1.2 MB and stays in L2 -- and confirming a hash hit on the blob bytes).
// The first four piece ids of a word stay in registers; after the wave scan of piece counts they
// are written to their slots, and only a word of more than four pieces is matched a second time to
// write the rest. The scan stops as soon as S-2 tokens exist.
//
// Every load whose index depends on data is clamp-then-select: LDS reads past the row end read the
// row's last byte and are discarded, table slots are masked, blob offsets are clamped into the
// blob (wordpiece.h). No address relies on a lane being inactive to stay in range.
#include "atpu/common.h"
#include "atpu/kernels.h"
#include "atpu/wordpiece.h"

namespace atpu {
namespace {

constexpr int kMaxRowBytes = 4096;

__device__ __forceinline__ int wave_inclusive_scan(int v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(v, o, 64);
    if (lane >= o) v += t;
  }
  return v;
}

__global__ __launch_bounds__(256) void tokenize_wp_kernel(const uint8_t* __restrict__ text,
                                                          const int32_t* __restrict__ offsets,
                                                          int32_t* __restrict__ ids, int32_t* __restrict__ lens, int B,
                                                          int S, wp::Table tbl, int max_row_bytes,
                                                          long long text_bytes) {
  // the row starts up to 15 bytes into its first 16-B piece and ends inside its last one:
  // at most 4112 bytes are staged
  __shared__ __attribute__((aligned(16))) uint8_t rowbuf[4][kMaxRowBytes + 32];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int row = blockIdx.x * 4 + w;
  if (row >= B) return;
  // offsets are device data: clamp the row into the text buffer, so that no address below
  // depends on them being sane
  const long long tb = text_bytes;
  const long long start = min(max((long long)offsets[row], 0LL), tb);
  const int n = (int)min(max((long long)offsets[row + 1] - start, 0LL), min((long long)max_row_bytes, tb - start));
  const long long a0 = start & ~15LL;
  const int sh = (int)(start - a0);
  // the last whole aligned 16-B piece of the text buffer (-1: none); a piece beyond it is the
  // buffer's clipped tail and is read byte by byte
  const long long last16 = tb >= 16 ? ((tb - 16) & ~15LL) : -1;
  for (int c = lane; c < (n > 0 ? (sh + n + 15) >> 4 : 0); c += 64) {
    const long long g = a0 + 16 * c;  // < start + n <= tb
    if (g <= last16) {
      *reinterpret_cast<uint4*>(rowbuf[w] + 16 * c) = *reinterpret_cast<const uint4*>(text + g);
    } else {
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        const uint8_t b = text[min(g + k, tb - 1)];
        rowbuf[w][16 * c + k] = g + k < tb ? b : (uint8_t)0;
      }
    }
  }
  const uint8_t* buf = rowbuf[w] + sh;
  // each wave reads only its own LDS slice: a wave-level fence suffices
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

  const int cap = S - 2;
  const int nm1 = max(n - 1, 0);
  const int lower = tbl.lowercase;
  int32_t* out = ids + (size_t)row * S;
  int ntok = 0;
  int carry = 0;
  for (int base = 0; base < n && ntok < cap; base += 64) {
    const int i = base + lane;
    const uint32_t c1 = buf[min(i, nm1)], c2 = buf[min(i + 64, nm1)];
    const int cls = i < n ? wp::byte_class(c1) : 0;
    const int cls2 = i + 64 < n ? wp::byte_class(c2) : 0;
    const uint64_t W = __ballot(cls == 2), W2 = __ballot(cls2 == 2);
    int prev = __shfl_up(cls, 1, 64);
    if (lane == 0) prev = carry;
    const bool st = cls == 1 || (cls == 2 && prev != 2);
    // this lane's word: bytes [i, i + wlen) of the row
    auto by = [buf, i, nm1, lower](int k) -> uint32_t { return wp::fold(buf[min(i + k, nm1)], lower); };
    int wlen = 0, np = 0;
    int p0 = 0, p1 = 0, p2 = 0, p3 = 0;  // the word's first four piece ids
    bool unk = false;
    if (st) {
      wlen = 1;
      if (cls == 2) {
        // word bytes from i on: bits lane..63 of W, then W2
        const uint64_t x = lane == 0 ? W : ((W >> lane) | (W2 << (64 - lane)));
        if (~x != 0) {
          wlen = __builtin_ctzll(~x);
        } else {  // 64+ word bytes: walk the rest
          int j = i + 64;
          while (j < n && wp::byte_class(buf[min(j, nm1)]) == 2) ++j;
          wlen = j - i;
        }
      }
      int chars = wlen;
      if (wlen > wp::kMaxWordChars) {
        chars = 0;
        for (int k = 0; k < wlen; ++k) chars += (buf[min(i + k, nm1)] & 0xC0) != 0x80;
      }
      bool ok = chars <= wp::kMaxWordChars;
      if (ok)
        ok = wp::match_word(tbl, by, wlen, [&](int p, int id) {
          p0 = p == 0 ? id : p0;
          p1 = p == 1 ? id : p1;
          p2 = p == 2 ? id : p2;
          p3 = p == 3 ? id : p3;
          np = p + 1;
        });
      if (!ok) {
        unk = true;
        np = 1;
        p0 = tbl.unk;
      }
    }
    const int incl = wave_inclusive_scan(np, lane);
    const int slot0 = ntok + incl - np;  // this word's first token slot
    if (st && slot0 < cap) {
      if (slot0 + 0 < cap && np > 0) out[1 + slot0] = p0;
      if (slot0 + 1 < cap && np > 1) out[2 + slot0] = p1;
      if (slot0 + 2 < cap && np > 2) out[3 + slot0] = p2;
      if (slot0 + 3 < cap && np > 3) out[4 + slot0] = p3;
      if (np > 4 && slot0 + 4 < cap && !unk)
        wp::match_word(tbl, by, wlen, [&](int p, int id) {
          if (p >= 4 && slot0 + p < cap) out[1 + slot0 + p] = id;
        });
    }
    ntok += __shfl(incl, 63, 64);
    carry = __shfl(cls, 63, 64);
  }
  ntok = min(ntok, cap);
  if (lane == 0) {
    out[0] = tbl.cls;
    out[1 + ntok] = tbl.sep;
    lens[row] = ntok + 2;
  }
  for (int j = ntok + 2 + lane; j < S; j += 64) out[j] = tbl.pad;
}

}  // namespace

void tokenize_wordpiece(const uint8_t* text, const int32_t* offsets, int32_t* ids, int32_t* lens, int B, int S,
                        const uint8_t* table, const int32_t* header, size_t table_bytes, int max_row_bytes,
                        hipStream_t stream, long long text_bytes) {
  ATPU_CHECK((reinterpret_cast<uintptr_t>(text) & 15) == 0, "tokenize_wordpiece: text buffer must be 16-byte aligned");
  ATPU_CHECK(table != nullptr && (reinterpret_cast<uintptr_t>(table) & 15) == 0,
             "tokenize_wordpiece: table must be a 16-byte aligned device buffer");
  ATPU_CHECK(S >= 2, "tokenize_wordpiece: S must be >= 2");
  ATPU_CHECK(max_row_bytes > 0 && max_row_bytes <= kMaxRowBytes,
             "tokenize_wordpiece: max_row_bytes must be in (0, 4096]");
  ATPU_CHECK(text_bytes >= 0, "tokenize_wordpiece: text_bytes must be >= 0");
  wp::Table t;
  ATPU_CHECK(wp::parse_header(header, table_bytes, table, &t), "tokenize_wordpiece: bad table header");
  if (B <= 0) return;
  hipLaunchKernelGGL(tokenize_wp_kernel, dim3((B + 3) / 4), dim3(256), 0, stream, text, offsets, ids, lens, B, S, t,
                     max_row_bytes, text_bytes);
  ATPU_HIP_CHECK(hipGetLastError());
}

}  // namespace atpu
