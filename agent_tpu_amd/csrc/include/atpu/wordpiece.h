// "atpu-wordpiece v1": greedy longest-match WordPiece over a real vocabulary, shared by the
// host twin (runtime/wordpiece.cpp) and the HIP kernel (kernels/tokenize_wp.hip), so the two
// cannot disagree on the table layout or the matching rules. Spec and pure-Python twin:
// agent_tpu_amd/tokenizer.py (WordPieceVocab).
//
// Packed table (one allocation, little endian):
//   bytes [0, 64)                 header, 16 int32: magic, slots, longest entry (bytes), blob
//                                 bytes, [PAD], [UNK], [CLS], [SEP], lowercase, entries
//   bytes [64, 64 + 16 * slots)   open-addressed slots {hash32, id, blob offset, len | kind << 16},
//                                 a power-of-two number at load <= 0.5; len == 0: empty slot
//   then the blob                 every entry's bytes with the "##" stripped, then >= 32 zero bytes
// hash32 is FNV-1a-32 of the entry; kind 1 (a "##" continuation piece) hashes from the FNV state
// after "##", kind 0 (a first piece) from the offset basis. A hit is confirmed on kind, length and
// bytes, so no result depends on hashes not colliding.
#pragma once

#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define ATPU_WP_HD __host__ __device__ __forceinline__
#else
#define ATPU_WP_HD inline
#endif

namespace atpu {
namespace wp {

constexpr uint32_t kMagic = 0x31505741u;  // "AWP1"
constexpr int kHeaderWords = 16, kHeaderBytes = 64;
constexpr int kMaxEntryBytes = 4096;  // rows are cut at <= 4096 bytes: a longer entry cannot match
constexpr int kMaxWordChars = 100;
constexpr int kBlobPad = 32;
constexpr uint32_t kContBit = 1u << 16;
constexpr uint32_t kBasis = 2166136261u, kPrime = 16777619u;

struct Slot {
  uint32_t hash, id, off, lenkind;
};

// The header's fields plus the two base pointers (host or device memory).
struct Table {
  const Slot* slots;
  const uint8_t* blob;
  uint32_t mask;        // slots - 1
  uint32_t blob_bytes;  // with the zero padding
  int32_t max_len;      // longest entry in bytes, "##" stripped
  int32_t pad, unk, cls, sep;
  int32_t lowercase;
};

// Reads and checks a header against the size of the allocation it heads; the pointers of ``t``
// are set relative to ``base`` (which may be a device address: it is not dereferenced here).
inline bool parse_header(const int32_t* hdr, size_t table_bytes, const uint8_t* base, Table* t) {
  if (table_bytes < static_cast<size_t>(kHeaderBytes) || static_cast<uint32_t>(hdr[0]) != kMagic) return false;
  const int64_t slots = hdr[1], max_len = hdr[2], blob = hdr[3];
  if (slots < 2 || (slots & (slots - 1)) != 0 || blob < kBlobPad) return false;
  if (max_len < 1 || max_len > kMaxEntryBytes || max_len > blob - kBlobPad) return false;
  if (static_cast<int64_t>(table_bytes) != kHeaderBytes + 16 * slots + blob) return false;
  if (hdr[9] < 0 || 2 * static_cast<int64_t>(hdr[9]) > slots) return false;  // load <= 0.5
  t->slots = reinterpret_cast<const Slot*>(base + kHeaderBytes);
  t->blob = base + kHeaderBytes + 16 * slots;
  t->mask = static_cast<uint32_t>(slots - 1);
  t->blob_bytes = static_cast<uint32_t>(blob);
  t->max_len = static_cast<int32_t>(max_len);
  t->pad = hdr[4], t->unk = hdr[5], t->cls = hdr[6], t->sep = hdr[7];
  t->lowercase = hdr[8] != 0;
  return true;
}

ATPU_WP_HD int byte_class(uint32_t c) {
  if (c == 0x20 || (c >= 0x09 && c <= 0x0D) || c < 0x20 || c == 0x7F) return 0;
  if ((c >= 0x21 && c <= 0x2F) || (c >= 0x3A && c <= 0x40) || (c >= 0x5B && c <= 0x60) || (c >= 0x7B && c <= 0x7E))
    return 1;
  return 2;
}

ATPU_WP_HD uint32_t fold(uint32_t c, int lowercase) { return (lowercase && c >= 'A' && c <= 'Z') ? c + 32 : c; }

ATPU_WP_HD uint32_t fnv_step(uint32_t h, uint32_t c) { return (h ^ c) * kPrime; }

ATPU_WP_HD uint32_t cont_basis() { return fnv_step(fnv_step(kBasis, '#'), '#'); }

// Id of the entry (kind, bytes [s, s+len) of the word) or -1. ``by(j)`` is byte j of the word,
// folded. Every load is clamp-then-select: the slot index is masked, the blob offset is clamped
// so that [off, off+len) lies in the blob whatever the slot holds, and the compare reads all
// ``len`` bytes without an early exit. The probe count is bounded by the table size, so a
// damaged table cannot hang the caller.
template <typename Bytes>
ATPU_WP_HD int lookup(const Table& t, uint32_t h, uint32_t lenkind, const Bytes& by, int s, int len) {
  uint32_t idx = h & t.mask;
  for (uint32_t it = 0; it <= t.mask; ++it) {
    const Slot sl = t.slots[idx];
    if (sl.lenkind == 0) return -1;
    if (sl.hash == h && sl.lenkind == lenkind) {
      const uint32_t lim = t.blob_bytes - static_cast<uint32_t>(len);
      const uint32_t off = sl.off < lim ? sl.off : lim;
      uint32_t diff = 0;
      for (int k = 0; k < len; ++k) diff |= static_cast<uint32_t>(t.blob[off + k]) ^ by(s + k);
      if (diff == 0) return static_cast<int>(sl.id);
    }
    idx = (idx + 1) & t.mask;
  }
  return -1;
}

// Greedy longest-match of one word of ``wlen`` bytes: emit(p, id) for piece p = 0, 1, ...; false
// as soon as some position matches nothing (the whole word is then one [UNK], whatever was
// emitted). One forward pass per piece: the hash grows by one byte per candidate end and the
// last confirmed hit wins.
template <typename Bytes, typename Emit>
ATPU_WP_HD bool match_word(const Table& t, const Bytes& by, int wlen, Emit&& emit) {
  const uint32_t cont = cont_basis();
  int p = 0;
  for (int s = 0; s < wlen;) {
    uint32_t h = s == 0 ? kBasis : cont;
    const uint32_t kind = s == 0 ? 0u : kContBit;
    const int emax = wlen < s + t.max_len ? wlen : s + t.max_len;
    int best_e = 0, best_id = 0;
    for (int e = s + 1; e <= emax; ++e) {
      h = fnv_step(h, by(e - 1));
      const int id = lookup(t, h, kind | static_cast<uint32_t>(e - s), by, s, e - s);
      best_e = id >= 0 ? e : best_e;
      best_id = id >= 0 ? id : best_id;
    }
    if (best_e == 0) return false;
    emit(p++, best_id);
    s = best_e;
  }
  return true;
}

}  // namespace wp
}  // namespace atpu
