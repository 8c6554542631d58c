// Host twin of the WordPiece vocabulary tokenizer ("atpu-wordpiece v1") and the builder of the
// packed table both twins read (atpu/wordpiece.h). Its own translation unit: no dependency on
// the rest of the host runtime.
#include <algorithm>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "atpu/runtime.h"
#include "atpu/wordpiece.h"

namespace atpu {

namespace {

uint32_t fnv(uint32_t h, const uint8_t* p, size_t n) {
  for (size_t i = 0; i < n; ++i) h = wp::fnv_step(h, p[i]);
  return h;
}

void put32(std::vector<uint8_t>& t, size_t at, uint32_t v) { std::memcpy(t.data() + at, &v, 4); }

}  // namespace

std::vector<uint8_t> wordpiece_build_table(const std::vector<std::string>& entries, bool lowercase) {
  if (entries.empty()) throw std::invalid_argument("wordpiece: empty vocabulary");
  struct E {
    uint32_t hash, id, off, lenkind;
  };
  // id of a special: the last line that holds it (as every other duplicate)
  int32_t special[4] = {-1, -1, -1, -1};
  static const char* const kNames[4] = {"[PAD]", "[UNK]", "[CLS]", "[SEP]"};
  std::vector<E> es;
  es.reserve(entries.size());
  std::vector<uint8_t> blob;
  int max_len = 1;
  for (size_t i = 0; i < entries.size(); ++i) {
    const std::string& e = entries[i];
    for (int k = 0; k < 4; ++k)
      if (e == kNames[k]) special[k] = static_cast<int32_t>(i);
    const bool cont = e.size() > 2 && e[0] == '#' && e[1] == '#';
    const uint8_t* p = reinterpret_cast<const uint8_t*>(e.data()) + (cont ? 2 : 0);
    const size_t n = e.size() - (cont ? 2 : 0);
    if (n == 0 || n > static_cast<size_t>(wp::kMaxEntryBytes)) continue;  // can never match
    const uint32_t h = fnv(cont ? wp::cont_basis() : wp::kBasis, p, n);
    es.push_back({h, static_cast<uint32_t>(i), static_cast<uint32_t>(blob.size()),
                  static_cast<uint32_t>(n) | (cont ? wp::kContBit : 0u)});
    blob.insert(blob.end(), p, p + n);
    max_len = std::max(max_len, static_cast<int>(n));
  }
  for (int k = 0; k < 4; ++k)
    if (special[k] < 0) throw std::invalid_argument(std::string("wordpiece: vocabulary has no ") + kNames[k]);
  blob.resize((blob.size() + wp::kBlobPad + 15) / 16 * 16, 0);
  if (blob.size() > 0x7fffffffu) throw std::invalid_argument("wordpiece: vocabulary too large");
  size_t slots = 16;
  while (slots < 2 * es.size()) slots *= 2;
  std::vector<uint8_t> t(wp::kHeaderBytes + 16 * slots + blob.size(), 0);
  const uint32_t mask = static_cast<uint32_t>(slots - 1);
  auto slot = [&](uint32_t i) { return reinterpret_cast<wp::Slot*>(t.data() + wp::kHeaderBytes) + i; };
  size_t stored = 0;
  for (const E& e : es) {
    const uint32_t len = e.lenkind & 0xffffu;
    uint32_t i = e.hash & mask;
    for (;; i = (i + 1) & mask) {
      wp::Slot* s = slot(i);
      if (s->lenkind == 0) {
        *s = {e.hash, e.id, e.off, e.lenkind};
        ++stored;
        break;
      }
      // the same entry again: the last occurrence wins
      if (s->hash == e.hash && s->lenkind == e.lenkind && std::memcmp(blob.data() + s->off, blob.data() + e.off, len) == 0) {
        s->id = e.id;
        break;
      }
    }
  }
  put32(t, 0, wp::kMagic);
  put32(t, 4, static_cast<uint32_t>(slots));
  put32(t, 8, static_cast<uint32_t>(max_len));
  put32(t, 12, static_cast<uint32_t>(blob.size()));
  for (int k = 0; k < 4; ++k) put32(t, 16 + 4 * k, static_cast<uint32_t>(special[k]));
  put32(t, 32, lowercase ? 1u : 0u);
  put32(t, 36, static_cast<uint32_t>(stored));
  std::memcpy(t.data() + wp::kHeaderBytes + 16 * slots, blob.data(), blob.size());
  return t;
}

void wordpiece_host(const uint8_t* text, const int32_t* offsets, int32_t* ids, int32_t* lens, int B, int S,
                    const uint8_t* table, size_t table_bytes, int max_row_bytes) {
  wp::Table t;
  int32_t hdr[wp::kHeaderWords];
  if (table_bytes < sizeof(hdr) || (reinterpret_cast<uintptr_t>(table) & 3) != 0)
    throw std::invalid_argument("wordpiece_host: bad table (64+ bytes, 4-byte aligned)");
  std::memcpy(hdr, table, sizeof(hdr));
  if (!wp::parse_header(hdr, table_bytes, table, &t)) throw std::invalid_argument("wordpiece_host: bad table");
  if (S < 2 || max_row_bytes <= 0 || max_row_bytes > wp::kMaxEntryBytes)
    throw std::invalid_argument("wordpiece_host: bad S/max_row_bytes");
  const int cap = S - 2;
  std::vector<int32_t> pieces;
  for (int r = 0; r < B; ++r) {
    const uint8_t* p = text + offsets[r];
    const int n = std::min(offsets[r + 1] - offsets[r], max_row_bytes);
    int32_t* out = ids + static_cast<size_t>(r) * S;
    int nt = 0;
    for (int i = 0; i < n && nt < cap;) {
      const int c = wp::byte_class(p[i]);
      if (c == 0) {
        ++i;
        continue;
      }
      int j = i + 1;
      if (c == 2)
        while (j < n && wp::byte_class(p[j]) == 2) ++j;
      int chars = 0;
      for (int k = i; k < j; ++k) chars += (p[k] & 0xC0) != 0x80;
      pieces.clear();
      const uint8_t* w = p + i;
      const int lower = t.lowercase;
      auto by = [w, lower](int k) { return wp::fold(w[k], lower); };
      const bool ok = chars <= wp::kMaxWordChars &&
                      wp::match_word(t, by, j - i, [&](int, int id) { pieces.push_back(id); });
      if (!ok) pieces.assign(1, t.unk);
      for (size_t k = 0; k < pieces.size() && nt < cap; ++k) out[1 + nt++] = pieces[k];
      i = j;
    }
    out[0] = t.cls;
    out[1 + nt] = t.sep;
    for (int k = nt + 2; k < S; ++k) out[k] = t.pad;
    lens[r] = nt + 2;
  }
}

}  // namespace atpu
