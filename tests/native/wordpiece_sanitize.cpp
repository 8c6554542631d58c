// Sanitizer harness of the host WordPiece tokenizer (runtime/wordpiece.cpp only): builds a
// packed table and tokenizes adversarial rows from exactly-sized heap buffers, built with
// -fsanitize=address,undefined on the host side. Any memory error aborts with a sanitizer
// report; exit 0 and "clean" mean clean.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <stdexcept>
#include <string>
#include <vector>

#include "atpu/runtime.h"

namespace {

std::vector<std::string> make_vocab() {
  std::vector<std::string> v = {"[PAD]", "[unused0]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"};
  for (char c = 'a'; c <= 'y'; ++c) {  // no z: [UNK]
    v.push_back(std::string(1, c));
    v.push_back("##" + std::string(1, c));
  }
  for (const char* p : {"ka", "lo", "##ka", "##lo", "kalo", "##kalokalokalokalokalokalokalokalo", ",", ".", "#", "##", "###",
                        "\xc3\xa9", "##\xc3\xa9", "ka", ""})
    v.push_back(p);
  return v;
}

// Rows packed into a heap buffer of exactly their total size, so a read past a row's end
// that leaves the text is a heap-buffer-overflow.
void run(const std::vector<uint8_t>& table, const std::vector<std::string>& rows, int S, int max_row_bytes) {
  std::vector<int32_t> offs(rows.size() + 1, 0);
  for (size_t r = 0; r < rows.size(); ++r) offs[r + 1] = offs[r] + static_cast<int32_t>(rows[r].size());
  std::vector<uint8_t> text;
  text.reserve(offs.back());
  for (const std::string& r : rows) text.insert(text.end(), r.begin(), r.end());
  text.shrink_to_fit();
  const int B = static_cast<int>(rows.size());
  std::vector<int32_t> ids(static_cast<size_t>(B) * S, -1), lens(B, -1);
  atpu::wordpiece_host(text.data(), offs.data(), ids.data(), lens.data(), B, S, table.data(), table.size(),
                       max_row_bytes);
  for (int r = 0; r < B; ++r) {
    if (lens[r] < 2 || lens[r] > S || ids[static_cast<size_t>(r) * S] != 3 || ids[static_cast<size_t>(r) * S + lens[r] - 1] != 4)
      std::abort();
    for (int k = 0; k < S; ++k)
      if (ids[static_cast<size_t>(r) * S + k] < 0) std::abort();
  }
}

}  // namespace

int main() {
  const std::vector<uint8_t> table = atpu::wordpiece_build_table(make_vocab(), true);
  std::mt19937 rng(1234);
  const int max_row = 2048;
  for (int S : {2, 8, 128}) {
    run(table, {}, S, max_row);
    run(table, {"", "", ""}, S, max_row);
    run(table, {std::string(max_row, 'k'), "", std::string(max_row + 500, 'a'), std::string(max_row, '\xa9')}, S, max_row);
    // a word that ends exactly at the end of the buffer (and one cut there by max_row_bytes)
    run(table, {"lo ka, kalokalo"}, S, max_row);
    run(table, {std::string(max_row - 4, ' ') + "kalokalo"}, S, max_row);
    run(table, {"kaloz", "z", "KALO.#", std::string(99, 'a'), std::string(100, 'a'), std::string(101, 'a'),
                "kalokalokalokalokalokalokalokalokalo", "\xc3\xa9\xc3\xa9 caf\xc3\xa9"},
        S, max_row);
    for (int it = 0; it < 200; ++it) {
      std::vector<std::string> rows(1 + rng() % 5);
      for (std::string& r : rows) {
        r.resize(rng() % 3000);
        const bool wordy = rng() % 2;
        for (char& c : r) c = wordy ? "kalo ,z\xc3\xa9#K"[rng() % 12] : static_cast<char>(rng() & 0xff);
      }
      run(table, rows, S, 1 + static_cast<int>(rng() % 4096));
    }
  }
  // refused inputs raise, they do not read
  int refused = 0;
  try {
    atpu::wordpiece_build_table({"[PAD]", "[UNK]", "[CLS]"}, true);
  } catch (const std::invalid_argument&) {
    ++refused;
  }
  try {
    std::vector<uint8_t> cut(table.begin(), table.end() - 16);
    int32_t offs[2] = {0, 0}, ids[8], lens[1];
    atpu::wordpiece_host(nullptr, offs, ids, lens, 1, 8, cut.data(), cut.size(), max_row);
  } catch (const std::invalid_argument&) {
    ++refused;
  }
  if (refused != 2) std::abort();
  std::puts("wordpiece host twin: clean");
  return 0;
}
