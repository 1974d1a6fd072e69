// regex_fuzz.cpp -- PatternMatch's regex compiler and table walker (deequ_amd/csrc/dq_regex.h,
// dq_regex.cpp) under the host sanitizers.  The compiler parses caller-supplied text, so this
// stand-alone program feeds it the patterns the tests use, seeded random byte strings, and random
// edits of the valid patterns (which reach far deeper into the parser than noise does), and walks
// seeded random byte strings -- valid UTF-8 or not -- through every table that compiles.  It also
// checks each image's invariants: every entry is a row offset inside the table, row 0 is absorbing.
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I deequ_amd/csrc tools/regex_fuzz.cpp deequ_amd/csrc/dq_regex.cpp -o /tmp/regex_fuzz
//   /tmp/regex_fuzz [iterations]
//
// Host code only: it is never loaded into Python and never runs on a GPU.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "dq_regex.h"

namespace {

struct Bytes {
  const uint8_t* p;
  uint32_t operator[](int64_t i) const { return p[i]; }
};

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint64_t rnd() {  // splitmix64
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

const char* kPatterns[] = {
    "foo", "a\\.b\\*c\\\\d", "x\\ty|u\\nv|p\\fq", "\\x41\xc3\xa9\\x7e", "a.c", "[abc]x[^a-c]z", "[a-f0-9]{4}-[^\\s-]",
    "\\d+\\.\\d+", "\\D\\d\\s\\S", "\\w+@\\W", "[\\d\\s]{3}[^\\w]", "[\\W\\d]q[+*?.$^(|){-]", "(ab)+c",
    "(?:ab|cd)e(f|g(h|i))", "cat|dog|bird", "ab?c", "ab*c", "ab+c", "a{3}b", "a{2,}b", "a{2,4}b",
    "a+?b|c*?d|e??f|g{2,3}?h", "^abc", "abc$", "^\\d+$", "^ab|cd$", "\xc3\xa9+x|\xe4\xbe\x8b\xe5\xad\x90",
    "[^\\s]\xe4\xbe\x8b|[\xc3\xa0-\xc3\xbf]{2}", "\\d{3}-\\d{2}-\\d{4}", "\\u00e9[\\u4e00-\\u9fff]+",
    "[0-9a-f]{8}-[0-9a-f]{4}-[0-9a-f]{4}-[0-9a-f]{4}-[0-9a-f]{12}",
    "^[0-9a-f]{8}-[0-9a-f]{4}-[0-9a-f]{4}-[0-9a-f]{4}-[0-9a-f]{12}$",
    "(https?|ftp)://[^\\s/$.?#].[^\\s]*",
    "(?:[a-z0-9!#$%&'*+/=?^_`{|}~-]+(?:\\.[a-z0-9!#$%&'*+/=?^_`{|}~-]+)*|\"(?:[\\x01-\\x08\\x0b\\x0c\\x0e-\\x1f\\x21"
    "\\x23-\\x5b\\x5d-\\x7f]|\\\\[\\x01-\\x09\\x0b\\x0c\\x0e-\\x7f])*\")@(?:(?:[a-z0-9](?:[a-z0-9-]*[a-z0-9])?\\.)+[a-z0-9]"
    "(?:[a-z0-9-]*[a-z0-9])?|\\[(?:(?:25[0-5]|2[0-4][0-9]|[01]?[0-9][0-9]?)\\.){3}(?:25[0-5]|2[0-4][0-9]|[01]?[0-9][0-9]?|"
    "[a-z0-9-]*[a-z0-9]:(?:[\\x01-\\x08\\x0b\\x0c\\x0e-\\x1f\\x21-\\x5a\\x53-\\x7f]|\\\\[\\x01-\\x09\\x0b\\x0c\\x0e-\\x7f])+)\\])",
    // declined ones
    "(a)\\1", "(?=a)b", "(?<!a)b", "\\bx", "a*+b", "(?>a)b", "(?i)a", "(?<name>a)", "\\p{L}", "\\hx", "[a-z&&[^b]]",
    "[a[b]]", "a*", "^$", "(|a)", "(a|b)*a(a|b){14}", "(a|b)*a(a|b){200}", "((((a{1000}){1000}){1000}){1000}){1000}",
    "((((((((((((((((((((((((((((((((((((((((((((((((((((((((((((((((((((((((((((((((((((((((((((((((((((((((((((((((((("
    "((((((((((((((((((((((((((((((((((((((((((((((((((((a",
    ".{1000}.{1000}.{1000}x", "[^\\x00-\\x{10FFFF}]", "\\", "[", "a{", "a{2,", "\\x4", "\\u00e", "(?", "a{99999999999999999999}",
};

const char kPieces[] = "\\()[]{}|?*+.^$-,0123456789abxdswDSWux\n\r\t :<=!>&pPkQE\x80\xbf\xc3\xa9\xe4\xf0\xff";

int checked = 0, accepted = 0;

void run(const std::string& pat) {
  dq::regex::Dfa dfa;
  std::string err;
  ++checked;
  if (!dq::regex::compile(reinterpret_cast<const uint8_t*>(pat.data()), (int32_t)pat.size(), &dfa, &err)) {
    if (err.empty()) {
      std::fprintf(stderr, "declined without a message\n");
      std::abort();
    }
    return;
  }
  ++accepted;
  const size_t entries = (size_t)dfa.n_states * dfa.n_cols;
  if (dfa.table.size() != entries || dfa.start_row >= entries || dfa.n_cols < 2) std::abort();
  for (size_t i = 0; i < entries; ++i)
    if (dfa.table[i] % dfa.n_cols != 0 || dfa.table[i] >= entries) std::abort();
  for (uint32_t c = 0; c < dfa.n_cols; ++c)
    if (dfa.table[c] != 0) std::abort();  // the accept row is absorbing
  for (int b = 0; b < 256; ++b)
    if (dfa.cmap[b] >= dfa.n_cols - 1) std::abort();
  const std::vector<uint8_t> img = dfa.image();
  if (img.size() % 16 != 0 || img.size() < dq::regex::kRegexHeaderBytes + 256 + 2 * entries) std::abort();
  if (dq::regex::regex_walk(dfa.cmap, dfa.table.data(), dfa.n_cols, dfa.start_row, Bytes{nullptr}, 0)) {
    std::fprintf(stderr, "an accepted pattern matched the empty string\n");
    std::abort();
  }
  for (int t = 0; t < 24; ++t) {
    // (exactly sized heap buffers: a read past the row is a sanitizer report)
    std::vector<uint8_t> text((size_t)(rnd() % 96));
    const bool ascii = (rnd() & 1) != 0;
    for (uint8_t& b : text) b = ascii ? (uint8_t)(rnd() % 96 + 32) : (uint8_t)rnd();
    if (!text.empty() && (rnd() & 3) == 0 && pat.size() <= text.size())  // sometimes a piece of the pattern itself
      for (size_t i = 0; i < pat.size(); ++i) text[i] = (uint8_t)pat[i];
    (void)dq::regex::regex_walk(dfa.cmap, dfa.table.data(), dfa.n_cols, dfa.start_row, Bytes{text.data()},
                                (int64_t)text.size());
  }
}

}  // namespace

int main(int argc, char** argv) {
  const long iterations = argc > 1 ? std::atol(argv[1]) : 20000;
  const size_t n_fixed = sizeof(kPatterns) / sizeof(kPatterns[0]);
  for (size_t i = 0; i < n_fixed; ++i) run(kPatterns[i]);
  for (long it = 0; it < iterations; ++it) {
    std::string pat;
    const uint64_t mode = rnd() % 3;
    if (mode == 0) {  // random bytes
      pat.resize((size_t)(rnd() % 40));
      for (char& c : pat) c = (char)rnd();
    } else if (mode == 1) {  // random regex-looking pieces
      const size_t n = (size_t)(rnd() % 24);
      for (size_t i = 0; i < n; ++i) pat.push_back(kPieces[rnd() % (sizeof(kPieces) - 1)]);
    } else {  // a valid pattern under a few edits
      pat = kPatterns[rnd() % n_fixed];
      const int edits = 1 + (int)(rnd() % 4);
      for (int e = 0; e < edits; ++e) {
        const size_t at = pat.empty() ? 0 : (size_t)(rnd() % pat.size());
        const char c = kPieces[rnd() % (sizeof(kPieces) - 1)];
        switch (rnd() % 4) {
          case 0: if (!pat.empty()) pat[at] = c; break;
          case 1: if (!pat.empty()) pat.erase(at, 1 + (size_t)(rnd() % 3)); break;
          case 2: pat.insert(at, 1, c); break;
          default: pat = pat.substr(0, at); break;
        }
      }
    }
    run(pat);
  }
  std::printf("regex_fuzz: %d patterns compiled or declined, %d accepted and walked: clean\n", checked, accepted);
  return 0;
}
