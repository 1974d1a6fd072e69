// like_check.cpp -- the three matching modes of the regex compiler (deequ_amd/csrc/dq_regex.h,
// dq_regex.cpp: find-non-empty for PatternMatch, find for RLIKE, full for LIKE) under the host
// sanitizers.  It compiles the tests' pattern lists in every mode, checks each image's invariants
// (every entry a row offset inside the table, the accept row absorbing, the byte map inside the
// byte columns), checks a table of hand-written answers, and walks seeded random byte strings --
// valid UTF-8 or not, in exactly sized heap buffers -- through every table that compiles.  LIKE
// patterns are also made at random from `_`, `%`, literals and stray bytes.
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I deequ_amd/csrc tools/like_check.cpp deequ_amd/csrc/dq_regex.cpp -o /tmp/like_check
//   /tmp/like_check [iterations]
//
// Host code only: it is never loaded into Python and never runs on a GPU.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "dq_regex.h"

namespace {

using dq::regex::Dfa;
using dq::regex::Mode;

struct Bytes {
  const uint8_t* p;
  uint32_t operator[](int64_t i) const { return p[i]; }
};

uint64_t rng_state = 0x243F6A8885A308D3ull;
uint64_t rnd() {  // splitmix64
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

const char* kRegexes[] = {
    "foo", "a\\.b\\*c\\\\d", "a.c", "[abc]x[^a-c]z", "\\d+\\.\\d+", "\\w+@\\W", "(ab)+c", "cat|dog|bird", "ab?c", "a{2,4}b",
    "^abc", "abc$", "^\\d+$", "^ab|cd$", "\xc3\xa9+x|\xe4\xbe\x8b\xe5\xad\x90", "\\d{3}-\\d{2}-\\d{4}", "keyword",
    // nullable: declined in find-non-empty, answered in find
    "a*", "\\d*", "(|a)", "^$", "^\\d*$", "x*$", "a?", "(a|b*)", "x{0,3}", "", "^.*$", "^a*$",
    // declined in every mode
    "(a)\\1", "(?=a)b", "\\bx", "a*+b", "(?i)a", "\\p{L}", "[a-z&&[^b]]", "(a|b)*a(a|b){14}", "\\", "[", "a{2,",
};

const char* kLikes[] = {
    "", "%", "_", "%%", "a%", "%a", "%a%", "a_c", "a%b%c", "_%_", "abc", "CATEGORY%", "%keyword%", "%facets%",
    "\xe4\xbe\x8b%", "%\xf0\x9f\x98\x80", "\xc3\xa9_", "%ab%ab%", "%aab", "%a______", "%a______%b______%c_____",
    "______%\xc3\xa9______%", "%a_b_c_d_e_f_g%hijklmnop", "a.c", "a*", "(a|b)", "^a$",
    // declined
    "%a______________", "a\\%", "\\", "\xff", "%\xc3",
};

struct Known {
  int mode;
  const char* pattern;
  const char* text;
  bool want;
};
const Known kKnown[] = {
    {2, "", "", true}, {2, "", "a", false}, {2, "%", "", true}, {2, "%", "a\nb\r", true}, {2, "_", "\xc3\xa9", true},
    {2, "_", "\xe4\xbe\x8b", true}, {2, "_", "\xf0\x9f\x98\x80", true}, {2, "_", "ab", false}, {2, "_", "\n", true},
    {2, "a_c", "a\nc", true}, {2, "a_c", "a\rc", true}, {2, "abc", "abc\n", false}, {2, "a%", "a\n\n", true},
    {2, "%a", "a\n", false}, {2, "a%b%c", "aXbYc", true}, {2, "a%b%c", "abcb", false}, {2, "_%_", "a", false},
    {2, "_%_", "ab", true}, {2, "%aab", "aabaab", true}, {2, "%aab", "aaba", false}, {2, "a.c", "abc", false},
    {1, "a*", "xyz", true}, {1, "^$", "", true}, {1, "^$", "\n", true}, {1, "^$", "a", false}, {1, "^$", "\n\n", false},
    {1, "^\\d*$", "", true}, {1, "^\\d*$", "123", true}, {1, "^\\d*$", "123\n", true}, {1, "^\\d*$", "12a", false},
    {1, "x*$", "abc", true}, {1, "(|a)", "q", true}, {1, "", "abc", true}, {1, "foo", "xfoo", true}, {1, "foo", "fo", false},
    {1, "^.*$", "a\nb", false}, {1, "^.*$", "ab\n", true}, {1, "b$", "b\r\n", true}, {1, "b\\r$", "b\r\n", false},
    {0, "foo", "xfoox", true}, {0, "foo", "fo", false}, {0, "abc$", "abc\n", true},
};

int checked = 0, accepted = 0;

bool compile(int mode, const std::string& pat, Dfa* dfa, std::string* err) {
  const uint8_t* p = reinterpret_cast<const uint8_t*>(pat.data());
  if (mode == 2) return dq::regex::compile_like(p, (int32_t)pat.size(), dfa, err);
  return dq::regex::compile_mode(p, (int32_t)pat.size(), (Mode)mode, dfa, err);
}

void fail(const char* what, int mode, const std::string& pat) {
  std::fprintf(stderr, "like_check: %s (mode %d, pattern \"%s\")\n", what, mode, pat.c_str());
  std::abort();
}

void run(int mode, const std::string& pat) {
  Dfa dfa;
  std::string err;
  ++checked;
  if (!compile(mode, pat, &dfa, &err)) {
    if (err.empty()) fail("declined without a message", mode, pat);
    return;
  }
  ++accepted;
  const size_t entries = (size_t)dfa.n_states * dfa.n_cols;
  if (dfa.table.size() != entries || dfa.start_row >= entries || dfa.n_cols < 2) fail("table shape", mode, pat);
  if (entries * 2 > (size_t)dq::regex::kMaxTableBytes) fail("table over the LDS budget", mode, pat);
  for (size_t i = 0; i < entries; ++i)
    if (dfa.table[i] % dfa.n_cols != 0 || dfa.table[i] >= entries) fail("entry outside the table", mode, pat);
  for (uint32_t c = 0; c < dfa.n_cols; ++c)
    if (dfa.table[c] != 0) fail("the accept row is not absorbing", mode, pat);
  for (int b = 0; b < 256; ++b)
    if (dfa.cmap[b] >= dfa.n_cols - 1) fail("byte map outside the byte columns", mode, pat);
  const std::vector<uint8_t> img = dfa.image();
  if (img.size() % 16 != 0 || img.size() < dq::regex::kRegexHeaderBytes + 256 + 2 * entries) fail("image size", mode, pat);
  const bool empty = dq::regex::regex_walk(dfa.cmap, dfa.table.data(), dfa.n_cols, dfa.start_row, Bytes{nullptr}, 0);
  if (mode == 0 && empty) fail("find-non-empty matched the empty string", mode, pat);
  if (mode == 0) {  // compile() is that mode, image for image
    Dfa old;
    if (!dq::regex::compile(reinterpret_cast<const uint8_t*>(pat.data()), (int32_t)pat.size(), &old, &err) ||
        old.image() != img)
      fail("compile() and compile_mode(kFindNonEmpty) differ", mode, pat);
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
  for (const char* p : kRegexes)
    for (int mode = 0; mode < 2; ++mode) run(mode, p);
  for (const char* p : kLikes) run(2, p);
  for (const char* p : kRegexes) run(2, p);  // any text is a LIKE pattern (or holds a backslash)
  for (const Known& k : kKnown) {
    Dfa dfa;
    std::string err;
    if (!compile(k.mode, k.pattern, &dfa, &err)) fail(err.c_str(), k.mode, k.pattern);
    const std::vector<uint8_t> text(k.text, k.text + std::strlen(k.text));
    const bool got = dq::regex::regex_walk(dfa.cmap, dfa.table.data(), dfa.n_cols, dfa.start_row, Bytes{text.data()},
                                           (int64_t)text.size());
    if (got != k.want) fail((std::string("wrong answer on \"") + k.text + "\"").c_str(), k.mode, k.pattern);
  }
  static const char kLikePieces[] = "__%%%abcab01 .-\n\xc3\xa9\xe4\xbe\x8b\xf0\x9f\x98\x80\x80\xff\\";
  for (long it = 0; it < iterations; ++it) {
    std::string pat;
    const size_t n = (size_t)(rnd() % 28);
    for (size_t i = 0; i < n; ++i) pat.push_back(kLikePieces[rnd() % (sizeof(kLikePieces) - 1)]);
    run(2, pat);
    if ((it & 3) == 0) {  // a regex under a few edits, in both find modes
      std::string re = kRegexes[rnd() % (sizeof(kRegexes) / sizeof(kRegexes[0]))];
      const int edits = (int)(rnd() % 3);
      for (int e = 0; e < edits && !re.empty(); ++e) re[rnd() % re.size()] = "\\()[]{}|?*+.^$ab0"[rnd() % 18];
      run(0, re);
      run(1, re);
    }
  }
  std::printf("like_check: %d patterns compiled or declined over the three modes, %d accepted and walked, %zu known "
              "answers: clean\n", checked, accepted, sizeof(kKnown) / sizeof(kKnown[0]));
  return 0;
}
