// dq_regex.h -- PatternMatch's regex engine (PatternMatch.scala:37-55): a java.util.regex pattern
// compiled on the host (dq_regex.cpp) into a byte-level search DFA over UTF-8, and the table
// walker the host (dq_diag_regex_match, tests) and the gfx950 kernel (dq_regex.hip) share.
//
// The DFA answers "does Matcher.find() succeed with a non-empty group 0" for the subset of the
// syntax whose answer a regular language decides: no back-references, look-around, possessive or
// atomic constructs, and no pattern that can match the empty string (PatternMatch).
// Everything else is declined at compile time, never approximated.
//
// Image of one compiled pattern (what travels to the device; all little-endian):
//   uint32 n_states, n_cols, start_row, n_entries      (kRegexHeaderBytes)
//   uint8  cmap[256]                                   byte -> column
//   uint16 table[n_states * n_cols]                    row offsets: next = table[row + column]
// A state is named by its row offset (state * n_cols), so a step is two loads and one add.  Row 0
// is the accept state and is absorbing; column n_cols - 1 is "end of input" (taken once after the
// last byte: `$` and nothing else makes it lead to row 0).  Internal, not ABI.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#ifndef DQ_HD
#define DQ_HD __host__ __device__
#endif
#else
#ifndef DQ_HD
#define DQ_HD
#endif
#endif

namespace dq {
namespace regex {

constexpr int kMaxStates = 2048;             // subset construction stops here (DQ_ERR_UNSUPPORTED)
constexpr int kMaxTableBytes = 48 * 1024;    // the kernel's LDS budget for one transition table
constexpr int kMaxNfaNodes = 1 << 15;        // Thompson nodes (counted repetitions are unrolled)
constexpr int kMaxSubsetNodes = 1 << 20;     // NFA nodes summed over all DFA subsets (4 MiB of ints)
constexpr int kMaxRepeat = 1000;             // largest bound of {n,m}
constexpr int kMaxDepth = 128;               // nested groups
constexpr int kMaxPatternBytes = 1 << 16;
constexpr uint32_t kRegexHeaderBytes = 16;
constexpr uint32_t kRegexAccept = 0;         // row offset of the accept state

DQ_HD inline uint32_t regex_step(const uint8_t* cmap, const uint16_t* table, uint32_t row, uint32_t byte) {
  return table[row + cmap[byte]];
}
// After the last byte: the end-of-input column.  True = the row matched.
DQ_HD inline bool regex_finish(const uint16_t* table, uint32_t n_cols, uint32_t row) {
  return table[row + n_cols - 1u] == kRegexAccept;
}
// One row's bytes text[0 .. n): never reads outside them, whatever they hold.
template <typename Src>
DQ_HD inline bool regex_walk(const uint8_t* cmap, const uint16_t* table, uint32_t n_cols, uint32_t start_row,
                             const Src& text, int64_t n) {
  uint32_t row = start_row;
  for (int64_t i = 0; i < n && row != kRegexAccept; ++i) row = regex_step(cmap, table, row, text[i]);
  return regex_finish(table, n_cols, row);
}

}  // namespace regex
}  // namespace dq

#include <string>
#include <vector>

namespace dq {
namespace regex {

struct Dfa {
  uint32_t n_states = 0, n_cols = 0, start_row = 0;
  uint8_t cmap[256] = {};
  std::vector<uint16_t> table;
  // the image above, padded to a multiple of 16 bytes
  std::vector<uint8_t> image() const;
};

// What a compiled image answers about one row's bytes.  The image format and the walker are the
// same for all three; only the construction differs.
enum Mode : int32_t {
  kFindNonEmpty = 0,  // Matcher.find() with a non-empty group 0 (PatternMatch, RowLevelSchemaValidator)
  kFind = 1,          // Matcher.find(0): any match, an empty one included (RLIKE)
  kFull = 2           // the whole value matches a LIKE pattern (compile_like only)
};

// Compiles pattern[0 .. len) (UTF-8 text of a Java regex).  False = not in the supported subset
// (or over a construction bound): *err names the construct and its byte offset.
bool compile(const uint8_t* pattern, int32_t len, Dfa* out, std::string* err);
// ... in kFindNonEmpty (what compile() is) or kFind: the unanchored search without the "can match
// the empty string" decline; a pattern whose unanchored (or ^-anchored) part is nullable matches
// every row, and its image starts in the accept row.
bool compile_mode(const uint8_t* pattern, int32_t len, Mode mode, Dfa* out, std::string* err);
// Compiles the SQL LIKE pattern[0 .. len) (UTF-8; `_` one code point, `%` any sequence of code
// points, line terminators included; everything else itself) anchored at both ends.  A backslash
// is declined (LIKE escapes are not evaluated here), as is a pattern over a construction bound.
bool compile_like(const uint8_t* pattern, int32_t len, Dfa* out, std::string* err);

}  // namespace regex
}  // namespace dq
