// match_check.cpp -- the cross-table checks' NULL-safe cell equality (deequ_amd/csrc/dq_celleq.h:
// the source dq_freq_match_rows_kernel runs on the device) under the host sanitizers.  This
// stand-alone program builds the boundary cells tests/match_cases.py names -- NaNs of different
// payloads, +-0.0, +-Inf, integer and decimal128 extremes, strings of lengths 0, 1, 7, 8, 9, 15,
// 16, 17 and 64, equal up to the last byte, multi-byte, NULLs -- and checks cell_equal on every
// pair against a byte-by-byte restatement, in both argument orders.  Every buffer is an allocation
// of exactly its size, and a string column's value buffer ends with its last row, so a read outside
// a row, or of one aligned word around it, is an AddressSanitizer error.
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I deequ_amd/csrc tools/match_check.cpp -o /tmp/match_check
//   /tmp/match_check
//
// Host code only: it is never loaded into Python and never runs on a GPU.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "dq_celleq.h"

namespace {

using dq::celleq::Cells;

int failures = 0;
long checks = 0;
#define CHECK(cond)                                                   \
  do {                                                                \
    ++checks;                                                         \
    if (!(cond)) {                                                    \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);   \
      ++failures;                                                     \
    }                                                                 \
  } while (0)

// A column in exact-size allocations, sliced at `offset`: rows before it are valid and hold other
// values, so a read of the wrong element shows as a wrong verdict.
struct Column {
  std::vector<void*> owned;
  Cells cells{};
  int64_t rows = 0;
  ~Column() {
    for (void* p : owned) std::free(p);
  }
  void* exact(const void* src, size_t n) {
    if (n == 0) return nullptr;
    void* p = std::malloc(n);
    std::memcpy(p, src, n);
    owned.push_back(p);
    return p;
  }
  void validity(const std::vector<bool>& null, int64_t offset) {
    std::vector<uint8_t> bits((size_t)(offset + (int64_t)null.size() + 7) / 8, 0);
    for (int64_t r = 0; r < offset; ++r) bits[(size_t)r >> 3] |= (uint8_t)(1u << (r & 7));
    for (size_t r = 0; r < null.size(); ++r)
      if (!null[r]) bits[(size_t)(offset + (int64_t)r) >> 3] |= (uint8_t)(1u << ((offset + (int64_t)r) & 7));
    cells.validity = static_cast<const uint8_t*>(exact(bits.data(), bits.size()));
    cells.offset = offset;
    rows = (int64_t)null.size();
  }
};

// fixed-width cells: `width` bytes each; a NULL slot holds 0xA5 bytes
void fixed_column(Column& c, int32_t type, int width, const std::vector<std::vector<uint8_t>>& vals,
                  const std::vector<bool>& null, int64_t offset) {
  std::vector<uint8_t> buf((size_t)(offset + (int64_t)vals.size()) * (size_t)width, 0x5A);
  for (size_t r = 0; r < vals.size(); ++r) {
    uint8_t* at = buf.data() + ((size_t)offset + r) * (size_t)width;
    if (null[r]) std::memset(at, 0xA5, (size_t)width);
    else std::memcpy(at, vals[r].data(), (size_t)width);
  }
  c.cells.type = type;
  c.cells.values = c.exact(buf.data(), buf.size());
  c.validity(null, offset);
}

void bool_column(Column& c, const std::vector<int>& vals, const std::vector<bool>& null, int64_t offset) {
  std::vector<uint8_t> bits((size_t)(offset + (int64_t)vals.size() + 7) / 8, 0);
  for (size_t r = 0; r < vals.size(); ++r) {
    const int64_t at = offset + (int64_t)r;
    if (null[r] || vals[r]) bits[(size_t)at >> 3] |= (uint8_t)(1u << (at & 7));  // (a NULL slot holds a set bit)
  }
  c.cells.type = dq::celleq::T_BOOL;
  c.cells.values = c.exact(bits.data(), bits.size());
  c.validity(null, offset);
}

// strings: a NULL slot spans three bytes of its own; the heap ends with the last row
void string_column(Column& c, const std::vector<std::string>& vals, const std::vector<bool>& null, int64_t offset) {
  std::string heap;
  std::vector<int32_t> offs;
  for (int64_t r = 0; r < offset; ++r) {
    offs.push_back((int32_t)heap.size());
    heap += "before";
  }
  for (size_t r = 0; r < vals.size(); ++r) {
    offs.push_back((int32_t)heap.size());
    heap += null[r] ? std::string("\xff\xfe\xfd") : vals[r];
  }
  offs.push_back((int32_t)heap.size());
  c.cells.type = dq::celleq::T_UTF8;
  c.cells.values = c.exact(heap.data(), heap.size());
  c.cells.offsets = static_cast<const int32_t*>(c.exact(offs.data(), offs.size() * sizeof(int32_t)));
  c.validity(null, offset);
}

template <typename Same>
void all_pairs(const char* what, const Column& a, const Column& b, const std::vector<bool>& an, const std::vector<bool>& bn,
               Same same) {
  long equal = 0;
  for (int64_t i = 0; i < a.rows; ++i)
    for (int64_t j = 0; j < b.rows; ++j) {
      const bool want = (an[(size_t)i] || bn[(size_t)j]) ? (an[(size_t)i] && bn[(size_t)j]) : same((size_t)i, (size_t)j);
      const bool got = dq::celleq::cell_equal(a.cells, i, b.cells, j);
      const bool back = dq::celleq::cell_equal(b.cells, j, a.cells, i);
      if (got != want || back != want) std::printf("%s: row %lld against row %lld: want %d, got %d / %d\n", what, (long long)i, (long long)j, (int)want, (int)got, (int)back);
      CHECK(got == want);
      CHECK(back == want);
      equal += want;
    }
  CHECK(equal > 0 && equal < (long)(a.rows * b.rows));
}

template <typename T>
std::vector<uint8_t> bytes_of(T v) {
  std::vector<uint8_t> out(sizeof(T));
  std::memcpy(out.data(), &v, sizeof(T));
  return out;
}

template <typename T>
void int_cases(const char* what, int32_t type, T lo, T hi) {
  const std::vector<T> v = {lo, (T)(lo + 1), (T)-1, (T)0, (T)1, (T)(hi - 1), hi, (T)0};
  std::vector<std::vector<uint8_t>> raw;
  std::vector<bool> null(v.size(), false);
  null.back() = true;
  for (T x : v) raw.push_back(bytes_of(x));
  Column a, b;
  fixed_column(a, type, (int)sizeof(T), raw, null, 0);
  fixed_column(b, type, (int)sizeof(T), raw, null, 3);
  all_pairs(what, a, b, null, null, [&](size_t i, size_t j) { return v[i] == v[j]; });
}

template <typename F, typename U>
void float_cases(const char* what, int32_t type, const std::vector<U>& bits) {
  std::vector<std::vector<uint8_t>> raw;
  std::vector<F> v;
  for (U u : bits) {
    raw.push_back(bytes_of(u));
    F f;
    std::memcpy(&f, &u, sizeof(F));
    v.push_back(f);
  }
  raw.push_back(bytes_of((U)0));
  v.push_back((F)0);
  std::vector<bool> null(v.size(), false);
  null.back() = true;
  Column a, b;
  fixed_column(a, type, (int)sizeof(F), raw, null, 1);
  fixed_column(b, type, (int)sizeof(F), raw, null, 0);
  all_pairs(what, a, b, null, null, [&](size_t i, size_t j) {
    if (std::isnan(v[i]) || std::isnan(v[j])) return std::isnan(v[i]) && std::isnan(v[j]);
    return v[i] == v[j];
  });
}

void decimal_cases() {
  // the two little-endian words of 0, 1, -1, 10^38 - 1, -(10^38 - 1), 2^64, 2^64 + 1, -(2^64), 2^63
  const uint64_t w[][2] = {{0, 0}, {1, 0}, {~0ull, ~0ull}, {0x098a223fffffffffull, 0x4b3b4ca85a86c47aull},
                           {0xf675ddc000000001ull, 0xb4c4b357a5793b85ull}, {0, 1}, {1, 1}, {0, ~0ull},
                           {0x8000000000000000ull, 0}, {0, 0}};
  std::vector<std::vector<uint8_t>> raw;
  for (const auto& x : w) {
    std::vector<uint8_t> r(16);
    std::memcpy(r.data(), x, 16);
    raw.push_back(r);
  }
  std::vector<bool> null(raw.size(), false);
  null.back() = true;
  const int32_t type = dq::celleq::T_DECIMAL128 | (38 << 8);
  Column a, b;
  fixed_column(a, type, 16, raw, null, 0);
  fixed_column(b, type, 16, raw, null, 5);
  all_pairs("decimal128", a, b, null, null, [&](size_t i, size_t j) { return raw[i] == raw[j]; });
}

void bool_cases() {
  const std::vector<int> v = {1, 0, 1, 0};
  std::vector<bool> null = {false, false, true, true};
  for (int64_t offset : {0, 1, 7, 9}) {
    Column a, b;
    bool_column(a, v, null, offset);
    bool_column(b, v, null, 0);
    all_pairs("bool", a, b, null, null, [&](size_t i, size_t j) { return v[i] == v[j]; });
  }
}

void string_cases() {
  std::vector<std::string> v;
  for (int n : {0, 1, 7, 8, 9, 15, 16, 17, 64}) {
    std::string base;
    for (int i = 0; i < n; ++i) base += (char)('a' + i % 26);
    v.push_back(base);
    if (n) {
      std::string last = base, first = base;
      last[(size_t)n - 1] = '#';  // equal up to the last byte
      first[0] = '#';
      v.push_back(last);
      v.push_back(first);
    }
  }
  for (const char* s : {"\xc3\xa9", "e\xcc\x81", "\xe6\x97\xa5\xe6\x9c\xac\xe8\xaa\x9e", "\xe6\x97\xa5\xe6\x9c\xac\xe8\xaa\x9f"})
    v.push_back(s);
  v.push_back("null slot");
  std::vector<bool> null(v.size(), false);
  null.back() = true;
  for (int64_t offset : {0, 3}) {
    // the last row is rotated so that every string in turn ends the heap
    for (size_t last = 0; last + 1 < v.size(); last += 5) {
      std::vector<std::string> w = v;
      std::vector<bool> wn = null;
      std::swap(w[last], w[w.size() - 1]);
      { const bool t = wn[last]; wn[last] = wn[wn.size() - 1]; wn[wn.size() - 1] = t; }
      Column a, b;
      string_column(a, w, wn, offset);
      string_column(b, v, null, 0);
      all_pairs("string", a, b, wn, null, [&](size_t i, size_t j) { return w[i] == v[j]; });
    }
  }
}

}  // namespace

int main() {
  using namespace dq::celleq;
  int_cases<int8_t>("int8", T_INT8, INT8_MIN, INT8_MAX);
  int_cases<int16_t>("int16", T_INT16, INT16_MIN, INT16_MAX);
  int_cases<int32_t>("int32", T_INT32, INT32_MIN, INT32_MAX);
  int_cases<int64_t>("int64", T_INT64, INT64_MIN, INT64_MAX);
  float_cases<double, uint64_t>("float64", T_FLOAT64,
                                {0x0000000000000000ull, 0x8000000000000000ull, 0x3ff0000000000000ull, 0xbff0000000000000ull,
                                 0x7ff0000000000000ull, 0xfff0000000000000ull, 0x0000000000000001ull, 0x7fefffffffffffffull,
                                 0x7ff8000000000000ull, 0x7ff8000000000001ull, 0xfff8000000000000ull, 0x7ff0000000000001ull});
  float_cases<float, uint32_t>("float32", T_FLOAT32,
                               {0x00000000u, 0x80000000u, 0x3f800000u, 0xbf800000u, 0x7f800000u, 0xff800000u, 0x00000001u,
                                0x7f7fffffu, 0x7fc00000u, 0x7fc00001u, 0xffc00000u, 0x7f800001u});
  decimal_cases();
  bool_cases();
  string_cases();
  std::printf("match_check: %ld checks, %d failures\n", checks, failures);
  return failures ? 1 : 0;
}
