// schema_check.cpp -- RowLevelSchemaValidator's shared cell tests (deequ_amd/csrc/dq_schema.h: the
// source the evaluate kernel runs on the device) under the host sanitizers.  This stand-alone
// program reads vectors the Python restatement wrote (tools/schema_vectors.py: one line per cell,
// "kind precision scale result value hex-of-the-text") and checks parse_int32 / parse_decimal
// against them.  Every cell is copied into an allocation of exactly its length, so a read one byte
// outside the cell is an AddressSanitizer error.
//
//   python tools/schema_vectors.py /tmp/schema_vectors.txt
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I deequ_amd/csrc tools/schema_check.cpp -o /tmp/schema_check
//   /tmp/schema_check /tmp/schema_vectors.txt
//
// Host code only: it is never loaded into Python and never runs on a GPU.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "dq_schema.h"

namespace {

struct Text {
  const uint8_t* p;
  uint32_t operator[](int32_t i) const { return p[i]; }
};

int failures = 0;
#define CHECK(cond)                                                   \
  do {                                                                \
    if (!(cond)) {                                                    \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);   \
      ++failures;                                                     \
    }                                                                 \
  } while (0)

// (result, value) of one cell held in an allocation of exactly n bytes
void run_cell(int kind, const std::string& text, int precision, int scale, int32_t* result, int64_t* value) {
  const int32_t n = (int32_t)text.size();
  uint8_t* exact = n ? static_cast<uint8_t*>(std::malloc((size_t)n)) : nullptr;
  if (n) std::memcpy(exact, text.data(), (size_t)n);
  *value = 0;
  if (kind == 1) {
    int32_t v = 0;
    *result = dq::schema::parse_int32(Text{exact}, n, &v) ? 1 : 0;
    if (*result == 1) *value = v;
  } else {
    int64_t v = 0;
    *result = dq::schema::parse_decimal(Text{exact}, n, precision, scale, &v);
    if (*result == 1) *value = v;
  }
  std::free(exact);
}

int hex(char c) { return c <= '9' ? c - '0' : c - 'a' + 10; }

}  // namespace

int main(int argc, char** argv) {
  {  // by hand (RowLevelSchemaValidatorTest.scala:149-177 among them)
    int32_t r;
    int64_t v;
    run_cell(2, "299.000", 10, 2, &r, &v);
    CHECK(r == 1 && v == 29900);
    run_cell(2, "-99.99", 10, 2, &r, &v);
    CHECK(r == 1 && v == -9999);
    run_cell(2, "###", 10, 2, &r, &v);
    CHECK(r == 0);
    run_cell(2, "99.995", 4, 2, &r, &v);
    CHECK(r == 0);
    run_cell(2, "9.995", 4, 2, &r, &v);
    CHECK(r == 1 && v == 1000);
    run_cell(2, "1e5000", 4, 2, &r, &v);
    CHECK(r == 2);
    run_cell(2, "", 4, 2, &r, &v);
    CHECK(r == 0);
    run_cell(1, "-2147483648", 0, 0, &r, &v);
    CHECK(r == 1 && v == -2147483648ll);
    run_cell(1, "2147483648", 0, 0, &r, &v);
    CHECK(r == 0);
    run_cell(1, "", 0, 0, &r, &v);
    CHECK(r == 0);
    run_cell(1, ".", 0, 0, &r, &v);
    CHECK(r == 1 && v == 0);
  }
  long long n_cells = 0;
  if (argc > 1) {
    std::ifstream in(argv[1]);
    if (!in) {
      std::printf("schema_check: cannot read %s\n", argv[1]);
      return 2;
    }
    std::string line;
    while (std::getline(in, line)) {
      if (line.empty()) continue;
      std::istringstream ls(line);
      int kind, precision, scale, want_r;
      long long want_v;
      std::string hx;
      ls >> kind >> precision >> scale >> want_r >> want_v;
      if (!ls) {
        std::printf("schema_check: malformed line: %s\n", line.c_str());
        return 2;
      }
      ls >> hx;  // (absent for the empty cell)
      std::string text;
      for (size_t i = 0; i + 1 < hx.size(); i += 2) text.push_back((char)(hex(hx[i]) * 16 + hex(hx[i + 1])));
      int32_t r;
      int64_t v;
      run_cell(kind, text, precision, scale, &r, &v);
      if (r != want_r || v != want_v) {
        std::printf("FAILED cell %s (kind %d, %d, %d): got (%d, %lld), want (%d, %lld)\n", hx.c_str(), kind, precision,
                    scale, r, (long long)v, want_r, want_v);
        ++failures;
      }
      ++n_cells;
    }
  }
  if (failures) std::printf("schema_check: %d check(s) FAILED (%lld cells from the file)\n", failures, n_cells);
  else std::printf("schema_check: all checks passed (%lld cells from the file)\n", n_cells);
  return failures ? 1 : 0;
}
