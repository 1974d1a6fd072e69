// decimal_check.cpp -- the decimal arithmetic shared by the decimal scan, dq_cast_decimal and
// dq_plan_finish (deequ_amd/csrc/dq_decimal.h: the source the kernels run on the device) under the
// host sanitizers.  This stand-alone program reads vectors Python's exact arithmetic wrote
// (tools/decimal_vectors.py: one line per value, "scale lo hi double-bits toByteArray-hex") and
// checks to_double and the toByteArray stream against them.
//
//   python tools/decimal_vectors.py /tmp/decimal_vectors.txt
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I deequ_amd/csrc tools/decimal_check.cpp -o /tmp/decimal_check
//   /tmp/decimal_check /tmp/decimal_vectors.txt
//
// Host code only: it is never loaded into Python and never runs on a GPU.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>

#include "dq_decimal.h"

namespace {

int failures = 0;
#define CHECK(cond)                                                   \
  do {                                                                \
    if (!(cond)) {                                                    \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);   \
      ++failures;                                                     \
    }                                                                 \
  } while (0)

uint64_t bits_of(double d) {
  uint64_t b;
  std::memcpy(&b, &d, 8);
  return b;
}

// toByteArray of (lo, hi) as lowercase hex, written through an allocation of exactly its length
std::string byte_hex(uint64_t lo, int64_t hi) {
  const int len = dq::dec::byte_length(lo, hi);
  const dq::dec::u128 st = dq::dec::be_stream(lo, hi, len);
  uint8_t* exact = static_cast<uint8_t*>(std::malloc((size_t)len));
  for (int j = 0; j < len; ++j) exact[j] = (uint8_t)(st >> (8 * j));
  std::string out;
  char buf[3];
  for (int j = 0; j < len; ++j) {
    std::snprintf(buf, sizeof buf, "%02x", exact[j]);
    out += buf;
  }
  std::free(exact);
  return out;
}

}  // namespace

int main(int argc, char** argv) {
  {  // by hand: BigInteger.toByteArray's documented shapes, and a few casts
    CHECK(byte_hex(0, 0) == "00");
    CHECK(byte_hex(128, 0) == "0080");
    CHECK(byte_hex((uint64_t)-128, -1) == "80");
    CHECK(byte_hex((uint64_t)-129, -1) == "ff7f");
    CHECK(byte_hex(0, INT64_MIN).size() == 32);
    CHECK(dq::dec::to_double(0, 0, 38) == 0.0);
    CHECK(dq::dec::to_double(12345, 0, 2) == 123.45);
    CHECK(dq::dec::to_double((uint64_t)-12345, -1, 2) == -123.45);
    CHECK(dq::dec::to_double(0, INT64_MIN, 0) == -0x1p127);
    CHECK(dq::dec::to_double(1, 0, 38) == 1e-38);
  }
  long long n = 0;
  if (argc > 1) {
    std::ifstream in(argv[1]);
    if (!in) {
      std::printf("decimal_check: cannot read %s\n", argv[1]);
      return 2;
    }
    std::string line;
    while (std::getline(in, line)) {
      if (line.empty()) continue;
      std::istringstream ls(line);
      int scale;
      unsigned long long lo, hi, want;
      std::string hx;
      ls >> scale >> std::hex >> lo >> hi >> want >> hx;
      if (!ls) {
        std::printf("decimal_check: malformed line: %s\n", line.c_str());
        return 2;
      }
      const uint64_t got = bits_of(dq::dec::to_double((uint64_t)lo, (int64_t)hi, scale));
      if (got != (uint64_t)want) {
        std::printf("FAILED cast %s: got %016llx, want %016llx\n", line.c_str(), (unsigned long long)got, want);
        ++failures;
      }
      const std::string bytes = byte_hex((uint64_t)lo, (int64_t)hi);
      if (bytes != hx) {
        std::printf("FAILED bytes %s: got %s\n", line.c_str(), bytes.c_str());
        ++failures;
      }
      ++n;
    }
  }
  if (failures) std::printf("decimal_check: %d check(s) FAILED (%lld values from the file)\n", failures, n);
  else std::printf("decimal_check: all checks passed (%lld values from the file)\n", n);
  return failures ? 1 : 0;
}
