// take_check.cpp -- take's byte-copy addressing (deequ_amd/csrc/dq_take.h: copy_plan, the source
// dq_take_bytes_kernel and dq_take_pieces_kernel run on the device) under the host sanitizers.
// This stand-alone program copies cells of the lengths tests/test_gpu_take.py uses -- 0, 1, 3, 4,
// 5, 15, 16, 17 and both thresholds -1, +0, +1 -- from every source residue mod 16 to every
// destination residue mod 16, as one lane, as the 64 lanes of a wave and as the 256 lanes of a
// workgroup (the three ways the kernels call it), and cut into pieces as the pieces kernel cuts a
// long cell.  Every source and destination is an allocation of its own that ends with the cell's
// last byte (and starts at most 15 bytes before its first, which gives the address its residue),
// so an access past the cell is an AddressSanitizer error.  Each access is checked to be 16, 4 or 1 bytes wide, aligned to its width at both
// addresses and inside the cell; every byte must be written exactly once; the result is compared
// byte for byte.  find_chunk is checked against a linear search, empty chunks included.
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I deequ_amd/csrc tools/take_check.cpp -o /tmp/take_check
//   /tmp/take_check
//
// Host code only: it is never loaded into Python and never runs on a GPU.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "dq_take.h"

namespace {

namespace take = dq::take;

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

// `len` bytes whose first byte's address is `residue` mod 16 and whose last byte is the last of
// the allocation: malloc's blocks are 16-byte aligned, so the cell starts `residue` bytes in, and
// those bytes in front are the only slack (an access before the cell fails HostCopy's own check).
struct Exact {
  uint8_t* block = nullptr;
  uint8_t* p = nullptr;
  Exact(int64_t len, int residue) {
    block = static_cast<uint8_t*>(std::malloc((size_t)len + (size_t)residue + (len + residue == 0 ? 1 : 0)));
    if (block && (reinterpret_cast<uintptr_t>(block) & 15u) == 0u) p = block + residue;
  }
  ~Exact() { std::free(block); }
};

// copy_plan's access on the host: checked, counted, then one memcpy of the width.
struct HostCopy {
  const uint8_t* s;
  uint8_t* d;
  int64_t len;
  std::vector<uint8_t>* written;
  void operator()(int64_t off, int width) {
    CHECK(width == 16 || width == 4 || width == 1);
    CHECK(off >= 0 && off + width <= len);
    CHECK(((reinterpret_cast<uintptr_t>(s) + (uintptr_t)off) & (uintptr_t)(width - 1)) == 0);
    CHECK(((reinterpret_cast<uintptr_t>(d) + (uintptr_t)off) & (uintptr_t)(width - 1)) == 0);
    if (off < 0 || off + width > len) return;
    std::memcpy(d + off, s + off, (size_t)width);
    for (int i = 0; i < width; ++i) ++(*written)[(size_t)(off + i)];
  }
};

// One cell copied by n_lanes lanes, in pieces of `piece` bytes (piece >= len: in one).
void copy_cell(int64_t len, int src_res, int dst_res, int n_lanes, int64_t piece) {
  Exact src(len, src_res), dst(len, dst_res);
  CHECK(src.p && dst.p);
  if (!src.p || !dst.p) return;
  for (int64_t i = 0; i < len; ++i) src.p[i] = (uint8_t)((i * 7 + src_res * 13 + dst_res) % 251 + 1);
  std::memset(dst.p, 0, (size_t)len);
  std::vector<uint8_t> written((size_t)len, 0);
  for (int64_t at = 0; at < len || at == 0; at += piece) {
    const int64_t n = len - at < piece ? len - at : piece;
    HostCopy op{src.p + at, dst.p + at, n, nullptr};
    std::vector<uint8_t> w((size_t)n, 0);
    op.written = &w;
    for (int lane = 0; lane < n_lanes; ++lane)
      take::copy_plan(reinterpret_cast<uintptr_t>(src.p + at), reinterpret_cast<uintptr_t>(dst.p + at), n, lane, n_lanes, op);
    for (int64_t i = 0; i < n; ++i) written[(size_t)(at + i)] = (uint8_t)(written[(size_t)(at + i)] + w[(size_t)i]);
    if (len == 0) break;
  }
  bool once = true;
  for (int64_t i = 0; i < len; ++i) once = once && written[(size_t)i] == 1;
  CHECK(once);
  CHECK(len == 0 || std::memcmp(src.p, dst.p, (size_t)len) == 0);
  // the widest unit is used where the residues allow it
  const int unit = take::copy_unit(reinterpret_cast<uintptr_t>(src.p), reinterpret_cast<uintptr_t>(dst.p));
  CHECK(unit == (src_res == dst_res ? 16 : (src_res & 3) == (dst_res & 3) ? 4 : 1));
}

void check_find_chunk() {
  const std::vector<std::vector<int64_t>> layouts = {{10}, {1, 64, 35}, {1, 64, 0, 35}, {0, 0, 5, 0, 0, 7, 0}, {3, 0}};
  for (const auto& rows : layouts) {
    std::vector<int64_t> prefix(rows.size() + 1, 0);
    for (size_t c = 0; c < rows.size(); ++c) prefix[c + 1] = prefix[c] + rows[c];
    for (int64_t idx = 0; idx < prefix.back(); ++idx) {
      int want = 0;
      while (!(prefix[(size_t)want] <= idx && idx < prefix[(size_t)want + 1])) ++want;
      const int got = take::find_chunk(prefix.data(), (int)rows.size(), idx);
      CHECK(got == want);
      CHECK(rows[(size_t)got] > 0);
    }
  }
  std::vector<int64_t> many(take::kMaxChunks + 1, 0);
  for (int c = 0; c < take::kMaxChunks; ++c) many[(size_t)c + 1] = many[(size_t)c] + (c % 3);
  for (int64_t idx = 0; idx < many.back(); idx += 5) {
    const int got = take::find_chunk(many.data(), take::kMaxChunks, idx);
    CHECK(many[(size_t)got] <= idx && idx < many[(size_t)got + 1]);
  }
}

}  // namespace

int main() {
  const int64_t lengths[] = {0, 1, 3, 4, 5, 15, 16, 17, take::kWaveBytes - 1, take::kWaveBytes, take::kWaveBytes + 1,
                             take::kSplitBytes - 1, take::kSplitBytes, take::kSplitBytes + 1};
  for (int64_t len : lengths)
    for (int s = 0; s < 16; ++s)
      for (int d = 0; d < 16; ++d) {
        copy_cell(len, s, d, 1, INT64_MAX);                       // a lane on its own
        copy_cell(len, s, d, 64, INT64_MAX);                      // a wave
        copy_cell(len, s, d, take::kRowsPerBlock, take::kSplitBytes);  // a workgroup per piece
      }
  // a long cell: four pieces and a rest
  for (int s = 0; s < 16; s += 5)
    for (int d = 0; d < 16; d += 3) copy_cell(4 * take::kSplitBytes + 37, s, d, take::kRowsPerBlock, take::kSplitBytes);
  check_find_chunk();
  std::printf("%s: %ld checks, %d failures\n", failures ? "FAILED" : "ok", checks, failures);
  return failures ? 1 : 0;
}
