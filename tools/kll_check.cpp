// kll_check.cpp -- KLLSketch's host sketch (deequ_amd/csrc/dq_kll.h, dq_kll.cpp) under the host
// sanitizers.  This stand-alone program runs the sequential sketch and the slab-and-tree layout
// over the layouts the tests use (k = 2 with slabs of 37 and 1000 rows, k = 64 with 4096,
// k = 2048 with 1000, 4096 and 50 000; 300 000 seeded rows with ~5 % NULLs; NaN, infinities and
// signed zeros) and checks the reference's known answers (KLLProfileTest.scala:59-155), weight
// conservation, the export image, and the reference's rank criterion (KLLProbTest.scala).
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I deequ_amd/csrc tools/kll_check.cpp deequ_amd/csrc/dq_kll.cpp -o /tmp/kll_check
//   /tmp/kll_check
//
// Host code only: it is never loaded into Python and never runs on a GPU.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "dq_kll.h"

namespace {

using dq::kll::Sketch;

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint64_t rnd() {  // splitmix64
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
double uniform() { return (double)(rnd() >> 11) * (1.0 / 9007199254740992.0); }

int failures = 0;
#define CHECK(cond)                                                   \
  do {                                                                \
    if (!(cond)) {                                                    \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);   \
      ++failures;                                                     \
    }                                                                 \
  } while (0)

std::vector<std::vector<double>> items(const Sketch& s) {
  std::vector<std::vector<double>> out;
  for (const auto& c : s.levels) out.push_back(c.buf);
  return out;
}

void check_export(const Sketch& s) {
  std::vector<int64_t> words((size_t)s.export_words());
  s.export_to(words.data());
  CHECK(words[0] == (int64_t)s.levels.size());
  int64_t n = 0;
  for (size_t h = 0; h < s.levels.size(); ++h) {
    CHECK(words[3 + 3 * h] == (int64_t)s.levels[h].buf.size());
    n += words[3 + 3 * h];
  }
  CHECK(3 + 3 * (int64_t)s.levels.size() + n == s.export_words());
}

}  // namespace

int main() {
  using V = std::vector<std::vector<double>>;
  {  // KLLProfileTest.scala:59-87 and :127-155: 1..6 with KLLParameters(2, 0.64, 2)
    Sketch s(2, 0.64);
    for (int i = 1; i <= 6; ++i) s.update_untyped(i);
    CHECK(items(s) == (V{{5, 6}, {1, 3}}));
    CHECK(s.min == 1.0 && s.max == 6.0);
    CHECK(s.rank_exclusive(3.5) - s.rank_exclusive(1.0) == 4 && s.rank(6.0) - s.rank_exclusive(3.5) == 2);
  }
  {  // KLLProfileTest.scala:96-121: 1..30
    Sketch s(2, 0.64);
    for (int i = 1; i <= 30; ++i) s.update_untyped(i);
    CHECK(items(s) == (V{{27, 28, 29, 30}, {25}, {1, 6, 10, 15, 19, 23}}));
    CHECK(s.rank_exclusive(15.5) - s.rank_exclusive(1.0) == 16 && s.rank(30.0) - s.rank_exclusive(15.5) == 14);
    check_export(s);
  }
  const int64_t n = 300000;
  std::vector<double> vals((size_t)n);
  std::vector<uint8_t> valid((size_t)n);
  int64_t n_valid = 0;
  for (int64_t i = 0; i < n; ++i) {
    vals[i] = (uniform() - 0.5) * 2e4;
    valid[i] = uniform() >= 0.05;
    n_valid += valid[i];
  }
  const struct { int k; int64_t slab; } layouts[] = {{2, 37}, {2, 1000}, {64, 4096}, {2048, 1000}, {2048, 4096},
                                                     {2048, 50000}, {2048, 300000}};
  for (const auto& l : layouts) {
    const Sketch s = dq::kll::sketch_slabs(vals.data(), valid.data(), n, l.k, 0.64, l.slab);
    CHECK(s.weight() == n_valid);
    CHECK(s.actual < s.total || l.slab >= n);
    CHECK(s.rank(s.max) == n_valid && s.rank_exclusive(s.min) == 0);
    check_export(s);
    std::printf("k=%d slab_rows=%lld: %zu levels, %lld items, weight %lld\n", l.k, (long long)l.slab, s.levels.size(),
                (long long)s.actual, (long long)s.weight());
  }
  {  // NaN, infinities, signed zeros; an all-NULL input; an empty one
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    std::vector<double> sp;
    for (int r = 0; r < 40; ++r)
      for (double v : {0.0, -0.0, inf, -inf, nan, 1.5, -0.0, 0.0, nan, 1152921504606846976.0, -3.0}) sp.push_back(v);
    for (int64_t slab : {7, 1000}) {
      const Sketch s = dq::kll::sketch_slabs(sp.data(), nullptr, (int64_t)sp.size(), 2, 0.64, slab);
      CHECK(s.weight() == (int64_t)sp.size());
      CHECK(s.min != s.min && s.max != s.max);
    }
    std::vector<uint8_t> none(sp.size(), 0);
    const Sketch e = dq::kll::sketch_slabs(sp.data(), none.data(), (int64_t)sp.size(), 2048, 0.64, 16);
    CHECK(e.weight() == 0 && e.min == dq::kll::kInitMin && e.max == dq::kll::kInitMax);
    const Sketch z = dq::kll::sketch_slabs(nullptr, nullptr, 0, 2048, 0.64, 16);
    CHECK(z.weight() == 0 && z.levels.size() == 1);
    check_export(z);
  }
  for (int k : {100, 1000}) {  // KLLProbTest.scala:28-56, the zoom-in stream, and :89-122, ten merged partitions
    const int64_t len = 1000000;
    Sketch s(k, 0.64);
    for (int64_t i = 1; i <= len / 2; ++i) {
      s.update((double)i);
      s.update((double)(len + 1 - i));
    }
    const double eps = 100.0 / k;
    const int64_t step = (int64_t)std::ceil(std::fmax(eps * 0.2 * len, 1));
    int bad = 0;
    for (int64_t x = 1; x < len; x += step)
      if (std::llabs(s.rank((double)x) - x) >= eps * len) ++bad;
    CHECK(bad == 0);
    Sketch last(k, 0.64);
    const int64_t plen = 100000;
    for (int m = 0; m < 10; ++m) {
      Sketch part(k, 0.64);
      for (int64_t i = 1; i <= plen / 2; ++i) {
        part.update((double)(i + m * plen));
        part.update((double)(m * plen + plen + 1 - i));
      }
      last.merge(part);
    }
    bad = 0;
    for (int64_t x = 1; x < plen * 10; x += step)
      if (std::llabs(last.rank((double)x) - x) >= eps * plen * 10) ++bad;
    CHECK(bad == 0 && last.weight() == plen * 10);
  }
  std::printf(failures ? "kll_check: %d check(s) FAILED\n" : "kll_check: all checks passed\n", failures);
  return failures ? 1 : 0;
}
