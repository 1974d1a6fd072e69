// aq_check.cpp -- ApproxQuantile's host digest (deequ_amd/csrc/dq_quantile.h, dq_quantile.cpp) under
// the host sanitizers.  This stand-alone program folds a few thousand random batch summaries
// (normal, constant, two-valued, descending and special-value columns; relativeError 0.25, 0.01 and
// 0.001; batches of 1 to a few thousand values) through merge and compress, and checks after every
// merge: the sum of g is the count, g + delta <= max(1, floor(2 eps n)), the running sums of g
// bracket the true ranks, every query is within ceil(eps n) ranks, and the serialised form
// round-trips.  It also checks the reference's known answers (AnalysisTest.scala:95,
// AnalyzerTests.scala:570-601, IncrementalAnalyzerTest.scala:176-199).
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I deequ_amd/csrc tools/aq_check.cpp deequ_amd/csrc/dq_quantile.cpp -o /tmp/aq_check
//   /tmp/aq_check
//
// Host code only: it is never loaded into Python and never runs on a GPU.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "dq_quantile.h"

namespace {

using dq::aq::Digest;

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint64_t rnd() {  // splitmix64
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
double uniform() { return (double)(rnd() >> 11) * (1.0 / 9007199254740992.0); }
double normal() { return std::sqrt(-2.0 * std::log(1.0 - uniform())) * std::cos(6.283185307179586 * uniform()); }

int failures = 0;
#define CHECK(cond)                                                 \
  do {                                                              \
    if (!(cond)) {                                                  \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++failures;                                                   \
    }                                                               \
  } while (0)

double draw(int kind, int64_t i) {
  switch (kind) {
    case 0: return normal() * 1e4;
    case 1: return 42.5;
    case 2: return uniform() < 0.3 ? -1.5 : 7.25;
    case 3: return 1e6 - (double)i;
    default: {
      const uint64_t r = rnd() % 16;
      if (r == 0) return 0.0;
      if (r == 1) return -0.0;
      if (r == 2) return std::numeric_limits<double>::infinity();
      if (r == 3) return -std::numeric_limits<double>::infinity();
      if (r == 4) return std::numeric_limits<double>::quiet_NaN();
      return normal();
    }
  }
}

// the batch summary as the GPU hands it over: the sorted keys at the target ranks
Digest summarise(double eps, const std::vector<double>& values, std::vector<uint64_t>* all_keys) {
  std::vector<uint64_t> keys(values.size());
  for (size_t i = 0; i < values.size(); ++i) keys[i] = dq::aq::key_of_value(values[i]);
  std::sort(keys.begin(), keys.end());
  all_keys->insert(all_keys->end(), keys.begin(), keys.end());
  const int64_t n = (int64_t)keys.size();
  if (n == 0) return Digest(eps);
  const int64_t gap = dq::aq::batch_gap(eps, n), m = dq::aq::batch_ranks(n, gap);
  std::vector<uint64_t> picked((size_t)m);
  for (int64_t j = 0; j < m; ++j) picked[(size_t)j] = keys[(size_t)(dq::aq::batch_rank(j, m, n, gap) - 1)];
  CHECK((double)m <= 2.0 / eps + 2.0);
  return Digest::from_batch(eps, n, picked.data(), m);
}

void check_digest(const Digest& d, std::vector<uint64_t>& sorted_keys) {
  std::sort(sorted_keys.begin(), sorted_keys.end());
  const int64_t n = (int64_t)sorted_keys.size();
  CHECK(d.count == n);
  const int64_t bound = std::max<int64_t>(1, (int64_t)std::floor(2.0 * d.eps * (double)n));
  int64_t rmin = 0;
  uint64_t prev = 0;
  for (const dq::aq::Entry& e : d.sampled) {
    CHECK(e.g >= 1 && e.delta >= 0 && e.g + e.delta <= bound);
    rmin += e.g;
    const uint64_t k = dq::aq::key_of_value(e.value);
    CHECK(k >= prev);
    prev = k;
    const int64_t lo = std::lower_bound(sorted_keys.begin(), sorted_keys.end(), k) - sorted_keys.begin() + 1;
    const int64_t hi = std::upper_bound(sorted_keys.begin(), sorted_keys.end(), k) - sorted_keys.begin();
    CHECK(lo <= hi && lo <= rmin + e.delta && rmin <= hi);
  }
  CHECK(rmin == n);
  const int64_t allowed = (int64_t)std::ceil(d.eps * (double)n);
  const double qs[] = {0.0, 0.001, 0.01, 0.25, 0.5, 0.75, 0.99, 1.0};
  for (double q : qs) {
    bool empty = false;
    const double v = d.query(q, &empty);
    CHECK(empty == (n == 0));
    if (empty) continue;
    const int64_t t = std::max<int64_t>(1, (int64_t)std::ceil(q * (double)n));
    const uint64_t k = dq::aq::key_of_value(v);
    const int64_t lo = std::lower_bound(sorted_keys.begin(), sorted_keys.end(), k) - sorted_keys.begin() + 1;
    const int64_t hi = std::upper_bound(sorted_keys.begin(), sorted_keys.end(), k) - sorted_keys.begin();
    const int64_t err = (lo <= t && t <= hi) ? 0 : std::min(std::llabs(t - lo), std::llabs(t - hi));
    CHECK(err <= allowed);
  }
  std::vector<uint8_t> raw((size_t)d.serialised_bytes());
  CHECK(d.fits_int32());
  d.serialise(raw.data());
  Digest back;
  CHECK(Digest::deserialise(raw.data(), (int64_t)raw.size(), &back));
  CHECK(back.eps == d.eps && back.count == d.count && back.sampled.size() == d.sampled.size());
  for (size_t i = 0; i < back.sampled.size() && i < d.sampled.size(); ++i)
    CHECK(dq::aq::key_of_value(back.sampled[i].value) == dq::aq::key_of_value(d.sampled[i].value) &&
          back.sampled[i].g == d.sampled[i].g && back.sampled[i].delta == d.sampled[i].delta);
  CHECK(!Digest::deserialise(raw.data(), (int64_t)raw.size() - 1, &back));
}

double answer(const Digest& d, double q) {
  bool empty = false;
  return d.query(q, &empty);
}

}  // namespace

int main() {
  int64_t merges = 0;
  const double errors[] = {0.25, 0.01, 0.001};
  for (double eps : errors)
    for (int kind = 0; kind < 5; ++kind)
      for (int run = 0; run < 4; ++run) {
        Digest acc(eps);
        std::vector<uint64_t> keys;
        const int batches = run == 0 ? 1 : run == 1 ? 3 : run == 2 ? 10 : 60;
        int64_t row = 0;
        for (int b = 0; b < batches; ++b) {
          const int64_t n = run == 3 ? (int64_t)(rnd() % 700) : (int64_t)(1 + rnd() % 4000);
          std::vector<double> values((size_t)n);
          for (int64_t i = 0; i < n; ++i) values[(size_t)i] = draw(kind, row++);
          CHECK(acc.merge(summarise(eps, values, &keys)));
          ++merges;
          check_digest(acc, keys);
        }
      }
  {  // many small merges into one digest, and a digest merged with itself
    Digest acc(0.01);
    std::vector<uint64_t> keys;
    for (int b = 0; b < 2500; ++b) {
      std::vector<double> values((size_t)(1 + rnd() % 40));
      for (double& v : values) v = normal();
      CHECK(acc.merge(summarise(0.01, values, &keys)));
      ++merges;
      if (b % 100 == 99) check_digest(acc, keys);
    }
    const Digest copy = acc;
    CHECK(acc.merge(copy));
    keys.insert(keys.end(), keys.begin(), keys.begin() + (std::ptrdiff_t)keys.size());
    check_digest(acc, keys);
    CHECK(!acc.merge(Digest(0.02)));
  }
  {  // the reference's known answers
    std::vector<uint64_t> keys;
    CHECK(answer(summarise(0.01, {1, 2, 3, 4, 5, 6}, &keys), 0.5) == 3.0);
    std::vector<double> range;
    for (int v = -1000; v < 1000; ++v) range.push_back(v);
    const Digest r = summarise(0.01, range, &keys);
    CHECK(answer(r, 0.5) == 0.0 && answer(r, 0.25) == -500.0 && answer(r, 0.75) == 500.0);
    Digest first = summarise(0.01, {0.0, 1.0, 2.0}, &keys);
    CHECK(first.merge(summarise(0.01, {-2.0, -1.0}, &keys)));
    CHECK(answer(first, 0.5) == 0.0);
    CHECK(answer(summarise(0.01, {0.0, 1.0, 2.0, -2.0, -1.0}, &keys), 0.5) == 0.0);
  }
  std::printf("%lld merges, %d failures\n", (long long)merges, failures);
  return failures ? 1 : 0;
}
