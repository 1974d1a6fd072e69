// corrmat_check.cpp -- the correlation matrix's host path (deequ_amd/csrc/dq_corrmat.h: corrmat_host,
// the mirror of the kernel's slabs, shifts, guard, flags and merges, and corrmat_pair_rescue) under
// the host sanitizers.  Every column, validity and filter array is allocated at exactly its length,
// so a read one element outside a batch is an AddressSanitizer error; the results are checked
// against a two-pass long double computation of the same pairs.
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I deequ_amd/csrc tools/corrmat_check.cpp -o /tmp/corrmat_check
//   /tmp/corrmat_check
//
// Host code only: it is never loaded into Python and never runs on a GPU.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "dq_corrmat.h"

namespace {

int failures = 0;
#define CHECK(cond)                                                   \
  do {                                                                \
    if (!(cond)) {                                                    \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);   \
      ++failures;                                                     \
    }                                                                 \
  } while (0)

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint64_t next_u64() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return rng_state;
}

template <typename T>
T* exact_alloc(size_t n) {
  return n ? static_cast<T*>(std::malloc(n * sizeof(T))) : nullptr;
}

bool close_to(double got, long double want, long double scale) {
  if (want == 0.0L && scale == 0.0L) return got == 0.0;
  return std::fabs((long double)got - want) <= 1e-11L * scale;
}

// k columns of n rows; nulls / filter / special: 0 none, 1 some
void run_case(int k, int64_t n, bool nulls, bool filter, int special, int64_t max_ranges) {
  std::vector<double*> cols(k);
  std::vector<uint8_t*> valid(k, nullptr);
  uint8_t* where = filter ? exact_alloc<uint8_t>((size_t)n) : nullptr;
  for (int i = 0; i < k; ++i) {
    cols[i] = exact_alloc<double>((size_t)n);
    if (nulls && i % 2 == 1) valid[i] = exact_alloc<uint8_t>((size_t)n);
    for (int64_t r = 0; r < n; ++r) {
      cols[i][r] = 1000.0 * (i + 1) + (double)(int64_t)(next_u64() % 8193) / 8.0;
      if (valid[i]) valid[i][r] = next_u64() % 20 != 0;
    }
  }
  for (int64_t r = 0; r < n && where; ++r) where[r] = next_u64() % 2;
  if (special == 1 && n > 0) {  // an outlier shift on every slab of column 0
    for (int64_t r = 0; r < n; r += dq::kCorrmatSlabRows) cols[0][r] = 1e8;
  } else if (special == 2 && n > 2) {  // non-finite values in column 0
    cols[0][1] = INFINITY;
    cols[0][n - 1] = NAN;
  }
  const int64_t n_pairs = dq::corrmat_pairs(k);
  double* states = exact_alloc<double>((size_t)n_pairs * 6);
  uint8_t* flags = exact_alloc<uint8_t>((size_t)n_pairs);
  dq::corrmat_host(cols.data(), nulls ? valid.data() : nullptr, where, k, n, max_ranges, states, flags);
  for (int i = 0; i < k; ++i)
    for (int j = i; j < k; ++j) {
      const int64_t p = dq::corrmat_pair_index(i, j, k);
      CHECK(p >= 0 && p < n_pairs);
      const bool expect_flag = special != 0 && i == 0 && n > 0;
      long double cnt = 0, mx = 0, my = 0;
      auto sel = [&](int64_t r) { return (!valid[i] || valid[i][r]) && (!valid[j] || valid[j][r]) && (!where || where[r]); };
      for (int64_t r = 0; r < n; ++r)
        if (sel(r)) cnt += 1, mx += cols[i][r], my += cols[j][r];
      const double* s = states + 6 * p;
      CHECK(s[0] == (double)cnt);
      if (special == 2 && i == 0) {
        CHECK(flags[p] == 1);
        continue;  // (NaN states: n alone is defined)
      }
      if (cnt >= 32) CHECK(flags[p] == (expect_flag ? 1 : 0));  // (a handful of rows may rightly trip the guard)
      if (cnt == 0) {
        CHECK(s[1] == 0.0 && s[2] == 0.0 && s[3] == 0.0 && s[4] == 0.0 && s[5] == 0.0);
        continue;
      }
      mx /= cnt, my /= cnt;
      long double ck = 0, xmk = 0, ymk = 0;
      for (int64_t r = 0; r < n; ++r)
        if (sel(r)) {
          const long double dx = cols[i][r] - mx, dy = cols[j][r] - my;
          ck += dx * dy, xmk += dx * dx, ymk += dy * dy;
        }
      CHECK(close_to(s[1], mx, std::fabs(mx)) && close_to(s[2], my, std::fabs(my)));
      CHECK(close_to(s[4], xmk, xmk) && close_to(s[5], ymk, ymk) && close_to(s[3], ck, std::sqrt(xmk * ymk)));
      if (i == j) CHECK(s[1] == s[2] && s[3] == s[4] && s[4] == s[5]);
    }
  for (int i = 0; i < k; ++i) {
    std::free(cols[i]);
    std::free(valid[i]);
  }
  std::free(where);
  std::free(states);
  std::free(flags);
}

}  // namespace

int main() {
  const int64_t S = dq::kCorrmatSlabRows;
  const int64_t rows[] = {0, 1, 3, 4, 5, 63, 64, 65, S - 1, S, S + 1, 3 * S + 7};
  const int ks[] = {1, 2, 15, 16, 17, 33, 64};
  for (int64_t n : rows)
    for (int nulls = 0; nulls < 2; ++nulls)
      for (int filter = 0; filter < 2; ++filter) run_case(5, n, nulls, filter, 0, n % 2 ? 0 : 2);
  for (int k : ks) run_case(k, S + 1, k % 2, false, 0, 3);
  for (int special = 1; special <= 2; ++special) run_case(4, 2 * S + 9, false, false, special, 0);
  for (int k = 1; k <= 64; ++k) {  // the triangular index against its enumeration
    int64_t at = 0;
    for (int i = 0; i < k; ++i)
      for (int j = i; j < k; ++j) CHECK(dq::corrmat_pair_index(i, j, k) == at++);
    CHECK(at == dq::corrmat_pairs(k));
  }
  std::printf("%s (%d failures)\n", failures ? "FAILED" : "ok", failures);
  return failures ? 1 : 0;
}
