// dq_quantile.h -- ApproxQuantile / ApproxQuantiles (ApproxQuantile.scala, ApproxQuantiles.scala,
// StatefulApproxQuantile.scala): the Greenwald-Khanna digest on the host (dq_quantile.cpp) and what
// the host and the gfx950 multi-rank radix select (dq_quantile.hip) share.  DESIGN.md, ApproxQuantile,
// has the definitions: the order of values, the batch summary, the merge, the query and the
// serialised form.
#pragma once

#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define DQ_AQ_HD __host__ __device__ inline
#else
#define DQ_AQ_HD inline
#endif

namespace dq {
namespace aq {

constexpr int kMaxRanks = 2048;          // target ranks (and so active prefixes) of one batch summary
constexpr double kMinRelativeError = 0.001;  // 2 / eps + 2 target ranks must fit kMaxRanks
constexpr int kCounters = 32768;         // LDS counters of one workgroup: active prefixes x digit values
constexpr int kCountersLog = 15;
constexpr int kSelectBlock = 1024;       // threads of the counting and the planning workgroup
constexpr int kRowsPerThread = 8;     // loads a thread keeps in flight; a tile is 8192 rows
constexpr int kMaxBlocksPerPair = 256;   // one counting workgroup per CU
constexpr int32_t kCompressThreshold = 10000;  // written into the serialised form, not used here

constexpr uint64_t kCanonicalNaN = 0x7ff8000000000000ull;

// The sortable key of a double's bits (every NaN canonicalised first): unsigned order of the keys is
// java.lang.Double.compare's, -0.0 before 0.0, NaN last.
DQ_AQ_HD uint64_t canonical_bits(uint64_t b) {
  return (b & 0x7fffffffffffffffull) > 0x7ff0000000000000ull ? kCanonicalNaN : b;
}
DQ_AQ_HD uint64_t key_of_bits(uint64_t b) { return (b >> 63) ? ~b : (b | 0x8000000000000000ull); }
DQ_AQ_HD uint64_t bits_of_key(uint64_t k) { return (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k; }

inline uint64_t key_of_value(double v) {
  uint64_t b;
  memcpy(&b, &v, 8);
  return key_of_bits(canonical_bits(b));
}
inline double value_of_key(uint64_t k) {
  const uint64_t b = bits_of_key(k);
  double v;
  memcpy(&v, &b, 8);
  return v;
}

// Digit width of a pass over `n_active` active prefixes: every (prefix, digit value) has its own
// LDS counter, so 15 bits for one prefix down to 4 bits for 1025 .. 2048 of them.
DQ_AQ_HD int digit_bits(int n_active, int consumed) {
  int lg = 0;
  while ((1 << lg) < n_active) ++lg;
  const int bits = kCountersLog - lg, left = 64 - consumed;
  return bits < left ? bits : left;
}
// The most passes a batch can take when no pass has more than `ranks` active prefixes.
inline int max_passes(int ranks) {
  const int narrow = digit_bits(ranks, 0);
  return 1 + (64 - kCountersLog + narrow - 1) / narrow;
}

// gap and number of target ranks of a batch of n > 0 values: ranks 1, 1 + gap, ... while
// < n, then n.
DQ_AQ_HD int64_t batch_gap(double eps, int64_t n) {
  const int64_t g = (int64_t)(eps * (double)n);  // floor: the product is not negative
  return g < 1 ? 1 : g;
}
DQ_AQ_HD int64_t batch_ranks(int64_t n, int64_t gap) { return (n - 1 + gap - 1) / gap + 1; }
DQ_AQ_HD int64_t batch_rank(int64_t j, int64_t m, int64_t n, int64_t gap) { return j < m - 1 ? 1 + j * gap : n; }

// A (column, relativeError) of one launch.
struct DevAqPair {
  const void* values;       // row 0 of the batch at values[0]
  const uint8_t* validity;  // nullptr = all valid; row 0 at bit `bit_offset`
  int64_t bit_offset;
  int32_t type;             // dq_type
  int32_t pad;
  double eps;
};

// The select's working set of one pair in device memory, zeroed before a batch.
struct DevAqState {
  int32_t n_active, consumed, bits, cur;  // of the pass to come (pass 0: 1, 0, 15, 0 by definition)
  int32_t done, error;                    // error 1: more than kMaxRanks target ranks or prefixes
  int64_t n, gap, m;                      // valid rows, gap, target ranks (after pass 0)
};
struct alignas(16) DevAqWork {
  uint64_t prefix[2][kMaxRanks];  // active prefixes in ascending order, right-aligned
  uint32_t base[2][kMaxRanks];    // valid rows whose key lies before the prefix
  uint32_t jlo[2][kMaxRanks];     // first target rank index inside the prefix
  uint32_t hist[kCounters];       // counter of (active a, digit d) at (a << bits) + d
  uint64_t keys[kMaxRanks];       // the result: key at target rank j
  DevAqState st;
};

// ---------------------------------------------------------------- the host digest
struct Entry {
  double value;
  int64_t g, delta;
};

struct Digest {
  double eps = 0;
  int64_t count = 0;
  std::vector<Entry> sampled;

  explicit Digest(double relative_error = 0) : eps(relative_error) {}
  // the batch summary from the keys at its target ranks (n valid values)
  static Digest from_batch(double eps, int64_t n, const uint64_t* keys, int64_t m);
  // merge(this, that) -> this; false when the relative errors differ
  bool merge(const Digest& that);
  double query(double q, bool* empty) const;
  int64_t serialised_bytes() const { return 4 + 8 + 8 + 4 + 16 * (int64_t)sampled.size(); }
  bool fits_int32() const;  // every g and delta (the serialised form holds Int)
  void serialise(uint8_t* out) const;
  static bool deserialise(const uint8_t* in, int64_t len, Digest* out);
};

}  // namespace aq
}  // namespace dq
