// dq_kll.h -- KLLSketch (KLLSketch.scala, QuantileNonSample.scala, NonSampleCompactor.scala):
// the sequential reference sketch on the host, the capacity table, and what the host and the
// gfx950 kernels (dq_kll.hip) share: the sortable key of a double and the per-sketch device record.
//
// The reference's sketch is deterministic (the random offset of NonSampleCompactor.scala:46-51 is
// commented out), so a fixed partitioning pins its result exactly.  The partitioning here: a
// consumed batch is cut into slabs of `slab_rows` consecutive rows, every slab is one reference
// partition (KLLRunner.scala:150-177), and the slabs of a batch are merged by a balanced tree in
// slab order (round r: slab 2^(r+1) j absorbs slab 2^(r+1) j + 2^r); batches merge in arrival order.
#pragma once

#include <stdint.h>
#include <string.h>

#include <vector>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define DQ_KLL_HD __host__ __device__ inline
#else
#define DQ_KLL_HD inline
#endif

namespace dq {
namespace kll {

constexpr int kMaxLevels = 64;                 // a level h item weighs 2^h rows
constexpr int64_t kDefaultSlabRows = 1 << 16;  // rows per slab unless the sketcher overrides it
constexpr int kLdsBudgetBytes = 160 * 1024;    // one workgroup may hold all of a CU's LDS
constexpr int kLdsReserveBytes = 2048;         // level tables and reduction scratch
// items one workgroup keeps resident: the tree merge holds two sketches' items at once
constexpr int kMaxPoolItems = (kLdsBudgetBytes - kLdsReserveBytes) / 8;

// A double as a uint64 whose unsigned order is java.lang.Double.compare's for every non-NaN value
// (-0.0 before 0.0); invertible.  NaNs of either sign go last through key_ord (their order among
// themselves is by payload here; the reference's stable sort keeps them in arrival order).
DQ_KLL_HD uint64_t key_of_bits(uint64_t b) { return (b >> 63) ? ~b : (b | 0x8000000000000000ull); }
DQ_KLL_HD uint64_t bits_of_key(uint64_t k) { return (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k; }
DQ_KLL_HD uint64_t key_ord(uint64_t k) { return k < 0x000fffffffffffffull ? ~k : k; }  // negative NaNs
DQ_KLL_HD bool key_is_nan(uint64_t k) { return key_ord(k) > 0xfff0000000000000ull; }

inline double value_of_key(uint64_t k) {
  const uint64_t b = bits_of_key(k);
  double v;
  memcpy(&v, &b, 8);
  return v;
}

// KLLRunner.scala:28-29: the reference starts min / max at Int.MaxValue / Int.MinValue
constexpr double kInitMin = 2147483647.0;
constexpr double kInitMax = -2147483648.0;

// One sketch in device memory (the kernels' input and output; one per (column, slab)).
struct DevSketch {
  int32_t n_levels;
  int32_t error;  // 1: the levels outgrew the LDS pool, 2: more than kMaxLevels levels
  int32_t has_nan;
  int32_t pad;
  uint64_t min_key, max_key;  // of the non-NaN values, from kInitMin / kInitMax
  int32_t len[kMaxLevels];
  int32_t num_compress[kMaxLevels];
  int32_t offset[kMaxLevels];
  // the items follow in their own array: `stride` keys per sketch, level 0 first
};

// A (column, parameters) of one launch.
struct DevKllColumn {
  const void* values;       // row 0 of the batch at values[0]
  const uint8_t* validity;  // nullptr = all valid; row 0 at bit `bit_offset`
  int64_t bit_offset;
  int32_t type;             // dq_type
  int32_t pool_items;       // LDS pool of the slab kernel for these parameters
  int64_t stride;           // item keys per sketch in the item array
  int64_t sketch_base;      // first DevSketch of this column (one per slab)
  int64_t item_base;        // first item key of this column's blocks (slab s at item_base + s * stride)
  int32_t cap[kMaxLevels];
};

// capacity(height) = 2 * (ceil(sketchSize * pow(shrinkingFactor, height) / 2).toInt + 1)
// (QuantileNonSample.scala:78-80), in double on the host; .toInt saturates and maps NaN to 0.
int64_t capacity(int32_t sketch_size, double shrinking_factor, int height);
void capacity_table(int32_t sketch_size, double shrinking_factor, int32_t* cap, int64_t* sum);
// an upper bound of the levels a sketch of n updates can have
int levels_bound(const int32_t* cap, int64_t n);

bool java_less(double a, double b);     // java.lang.Double.compare(a, b) < 0
double java_min(double a, double b);    // java.lang.Math.min
double java_max(double a, double b);

struct Compactor {  // NonSampleCompactor
  int32_t num_compress = 0, offset = 0;
  std::vector<double> buf;
  std::vector<double> compact();
};

struct Sketch {  // QuantileNonSample[Double] with the min / max of UntypedQuantileNonSample
  int32_t sketch_size;
  double shrinking_factor;
  std::vector<Compactor> levels;
  int64_t actual = 0, total = 0;
  double min = kInitMin, max = kInitMax;

  Sketch(int32_t k, double c);
  int64_t cap(int h) const { return capacity(sketch_size, shrinking_factor, h); }
  void expand();
  void update(double v);         // sketch.update only
  void update_untyped(double v); // min, max, update (KLLRunner.scala:34-38)
  void condense();
  void merge(const Sketch& that);         // QuantileNonSample.merge
  void merge_untyped(const Sketch& that); // with min / max (KLLRunner.scala:40-44)
  int64_t rank(double x) const;           // getRank: weight of the items not greater than x
  int64_t rank_exclusive(double x) const; // getRankExclusive: weight of the items less than x
  int64_t weight() const;                 // sum len(level i) * 2^i
  int64_t export_words() const;           // 8-byte words of export_to
  void export_to(void* out) const;
};

// The slab-and-tree layout on the host: values[i] is row i (valid[i] != 0 or valid == nullptr).
Sketch sketch_slabs(const double* values, const uint8_t* valid, int64_t n, int32_t k, double c, int64_t slab_rows);

}  // namespace kll
}  // namespace dq
