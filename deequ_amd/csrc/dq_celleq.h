// dq_celleq.h -- the NULL-safe cell equality of the cross-table checks (`a <=> b` as Spark's
// EqualNullSafe evaluates it over two columns of one type), shared by the gfx950 match kernel
// (dq_freq.hip: dq_freq_match_rows_kernel), the host build behind dq_diag_cell_equal and
// tools/match_check.cpp.  Internal, not ABI.
//
//   NULL <=> NULL is TRUE, NULL <=> value FALSE; a NULL slot's payload is never read.
//   bool by bit; int8 .. int64 and decimal128 of one (precision, scale) by value, i.e. by their
//   bytes; float32 / float64 by Spark's double equality (`(isNaN(a) && isNaN(b)) || a == b`): any
//   NaN equals any NaN and -0.0 equals 0.0; utf8 by length, then by bytes.
//
// A utf8 row's bytes are only ever addressed inside [offsets[r], offsets[r + 1]) of either side:
// whole 8-byte words while at least 8 bytes remain, then single bytes.  The words are read
// unaligned (memcpy), so no aligned word around the row is touched either.
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
namespace celleq {

// dq_type codes (include/deequ_amd.h); a decimal's code carries (precision, scale) above the low byte.
enum : int32_t { T_BOOL = 1, T_INT8 = 2, T_INT16 = 3, T_INT32 = 4, T_INT64 = 5, T_FLOAT32 = 6, T_FLOAT64 = 7,
                 T_UTF8 = 8, T_DECIMAL128 = 9 };

// One column of either table, in place: row r of it is element `offset + r` of the buffers (bit
// `offset + r` of the validity bitmap and of a bool column's values), as a sliced Arrow array is.
struct Cells {
  const uint8_t* validity;  // nullptr = all valid
  const void* values;
  const int32_t* offsets;   // utf8
  int32_t type;
  int32_t pad;
  int64_t offset;
};

DQ_HD inline bool bit_at(const uint8_t* bits, int64_t i) { return (bits[i >> 3] >> (i & 7)) & 1u; }

DQ_HD inline bool is_null(const Cells& c, int64_t r) { return c.validity != nullptr && !bit_at(c.validity, c.offset + r); }

DQ_HD inline uint64_t load_u64(const uint8_t* p) {
  uint64_t v;
  __builtin_memcpy(&v, p, 8);
  return v;
}

DQ_HD inline bool bytes_equal(const uint8_t* a, const uint8_t* b, uint32_t n) {
  uint32_t k = 0;
  for (; k + 8 <= n; k += 8)
    if (load_u64(a + k) != load_u64(b + k)) return false;
  for (; k < n; ++k)
    if (a[k] != b[k]) return false;
  return true;
}

template <typename F>
DQ_HD inline bool float_equal(F x, F y) {
  return x == y || (x != x && y != y);  // (== holds for -0.0 and 0.0; a NaN is unequal to itself)
}

// Row i of a <=> row j of b.  The two columns have one type (the callers check it).
DQ_HD inline bool cell_equal(const Cells& a, int64_t i, const Cells& b, int64_t j) {
  const bool an = is_null(a, i), bn = is_null(b, j);
  if (an || bn) return an && bn;
  const int64_t ia = a.offset + i, jb = b.offset + j;
  switch (a.type & 0xff) {
    case T_BOOL:
      return bit_at(static_cast<const uint8_t*>(a.values), ia) == bit_at(static_cast<const uint8_t*>(b.values), jb);
    case T_INT8:
      return static_cast<const uint8_t*>(a.values)[ia] == static_cast<const uint8_t*>(b.values)[jb];
    case T_INT16:
      return static_cast<const uint16_t*>(a.values)[ia] == static_cast<const uint16_t*>(b.values)[jb];
    case T_INT32:
      return static_cast<const uint32_t*>(a.values)[ia] == static_cast<const uint32_t*>(b.values)[jb];
    case T_INT64:
      return static_cast<const uint64_t*>(a.values)[ia] == static_cast<const uint64_t*>(b.values)[jb];
    case T_FLOAT32:
      return float_equal(static_cast<const float*>(a.values)[ia], static_cast<const float*>(b.values)[jb]);
    case T_FLOAT64:
      return float_equal(static_cast<const double*>(a.values)[ia], static_cast<const double*>(b.values)[jb]);
    case T_DECIMAL128: {
      const uint64_t* x = static_cast<const uint64_t*>(a.values) + 2 * ia;
      const uint64_t* y = static_cast<const uint64_t*>(b.values) + 2 * jb;
      return x[0] == y[0] && x[1] == y[1];
    }
    case T_UTF8: {
      const int32_t ab = a.offsets[ia], ae = a.offsets[ia + 1];
      const int32_t bb = b.offsets[jb], be = b.offsets[jb + 1];
      if (ae - ab != be - bb) return false;
      return bytes_equal(static_cast<const uint8_t*>(a.values) + ab, static_cast<const uint8_t*>(b.values) + bb,
                         (uint32_t)(ae - ab));
    }
    default:
      return false;
  }
}

}  // namespace celleq
}  // namespace dq
