// dq_schema.h -- RowLevelSchemaValidator (schema/RowLevelSchemaValidator.scala:183-281): the
// per-cell tests of an int and a decimal definition, shared by the gfx950 evaluate kernel
// (dq_schema.hip), the host build behind dq_diag_schema_cell and tools/schema_check.cpp; and the
// structures the host planner (dq_schema_api.inc) hands the kernels.  Internal, not ABI.
//
// Int (Spark 2.2.2 Cast(StringType -> IntegerType) = UTF8String.toInt): optional sign, digits,
// optionally '.' and digits (validated, dropped); no trimming; NULL outside [-2^31, 2^31).
// Decimal (Cast(StringType -> DecimalType(p, s))): new java.math.BigDecimal(text), then
// setScale(s, ROUND_HALF_UP), NULL when the result's precision exceeds p.  For p <= 18 that needs no
// big integer: the digits kept at scale s, plus the rounding carry, either stay below 10^p (a
// uint64) or the cell is NULL.
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
namespace schema {

constexpr int kMaxDecimalPrecision = 18;   // 10^18 < 2^63: unscaled values are int64
constexpr int kMaxDecimalExponent = 1000;  // |exponent| above it: the cell is declined, not judged
constexpr uint64_t kPow10_18 = 1000000000000000000ull;

enum CellResult : int32_t { CELL_INVALID = 0, CELL_VALID = 1, CELL_UNSUPPORTED = 2 };

DQ_HD inline uint64_t pow10_u64(int p) {  // p <= 19
  uint64_t v = 1;
  for (int i = 0; i < p; ++i) v *= 10u;
  return v;
}

// UTF8String.toInt.  p[i] for 0 <= i < n only.
template <typename Src>
DQ_HD inline bool parse_int32(const Src& p, int32_t n, int32_t* out) {
  if (n <= 0) return false;
  int32_t i = 0;
  const uint32_t first = p[0];
  const bool neg = first == '-';
  if (neg || first == '+') {
    if (n == 1) return false;
    i = 1;
  }
  int64_t r = 0;  // accumulated negatively, as the reference does, so -2^31 parses
  for (; i < n; ++i) {
    const uint32_t b = p[i];
    if (b == '.') {
      ++i;
      break;
    }
    if (b - '0' >= 10u) return false;
    r = r * 10 - (int64_t)(b - '0');  // r >= -2^31 before the step: no int64 overflow
    if (r < -2147483648ll) return false;
  }
  for (; i < n; ++i)
    if ((uint32_t)p[i] - '0' >= 10u) return false;
  if (!neg) {
    if (r == -2147483648ll) return false;  // 2147483648 does not fit
    r = -r;
  }
  *out = (int32_t)r;
  return true;
}

// new BigDecimal(text).setScale(scale, ROUND_HALF_UP) with precision <= `precision` (<= 18).
// CELL_VALID: *out = the unscaled value.  CELL_UNSUPPORTED: a byte >= 0x80 (Java takes any Unicode
// digit) or a well-formed number whose exponent exceeds kMaxDecimalExponent in magnitude.
// Grammar: [+-] digits [. digits] | [+-] . digits, then optionally [eE] [+-] digits; nothing else.
template <typename Src>
DQ_HD inline int32_t parse_decimal(const Src& p, int32_t n, int32_t precision, int32_t scale, int64_t* out) {
  for (int32_t i = 0; i < n; ++i)
    if ((uint32_t)p[i] >= 0x80u) return CELL_UNSUPPORTED;
  if (n <= 0) return CELL_INVALID;
  int32_t i = 0;
  const uint32_t first = p[0];
  const bool neg = first == '-';
  if (neg || first == '+') i = 1;
  const int32_t digits_at = i;
  int32_t nd = 0, ip = -1;  // digits in all; digits before the point
  for (; i < n; ++i) {
    const uint32_t b = p[i];
    if (b - '0' < 10u) {
      ++nd;
    } else if (b == '.') {
      if (ip >= 0) return CELL_INVALID;
      ip = nd;
    } else if (b == 'e' || b == 'E') {
      break;
    } else {
      return CELL_INVALID;
    }
  }
  if (nd == 0) return CELL_INVALID;
  if (ip < 0) ip = nd;
  int64_t ex = 0;
  if (i < n) {  // the exponent
    ++i;
    bool eneg = false;
    if (i < n && (p[i] == '-' || p[i] == '+')) {
      eneg = p[i] == '-';
      ++i;
    }
    if (i >= n) return CELL_INVALID;
    for (; i < n; ++i) {
      const uint32_t b = p[i];
      if (b - '0' >= 10u) return CELL_INVALID;
      if (ex <= kMaxDecimalExponent) ex = ex * 10 + (int64_t)(b - '0');
    }
    if (ex > kMaxDecimalExponent) return CELL_UNSUPPORTED;
    if (eneg) ex = -ex;
  }
  // the first `keep` digits are the unscaled value; digit `keep` decides the rounding
  const int64_t keep = (int64_t)ip + ex + (int64_t)scale;
  uint64_t acc = 0;
  bool sat = false;
  uint32_t round = 0;
  int64_t j = 0;
  for (int32_t k = digits_at; j < nd && j <= keep; ++k) {
    const uint32_t b = p[k];
    if (b == '.') continue;
    const uint32_t dgt = b - '0';
    if (j < keep) {
      if (acc >= kPow10_18) sat = true;
      else acc = acc * 10u + dgt;
    } else {
      round = dgt >= 5u ? 1u : 0u;
    }
    ++j;
  }
  for (int64_t z = nd; z < keep && acc != 0 && !sat; ++z) {  // zeros the scale appends
    if (acc >= kPow10_18) sat = true;
    else acc *= 10u;
  }
  acc += round;
  if (sat || acc >= pow10_u64(precision)) return CELL_INVALID;
  *out = neg ? -(int64_t)acc : (int64_t)acc;
  return CELL_VALID;
}

// ---------------------------------------------------------------- planner <-> kernels
enum DefKind : int32_t { DEF_STRING = 0, DEF_INT = 1, DEF_DECIMAL = 2 };
enum DefFlags : int32_t {
  DF_NOT_NULL = 1,   // isNullable = false
  DF_MIN = 2,        // int: minValue (the conjunct that is NULL for a NULL cell, line 246); string: minLength
  DF_MAX = 4,        // int: maxValue; string: maxLength
  DF_MATCH = 8       // string: matches (the DFA image at dfas + dfa_off)
};

// One input column as the kernels address it.  Row r of the batch is bit `bit_offset + r` of
// validity (and of a bool column's values), element r of fixed-width `values` (already advanced),
// and the bytes values[offsets[r] - heap_base .. offsets[r + 1] - heap_base) of a utf8 column
// (offsets already advanced; heap_base != 0 when only the batch's slice of the heap was uploaded).
struct DevCol {
  const uint8_t* validity;  // nullptr = all valid
  const void* values;
  const int32_t* offsets;
  int64_t bit_offset;
  int32_t type;
  int32_t heap_base;
};

struct DevDef {
  int32_t column;
  int32_t kind;
  int32_t flags;
  int32_t precision, scale;
  int32_t lo, hi;
  uint32_t dfa_off;
  int64_t scratch_off;  // int / decimal: byte offset of the dense parsed column in the scratch area
};

}  // namespace schema
}  // namespace dq
