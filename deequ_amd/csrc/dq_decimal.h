// dq_decimal.h -- arithmetic on Spark DecimalType(p, s) values held as Arrow decimal128 (the
// 128-bit two's-complement unscaled value), as a host + device header: the decimal scan
// (dq_scan_dec.hip), the cast kernel behind dq_cast_decimal and the host side of dq_plan_finish run
// the same source; a host build is checked against Python's exact rationals on CPU (tests/).
//
//   * to_double: Spark 2.2.2 Cast(DecimalType -> DoubleType) = Decimal.toDouble =
//     java.math.BigDecimal.doubleValue: the correctly rounded (ties to even) value of
//     unscaled / 10^scale.  Three tiers, each exact:
//       1. |u| < 2^53 and scale <= 22: (double)u / 10^scale, one IEEE divide of two exact doubles;
//       2. |u| < 2^64: Eisel-Lemire over the 128-bit power-of-five table (dq_numparse.h), always
//          correct for an exact significand;
//       3. otherwise the quotient floor(u 2^k / 10^scale) to at least 56 bits by binary long
//          division plus a sticky bit for the remainder, rounded half-even.
//   * byte_length / be_stream: java.math.BigInteger.toByteArray of the unscaled value, the bytes
//     Spark's XxHash64Function hashes for a decimal of precision > 18 (InterpretedHashFunction).
// Internal, not ABI.
#pragma once

#include <cstdint>

#include "dq_numparse.h"

namespace dq {
namespace dec {

typedef unsigned __int128 u128;
typedef __int128 i128;

constexpr int kMaxPrecision = 38;

constexpr uint64_t kPow10U64[20] = {1ull,
                                    10ull,
                                    100ull,
                                    1000ull,
                                    10000ull,
                                    100000ull,
                                    1000000ull,
                                    10000000ull,
                                    100000000ull,
                                    1000000000ull,
                                    10000000000ull,
                                    100000000000ull,
                                    1000000000000ull,
                                    10000000000000ull,
                                    100000000000000ull,
                                    1000000000000000ull,
                                    10000000000000000ull,
                                    100000000000000000ull,
                                    1000000000000000000ull,
                                    10000000000000000000ull};

// 10^s, 0 <= s <= 38 (10^38 < 2^127)
DQ_HD inline u128 pow10_u128(int s) {
  return s <= 19 ? (u128)kPow10U64[s] : (u128)kPow10U64[19] * (u128)kPow10U64[s - 19];
}

DQ_HD inline u128 make_u128(uint64_t lo, uint64_t hi) { return ((u128)hi << 64) | (u128)lo; }

// bits of v (0 for 0)
DQ_HD inline int bit_length(u128 v) {
  const uint64_t hi = (uint64_t)(v >> 64);
  return hi ? 128 - numparse::clz64(hi) : 64 - numparse::clz64((uint64_t)v);
}

// |v| of a signed 128-bit value (2^127 for the minimum)
DQ_HD inline u128 magnitude(uint64_t lo, int64_t hi) {
  const u128 v = make_u128(lo, (uint64_t)hi);
  return hi < 0 ? (u128)0 - v : v;
}

// q 2^-k rounded to nearest, ties to even, as IEEE bits; `sticky`: the true value lies strictly
// above q 2^-k (by less than 2^-k).  q != 0; with sticky, q has at least 55 bits.
DQ_HD inline uint64_t round_bits(u128 q, bool sticky, int k) {
  const int sh = bit_length(q) - 53;
  uint64_t mant;
  if (sh <= 0) {
    mant = (uint64_t)(q << (-sh));  // exact
  } else {
    mant = (uint64_t)(q >> sh);
    const u128 rem = q & (((u128)1 << sh) - 1);
    const u128 half = (u128)1 << (sh - 1);
    if (rem > half || (rem == half && (sticky || (mant & 1ull)))) ++mant;
  }
  // mant in [2^52, 2^53] times 2^(sh - k): bit 52 of mant carries into the exponent field
  return ((uint64_t)(1023 + 52 + sh - k - 1) << 52) + mant;
}

// tier 3: mag / 10^scale for mag != 0, 1 <= scale <= 38
DQ_HD_NOINLINE inline uint64_t divide_bits(u128 mag, int scale) {
  const u128 d = pow10_u128(scale);
  const int bu = bit_length(mag), bd = bit_length(d);  // bd >= 4
  const int nb = bu > 56 + bd ? bu : 56 + bd;          // bits of the numerator N = mag << k
  const int k = nb - bu;
  const int t = nb - (bd - 1);  // quotient bits to produce (>= 57); the first bd - 1 bits of N give none
  const int a = t - k;          // = bu - bd + 1, in [-126, 125]
  u128 rem = a >= 0 ? (mag >> a) : (mag << (-a));  // N >> t < 2^(bd - 1) <= d
  u128 q = 0;
  for (int i = t - 1; i >= 0; --i) {
    const uint32_t bit = i >= k ? (uint32_t)(mag >> (i - k)) & 1u : 0u;
    rem = (rem << 1) | bit;  // < 2 d < 2^128
    q <<= 1;
    if (rem >= d) {
      rem -= d;
      q |= 1;
    }
  }
  return round_bits(q, rem != 0, k);
}

// tier of a magnitude at a scale: 1 divide, 2 Eisel-Lemire, 3 long division
DQ_HD inline int tier_of(u128 mag, int scale) {
  if ((mag >> 53) == 0 && scale <= 22) return 1;
  return (mag >> 64) == 0 ? 2 : 3;
}

// the tiers 2 and 3 (mag != 0)
DQ_HD inline double to_double_slow(u128 mag, int scale, bool neg) {
  uint64_t bits;
  if ((mag >> 64) == 0) {
    bits = numparse::adjusted_bits(numparse::eisel_lemire(-(int64_t)scale, (uint64_t)mag));
  } else if (scale == 0) {
    bits = round_bits(mag, false, 0);  // an integer: one rounding of its bits
  } else {
    bits = divide_bits(mag, scale);
  }
  return numparse::bits_double(bits | (neg ? 0x8000000000000000ull : 0ull));
}

DQ_HD inline double to_double_fast(u128 mag, int scale, bool neg) {  // tier 1 (also 0)
  const double v = (double)(uint64_t)mag / numparse::kPow10Exact[scale];
  return neg ? -v : v;
}

DQ_HD inline double to_double(uint64_t lo, int64_t hi, int scale) {
  const u128 mag = magnitude(lo, hi);
  if (tier_of(mag, scale) == 1) return to_double_fast(mag, scale, hi < 0);
  return to_double_slow(mag, scale, hi < 0);
}

// java.math.BigInteger.toByteArray().length: bitLength / 8 + 1, bitLength of a negative v that of ~v
DQ_HD inline int byte_length(uint64_t lo, int64_t hi) {
  const u128 v = make_u128(lo, (uint64_t)hi);
  return bit_length(hi < 0 ? ~v : v) / 8 + 1;
}

DQ_HD inline uint64_t bswap64(uint64_t x) { return __builtin_bswap64(x); }

// toByteArray as a byte stream packed little-endian into 128 bits: stream byte j (the value's
// big-endian byte j of `len`) sits at bits [8 j, 8 j + 8).
DQ_HD inline u128 be_stream(uint64_t lo, int64_t hi, int len) {
  const u128 all = make_u128(bswap64((uint64_t)hi), bswap64(lo));  // the 16-byte big-endian stream
  return all >> (8 * (16 - len));
}

}  // namespace dec
}  // namespace dq
