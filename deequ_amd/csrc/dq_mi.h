// dq_mi.h -- the parts of MutualInformation (MutualInformation.scala:38-81) that the kernels
// (dq_freq.hip "MutualInformation"), the host side of dq_freq_mutual_information and the host
// checks (dq_diag_mi_*, tools/mi_check.cpp, tests/) run from one source, as a host + device header:
//
//   * split: a joint group key of two key columns -> the two fields' offsets and lengths.  The
//     encoding is the table's (deequ_amd.h): a fixed-width value as its little-endian bytes, a
//     string part of a composite key as a u32 length and its UTF-8 bytes.  A field is re-encoded
//     as a single-column key by taking its bytes alone (a string without its length prefix).
//     A key that does not split exactly -- a length prefix running past the key, a truncated
//     fixed field, bytes left over -- is refused, and no byte at or past `len` is read.
//   * to_fixed: one term of the sum as a signed 128-bit integer with 96 fraction bits,
//     round(|t| 2^96) with ties to even, the sign put back after rounding (so to_fixed(-t) =
//     -to_fixed(t)).  A term is a double, i.e. m 2^e with m < 2^53: for e >= -96 the conversion
//     is exact, below it drops bits under 2^-96 by that one rule (|error| <= 2^-97).  Terms that
//     are not finite or not below 2^6 in magnitude are refused (the sum of |term| over a state
//     whose counts sum to at most numRows is below ln(2^63) < 2^6, so 128 bits never overflow).
//   * from_fixed: the 128-bit sum back to the nearest double (ties to even), exact for every
//     value: at most one rounding between the integer sum and the metric.
// Integer sums of fixed-point terms do not depend on their order, which is what lets the metric
// of a merged state equal that of the union bit for bit.  Internal, not ABI.
#pragma once

#include <cstdint>

#ifndef DQ_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define DQ_HD __host__ __device__
#else
#define DQ_HD
#endif
#endif

namespace dq {
namespace mi {

typedef unsigned __int128 u128;
typedef __int128 i128;

constexpr int kFracBits = 96;
constexpr int kTypeUtf8 = 8;  // DQ_T_UTF8 (deequ_amd.h; checked where both are visible)

struct Split {
  uint32_t off_a, len_a, off_b, len_b;
};

// Width of a fixed-width key type (DQ_T_BOOL .. DQ_T_FLOAT64), 0 for any other type.
DQ_HD inline uint32_t fixed_width(int type) {
  switch (type) {
    case 1: case 2: return 1u;  // bool, int8
    case 3: return 2u;          // int16
    case 4: case 6: return 4u;  // int32, float32
    case 5: case 7: return 8u;  // int64, float64
    default: return 0u;
  }
}

// One field starting at `pos`: false when it does not fit in key[0 .. len).  Src::u32(off) reads
// the little-endian u32 at key bytes off .. off + 3 and is only called with off + 4 <= len.
template <class Src>
DQ_HD inline bool field(const Src& key, uint32_t len, int type, uint32_t& pos, uint32_t& off, uint32_t& n) {
  if (type == kTypeUtf8) {
    if (len - pos < 4u) return false;
    const uint32_t sl = key.u32(pos);
    pos += 4u;
    if (sl > len - pos) return false;
    off = pos;
    n = sl;
    pos += sl;
    return true;
  }
  const uint32_t w = fixed_width(type);
  if (w == 0u || len - pos < w) return false;
  off = pos;
  n = w;
  pos += w;
  return true;
}

template <class Src>
DQ_HD inline bool split(const Src& key, uint32_t len, int type_a, int type_b, Split* out) {
  uint32_t pos = 0u;
  Split s{};
  if (!field(key, len, type_a, pos, s.off_a, s.len_a)) return false;
  if (!field(key, len, type_b, pos, s.off_b, s.len_b)) return false;
  if (pos != len) return false;
  *out = s;
  return true;
}

DQ_HD inline uint64_t double_bits(double d) {
  union {
    double d;
    uint64_t u;
  } v;
  v.d = d;
  return v.u;
}

DQ_HD inline double bits_to_double(uint64_t u) {
  union {
    double d;
    uint64_t u;
  } v;
  v.u = u;
  return v.d;
}

// q >> k rounded to nearest, ties to even (k >= 1).
DQ_HD inline u128 shr_rne(u128 q, int k) {
  if (k > 127) return 0;  // q < 2^127: below half a unit
  const u128 fl = q >> k;
  const u128 rem = q & ((((u128)1) << k) - 1);
  const u128 half = ((u128)1) << (k - 1);
  if (rem > half || (rem == half && (fl & 1))) return fl + 1;
  return fl;
}

// false: t is NaN, infinite or |t| >= 2^6 (the caller's flag word carries that, never the sum).
DQ_HD inline bool to_fixed(double t, i128* out) {
  const uint64_t b = double_bits(t);
  const int be = (int)((b >> 52) & 0x7FFu);
  if (be >= 1023 + 6) return false;  // |t| >= 2^6, infinities and NaNs
  uint64_t m = b & 0xFFFFFFFFFFFFFull;
  int e;  // |t| = m 2^e
  if (be == 0) {
    e = -1074;
  } else {
    m |= 1ull << 52;
    e = be - 1075;
  }
  const int sh = e + kFracBits;  // <= 5 - 52 + 96 = 49
  const u128 mag = sh >= 0 ? ((u128)m) << sh : shr_rne((u128)m, -sh);
  *out = (b >> 63) ? -(i128)mag : (i128)mag;
  return true;
}

// The nearest double (ties to even) of v / 2^96.
DQ_HD inline double from_fixed(i128 v) {
  if (v == 0) return 0.0;
  const bool neg = v < 0;
  const u128 mag = neg ? (u128)0 - (u128)v : (u128)v;
  const uint64_t hi = (uint64_t)(mag >> 64), lo = (uint64_t)mag;
  const int n = hi ? 128 - __builtin_clzll(hi) : 64 - __builtin_clzll(lo);  // bit length
  u128 sig = mag;
  int e = -kFracBits;  // value = sig 2^e
  if (n > 53) {
    sig = shr_rne(mag, n - 53);
    e += n - 53;
    if (sig >> 53) {  // rounded up to 2^53
      sig >>= 1;
      e += 1;
    }
  }
  // sig < 2^53 is exact as a double; its power-of-two scaling stays normal (2^-96 <= |value| < 2^32)
  uint64_t s = (uint64_t)sig;
  int k = 0;
  while (!(s >> 52)) {
    s <<= 1;
    ++k;
  }
  const uint64_t bits = ((uint64_t)neg << 63) | ((uint64_t)(e - k + 52 + 1023) << 52) | (s & 0xFFFFFFFFFFFFFull);
  return bits_to_double(bits);
}

}  // namespace mi
}  // namespace dq
