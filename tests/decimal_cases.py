"""Shared generators and exact references of the decimal-column tests (tests/test_decimal.py on
the CPU, tests/test_gpu_decimal.py on the GPU) and of tools/decimal_vectors.py.

The references are Python's own exact arithmetic, independent of the code under test:

* Cast(DecimalType(p, s) -> DoubleType) = java.math.BigDecimal.doubleValue, the correctly rounded
  value of unscaled / 10^s: `float(Fraction(u, 10 ** s))` (CPython rounds int / int half-even);
* sums, minima and maxima are Python ints, converted the same way once;
* Spark 2.2.2's XxHash64Function of a decimal (InterpretedHashFunction): hashLong(unscaled) when
  the column type's precision is <= 18, else XXH64 of BigInteger.toByteArray of the unscaled value.
"""
import random
import struct
from fractions import Fraction

import numpy as np

import pyoracle as O

MASK128 = (1 << 128) - 1


def exact_double(u: int, scale: int) -> float:
    return float(Fraction(u, 10 ** scale))


def to_byte_array(v: int) -> bytes:
    """java.math.BigInteger.toByteArray: minimal big-endian two's complement, length
    bitLength / 8 + 1 where bitLength of a negative v is that of ~v."""
    n = (~v if v < 0 else v).bit_length() // 8 + 1
    return (v & ((1 << (8 * n)) - 1)).to_bytes(n, "big")


def spark_hash(u: int, precision: int) -> int:
    if precision <= 18:
        return O.xxh64(struct.pack("<q", u), 42)
    return O.xxh64(to_byte_array(u), 42)


def hll_words(values, precision: int):
    """ApproxCountDistinctState words of the non-None unscaled values."""
    regs = [0] * 512
    for u in values:
        if u is None:
            continue
        idx, pw = O.hll_index_and_rank(spark_hash(u, precision))
        regs[idx] = max(regs[idx], pw)
    return O.hll_pack(regs)


def le_words(values):
    """(n, 2) uint64 array of the 16 little-endian bytes per row (None -> 0)."""
    out = np.zeros((len(values), 2), dtype=np.uint64)
    for i, u in enumerate(values):
        if u is not None:
            w = u & MASK128
            out[i, 0] = w & 0xFFFFFFFFFFFFFFFF
            out[i, 1] = w >> 64
    return out


def tie_values():
    """(unscaled, scale): exact ties of the cast, to be used with their neighbours u - 1, u + 1."""
    ties = [((2 ** 53 + 1) * 5 ** s, s) for s in (1, 10, 22)]
    ties.append((2 ** 100 + 2 ** 47, 0))
    ties.append(((2 ** 64 + 2 ** 11) * 5 ** 3, 3))
    return ties


def tie_cases():
    """(precision, scale, unscaled) around every tie, both signs; precision = the digits needed."""
    out = []
    for u, s in tie_values():
        for d in (-1, 0, 1):
            for sign in (1, -1):
                v = sign * (u + d)
                out.append((max(len(str(abs(v))), s, 1), s, v))
    return out


def tie_groups():
    """{(precision, scale): [unscaled, ...]}: the ties above with their neighbours and both signs,
    each group in the narrowest column type that holds it."""
    groups = {}
    for p, s, v in tie_cases():
        groups.setdefault(s, []).append((p, v))
    return {(max(p for p, _ in pv), s): [v for _, v in pv] for s, pv in groups.items()}


def tie_pool(precision: int, scale: int):
    """Exact ties of the cast that a decimal(precision, scale) column can hold, with their
    neighbours u +- 1 and both signs: (2^53 + 1 + 2k) 5^scale (a 54-bit odd numerator over 2^scale),
    its 2^11-fold (65 bits wide: the long-division tier, or the wide-integer rounding at scale 0), and
    at scale 0 2^100 + 2^47.  Empty when the type holds none: a tie needs 5^scale | u with a quotient
    of at least 54 bits, which decimal(9,2) and decimal(38,38) have no room for."""
    top = 10 ** precision - 1
    centres = [(2 ** 53 + 1 + 2 * k) * 5 ** scale for k in range(3)]
    centres += [c << 11 for c in centres]
    if scale == 0:
        centres.append(2 ** 100 + 2 ** 47)
    pool = []
    for c in centres:
        if c + 1 <= top:
            assert exact_double(c - 1, scale) < exact_double(c + 1, scale)  # (a tie: its neighbours differ)
            for d in (-1, 0, 1):
                pool += [c + d, -(c + d)]
    return pool


def cast_cases(seed: int = 7, n_random: int = 4000):
    """(precision, scale, unscaled): random values over every precision and scale with magnitudes
    of every bit length, +-(10^p - 1), 0 at every scale, and the ties with their neighbours."""
    rnd = random.Random(seed)
    out = []
    for p in range(1, 39):
        for u in (10 ** p - 1, -(10 ** p - 1)):
            for s in sorted({0, p // 2, p}):
                out.append((p, s, u))
    for s in range(0, 39):
        out.append((38, s, 0))
    out += tie_cases()
    for _ in range(n_random):
        p = rnd.randint(1, 38)
        s = rnd.randint(0, p)
        bits = rnd.randint(0, (10 ** p - 1).bit_length())
        u = rnd.getrandbits(bits) if bits else 0
        u = min(u, 10 ** p - 1)
        out.append((p, s, -u if rnd.random() < 0.5 else u))
    return out


def column_values(kind: str, n: int, precision: int, scale: int, seed: int = 11):
    """A column of unscaled values (None = NULL) of one of the GPU tests' kinds."""
    rnd = random.Random(seed * 1000003 + n * 131 + precision)
    top = 10 ** precision - 1
    if kind == "random":
        out = []
        for _ in range(n):
            if rnd.random() < 0.1:
                out.append(None)
                continue
            bits = rnd.randint(0, top.bit_length())
            u = min(rnd.getrandbits(bits) if bits else 0, top)
            out.append(-u if rnd.random() < 0.5 else u)
        return out
    if kind == "all_null":
        return [None] * n
    if kind == "null_runs":  # NULL runs that empty whole waves (64 rows) and more
        out = []
        for i in range(n):
            out.append(None if (i // 96) % 2 == 0 else rnd.randint(-top, top))
        return out
    if kind == "max":
        return [top] * n
    if kind == "min":
        return [-top] * n
    if kind == "alternating":  # sum 0 (even n) with a huge sum of |x|
        return [top if i % 2 == 0 else -top for i in range(n)]
    if kind == "ties":
        pool = tie_pool(precision, scale)
        if not pool:
            raise ValueError("decimal(%d,%d) holds no exact tie of the cast" % (precision, scale))
        # both signs, the positive values twice: a sign-symmetric column has a mean of exactly 0,
        # against which no relative bound can be met (that case is the "alternating" kind's)
        pool = pool + [v for v in pool if v > 0]
        return [pool[i % len(pool)] for i in range(n)]
    if kind == "byte_lengths":  # toByteArray lengths 1..16 (as far as the precision reaches)
        pool = []
        for nbytes in range(1, 17):
            for v in (1 << (8 * nbytes - 1)) - 1, -(1 << (8 * nbytes - 1)), 1 << (8 * nbytes - 9) if nbytes > 1 else 0:
                if abs(v) <= top:
                    pool.append(v)
        pool += [0, 128, -128, -129]
        pool = [v for v in pool if abs(v) <= top]
        return [pool[i % len(pool)] for i in range(n)]
    raise ValueError(kind)


KINDS = ("random", "all_null", "null_runs", "max", "min", "alternating", "ties", "byte_lengths")
