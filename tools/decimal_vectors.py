#!/usr/bin/env python3
"""Writes the vectors tools/decimal_check.cpp checks under the host sanitizers: the cast cases of
tests/decimal_cases.py with the answers of Python's exact arithmetic, one per line:

    scale lo hi double-bits toByteArray-hex

lo / hi = the two 64-bit words of the two's-complement unscaled value, double-bits = the IEEE bits
of float(Fraction(unscaled, 10^scale)), all in hexadecimal.

    python tools/decimal_vectors.py /tmp/decimal_vectors.txt
"""
import os
import struct
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import decimal_cases as C  # noqa: E402


def main(path):
    cases = C.cast_cases(seed=7, n_random=20000)
    with open(path, "w", encoding="ascii") as f:
        for _p, s, u in cases:
            w = u & C.MASK128
            bits = struct.unpack("<Q", struct.pack("<d", C.exact_double(u, s)))[0]
            f.write("%d %x %x %x %s\n" % (s, w & 0xFFFFFFFFFFFFFFFF, w >> 64, bits, C.to_byte_array(u).hex()))
    print("wrote %d vectors to %s" % (len(cases), path))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "decimal_vectors.txt")
