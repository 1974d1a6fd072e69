#!/usr/bin/env python3
"""Writes the vectors tools/schema_check.cpp checks under the host sanitizers: the hostile and
generated cells of tests/schema_cases.py with the answers of its Python restatement, one per line:

    kind precision scale result value hex-of-the-text

kind 1 = int (UTF8String.toInt), 2 = decimal; result 0 = the cast is NULL, 1 = value, 2 = declined.

    python tools/schema_vectors.py /tmp/schema_vectors.txt
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import schema_cases as S  # noqa: E402


def main(path):
    cells = S.HOSTILE_NUMBERS + S.HOSTILE_DECLINED + S.MULTIBYTE_TEXT + S.random_numbers(20000, np.random.default_rng(7))
    n = 0
    with open(path, "w", encoding="ascii") as f:
        for k, text in enumerate(cells):
            hx = text.encode("utf-8").hex()
            v = S.int_cell(text)
            f.write("1 0 0 %d %d %s\n" % ((0, 0, hx) if v is None else (1, v, hx)))
            types = S.DECIMAL_TYPES if k < 400 else [S.DECIMAL_TYPES[k % len(S.DECIMAL_TYPES)]]
            for p, s in types:
                v = S.decimal_cell(text, p, s)
                f.write("2 %d %d %d %d %s\n" % ((p, s) + ((2, 0) if v == S.DECLINE else (0, 0) if v is None else (1, v))
                                                + (hx,)))
                n += 1
            n += 1
    print("wrote %d vectors to %s" % (n, path))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "schema_vectors.txt")
