"""Shared by the RowLevelSchemaValidator tests (test_schema.py, test_gpu_schema.py): the reference's
known answers, a small Python restatement of the semantics (RowLevelSchemaValidator.scala:225-281
under Spark 2.2.2), and generators of hostile cells.  Test infrastructure: the product never imports it.

The restatement is a Kleene AND over per-cell tests.  Int cells: the oracle's UTF8String.toLong
narrowed to 32 bits.  Decimal cells: an ASCII grammar checked with `re` FIRST (Python's Decimal()
strips blanks and takes NaN, Infinity and '_'), then decimal.Decimal.quantize(ROUND_HALF_UP).
Lengths: the oracle's utf8_num_chars.  Patterns: pattern_cases.oracle."""
import decimal
import functools
import json
import os
import re
from collections import OrderedDict

import numpy as np

import pyoracle as O
import pattern_cases as P

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DECLINE = "decline"   # decimal_cell: the GPU must decline the cell
MAX_EXPONENT = 1000


def known_answers():
    with open(os.path.join(GOLDEN, "schema_known_answers.json"), encoding="utf-8") as f:
        return json.load(f)["cases"]


# ---------------------------------------------------------------- per-cell tests
@functools.lru_cache(maxsize=None)
def int_cell(text):
    """UTF8String.toInt: the value, or None (the cast is NULL)."""
    v = O.spark_string_to_long(text)
    return v if v is not None and -(1 << 31) <= v < (1 << 31) else None


_DEC = re.compile(r"[+-]?(?:[0-9]+\.?[0-9]*|\.[0-9]+)(?:[eE]([+-]?[0-9]+))?\Z")


@functools.lru_cache(maxsize=None)
def decimal_cell(text, precision, scale):
    """new java.math.BigDecimal(text).setScale(scale, ROUND_HALF_UP) within `precision` digits: the
    unscaled value, None (the cast is NULL), or DECLINE."""
    if any(c >= 0x80 for c in text.encode("utf-8")):
        return DECLINE
    m = _DEC.match(text)
    if m is None:
        return None
    if m.group(1) is not None and abs(int(m.group(1))) > MAX_EXPONENT:
        return DECLINE
    with decimal.localcontext() as ctx:
        ctx.prec = 5000
        ctx.Emax = decimal.MAX_EMAX
        ctx.Emin = decimal.MIN_EMIN
        q = decimal.Decimal(text).quantize(decimal.Decimal(1).scaleb(-scale), rounding=decimal.ROUND_HALF_UP)
        unscaled = int(q.scaleb(scale))
    return unscaled if abs(unscaled) < 10 ** precision else None


# ---------------------------------------------------------------- Kleene logic (None = NULL)
def k_or(a, b):
    if a is True or b is True:
        return True
    return None if a is None or b is None else False


def k_and_all(values):
    if any(v is False for v in values):
        return False
    return None if any(v is None for v in values) else True


def conjuncts(defn, cell):
    """The conjuncts one definition adds for one cell (None = NULL cell); DECLINE among them when a
    decimal cell must be declined."""
    kind = defn["kind"]
    is_null = cell is None
    out = []
    if not defn.get("isNullable", True):
        out.append(not is_null)
    if kind == "int":
        cast = None if is_null else int_cell(cell)
        out.append(k_or(is_null, cast is not None))
        if defn.get("minValue") is not None:  # line 246: colIsNull.isNull is always FALSE
            out.append(k_or(False, None if cast is None else cast >= defn["minValue"]))
        if defn.get("maxValue") is not None:
            out.append(k_or(is_null, None if cast is None else cast <= defn["maxValue"]))
    elif kind == "decimal":
        cast = None if is_null else decimal_cell(cell, defn["precision"], defn["scale"])
        out.append(DECLINE if cast == DECLINE else k_or(is_null, cast is not None))
    elif kind == "string":
        length = None if is_null else O.utf8_num_chars(cell.encode("utf-8"))
        if defn.get("minLength") is not None:
            out.append(k_or(is_null, None if length is None else length >= defn["minLength"]))
        if defn.get("maxLength") is not None:
            out.append(k_or(is_null, None if length is None else length <= defn["maxLength"]))
        if defn.get("matches") is not None:
            out.append(k_or(is_null, None if is_null else P.oracle(defn["matches"], cell) == 1))
    else:
        raise ValueError("the restatement has no %s columns" % kind)
    return out


class Mirror:
    pass


def mirror(columns, defs):
    """columns: OrderedDict name -> (dtype, values); defs: the builder calls as dicts, in order."""
    names = list(columns)
    n = len(next(iter(columns.values()))[1]) if names else 0
    res = Mirror()
    res.valid_idx, res.invalid_idx, res.null_idx, res.declined = [], [], [], []
    memo = {}  # (definition, cell) -> conjuncts: large tables repeat their cells
    for r in range(n):
        cs = []
        for k, dn in enumerate(defs):
            cell = columns[dn["name"]][1][r]
            c = memo.get((k, cell))
            if c is None:
                c = memo[(k, cell)] = conjuncts(dn, cell)
            if DECLINE in c and dn["name"] not in res.declined:
                res.declined.append(dn["name"])
            cs += c
        verdict = k_and_all([c for c in cs if c != DECLINE])
        (res.valid_idx if verdict is True else res.invalid_idx if verdict is False else res.null_idx).append(r)
    last = {dn["name"]: dn for dn in defs}  # castExpressions.toMap
    res.decimals = {c: (last[c]["precision"], last[c]["scale"]) for c in names
                    if c in last and last[c]["kind"] == "decimal"}
    res.valid_cols, res.invalid_cols = OrderedDict(), OrderedDict()
    for c in names:
        dtype, values = columns[c]
        res.invalid_cols[c] = (dtype, [values[r] for r in res.invalid_idx])
        picked = [values[r] for r in res.valid_idx]
        dn = last.get(c)
        if dn is not None and dn["kind"] == "int":
            res.valid_cols[c] = ("int32", [None if v is None else int_cell(v) for v in picked])
        elif dn is not None and dn["kind"] == "decimal" and not res.declined:
            res.valid_cols[c] = ("int64", [None if v is None else decimal_cell(v, dn["precision"], dn["scale"])
                                           for v in picked])
        else:
            res.valid_cols[c] = (dtype, picked)
    return res


def build_schema(defs):
    import deequ_amd as d
    s = d.RowLevelSchema()
    for dn in defs:
        kw = {k: v for k, v in dn.items() if k not in ("kind", "name")}
        s = {"int": s.withIntColumn, "decimal": s.withDecimalColumn, "string": s.withStringColumn,
             "timestamp": s.withTimestampColumn}[dn["kind"]](dn["name"], **kw)
    return s


# ---------------------------------------------------------------- hostile cells
HOSTILE_NUMBERS = [
    ".", "+", "-", "1.", ".5", "1.9", "2147483647", "2147483648", "-2147483648", "-2147483649", " 1", "1 ",
    "99.995", "9.995", "99.994", "9.994", "0.005", "-0.005", "0.004", "-0.004", "1e2", "1E-3", "1e", "e1", "1e+",
    "1e-", "1e+2", "1.e2", ".e2", "+.5", "-.5", "+.", "-.", "..", "1..2", "1.2.3", "0" * 40 + "7",
    "0" * 40 + "7.5", "0." + "3" * 30, "1." + "0" * 30, "", "0", "-0", "+0", "00", "0.0", "-0.0", "1e0", "0e0",
    "0e999", "0e-999", "1e1000", "1e-1000", "123456789012345678", "1234567890123456789", "999999999999999999.5",
    "99999999.994", "99999999.995", "-99999999.995", "0.994999999999999999999999", "0.995000000000000000000001",
    "12e-1", "125e-1", "125e-3", "5e-3", "4e-3", "5e-4", "100e-2", "1_0", "NaN", "Infinity", "-Infinity", "inf",
    "1d", "1f", "0x10", "١٢٣", "1 ", "12\n", "\n12", "+-1", "--1", "1-", "1+", "9" * 19, "9" * 18, "-" + "9" * 18,
    "4.5", "5.5", "-4.5", "0.5", "-0.5", "0.49", "1e5", "1e17", "1e18", "1.5e1", "15e-1", "000", "-", "+1.", "1.e",
    "2147483647.999", "-2147483648.999", "2147483648.0", "1.a", "1.5a", "a", "1e0000000000000002", "1e00000000001001",
]
HOSTILE_DECLINED = ["1e5000", "1e-5000", "1é", "é", "１２", "1e1001", "0e1001", "12ée2"]
MULTIBYTE_TEXT = ["", "a", "é", "ab", "éé", "日本", "日本語", "😀", "a😀", "a😀b", "ñandú", "ñandú€", "abcd", "abcde",
                  "日本語日", "😀😀😀", "éééé", "ééééé", "x" * 15 + "é", "x" * 16 + "é", "é" * 8 + "zz"]
DECIMAL_TYPES = [(4, 2), (10, 2), (18, 0), (18, 18), (1, 0), (1, 1), (5, 5), (9, 3), (18, 6)]


def random_numbers(n, rng):
    """n cells: well-formed numbers of every shape, near-misses, and noise."""
    out = []
    alphabet = "0123456789+-.eE 9"
    for _ in range(n):
        kind = int(rng.integers(6))
        if kind == 0:  # noise over the numeric alphabet
            out.append("".join(alphabet[int(i)] for i in rng.integers(len(alphabet), size=int(rng.integers(0, 9)))))
            continue
        if kind == 1:  # around the 32-bit bounds
            out.append(str(int(rng.choice([-(1 << 31), (1 << 31) - 1, 0])) + int(rng.integers(-3, 4))))
            continue
        sign = ["", "", "+", "-"][int(rng.integers(4))]
        ni = int(rng.integers(0, 12)) if kind != 5 else int(rng.integers(15, 25))
        nf = int(rng.integers(0, 8)) if kind != 5 else int(rng.integers(0, 25))
        digits = lambda k: "".join(str(int(x)) for x in rng.integers(10, size=k))  # noqa: E731
        s = sign + digits(ni)
        if nf or rng.random() < 0.2:
            s += "." + digits(nf)
        if kind >= 3 and rng.random() < 0.6:
            s += "eE"[int(rng.integers(2))] + ["", "+", "-"][int(rng.integers(3))] + str(int(rng.integers(0, 30)))
        if kind == 4 and s:  # one mutation
            i = int(rng.integers(len(s)))
            s = s[:i] + alphabet[int(rng.integers(len(alphabet)))] + s[i + (rng.random() < 0.5):]
        out.append(s)
    return out
