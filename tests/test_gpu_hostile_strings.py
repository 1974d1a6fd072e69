"""The string kernels over sliced utf8 columns in hostile buffers (tests/hostile.py), row by row.

A device utf8 column is used in place: `offsets + offset`, heap offsets that do not start at 0,
and a heap whose bytes before, between (NULL slots) and after the window's strings are digits /
0xFF 0x80 / text that would complete a literal.  The kernels load whole words or 16 / 24-byte
windows and mask; a wrong mask is invisible when the neighbours are zeros, and invisible in an
aggregate over thousands of rows.  Here every row is observable:

* ApproxCountDistinct over strings no two of which share an HLL register, so the words pin every
  row's hash: every (start mod 8, byte length 0..40), lengths 41..72, multi-byte UTF-8; through
  the HLL kernel, the fused string pass and DQ_NO_STRING_PASS=1;
* DataType over tables of one class each; Min / MaxLength over tables of one character count;
* Compliance with string literals and PatternMatch where the guard bytes would complete a match;
* the string -> long / double casts row by row; dq_profile_few_strings against Python counts;
* a whole ColumnProfiler run against the oracle's profile.

All bit-exact against the oracle, host and device resident, every flavour."""
import collections
import math
import struct
from fractions import Fraction

import numpy as np
import pytest

import deequ_amd as d
import hostile as H
import pattern_cases as C
import pyoracle as O
from deequ_amd.profiles import ColumnProfilerRunner, NumericColumnProfile, cast_string_column, cast_string_columns
from helpers import oracle_table
from test_gpu_parity import _check_state
from test_gpu_pattern_match import run_plan
from test_gpu_profile_few import _batched_few
from test_gpu_profiles import _spark_to_long

pytestmark = pytest.mark.gpu

matrix = pytest.mark.parametrize(
    "flavour,device", [(f, dev) for f in H.FLAVOURS for dev in (True, False)],
    ids=["%s-%s" % (f, "device" if dev else "host") for f in H.FLAVOURS for dev in (True, False)])
OFFSETS = (24, 61)  # validity in place at a byte address that is no multiple of 4; realigned
_DIGITS = "3141592653589793238462643383279502884197169399375105820974944592"


def _table(values, offset, flavour, device, name="s"):
    col = H.hostile_column("string", values, offset=offset, flavour=flavour, device=device)
    assert col.offset == offset and col.validity is not None
    return d.Table({name: col})


def _digits(ln, k):
    return (_DIGITS[k:] + _DIGITS)[:ln]


# ---------------------------------------------------------------- ApproxCountDistinct
_HLL = {}


def _hll_case():
    if not _HLL:
        values = H.distinct_register_strings()
        ot = oracle_table({"s": ["string", values]})
        _HLL.update(values=values, words=list(O.approx_count_distinct_state(ot, "s").words),
                    counts=tuple(O.datatype_state(ot, "s")))
    return _HLL["values"], _HLL["words"], _HLL["counts"]


@matrix
def test_hll_words_pin_every_row(gpu, monkeypatch, flavour, device):
    values, words, counts = _hll_case()
    acd, dt = d.ApproxCountDistinct("s"), d.DataType("s")
    tables = [_table(values, off, flavour, device) for off in OFFSETS]

    def check(fused_only=False):
        for t in tables:
            if not fused_only:
                assert list(d.run_scan([acd], t)[acd].words) == words   # dq_hll_kernel alone
            st = d.run_scan([acd, dt], t)
            assert list(st[acd].words) == words
            assert tuple(st[dt].counts()) == counts
    check()                                             # [acd, dt]: the fused string pass
    monkeypatch.setenv("DQ_NO_STRING_PASS", "1")        # [acd, dt]: one kernel each
    monkeypatch.setenv("DEEQU_AMD_PLAN_CACHE", "0")     # (a pooled plan keeps its kernels)
    check(fused_only=True)


# ---------------------------------------------------------------- DataType
def _fractional(ln, k):
    if ln == 0:
        return None
    p = k % ln
    return _digits(p, k) + "." + _digits(ln - 1 - p, k + 3)


def _integral(ln, k):
    return "-" + _digits(ln - 1, k) if (k % 3 == 1 and ln >= 2) else _digits(ln, k)


def _boolean(ln, k):
    return {4: "true", 5: "false"}.get(ln)


def _text(ln, k):
    return ("x" + "tru1.0e-5false "[k:] + "k" * ln)[:ln] if ln else None


CLASSES = [("fractional", 1, _fractional), ("integral", 2, _integral), ("boolean", 3, _boolean), ("string", 4, _text)]


@matrix
@pytest.mark.parametrize("name,position,make", CLASSES, ids=[c[0] for c in CLASSES])
def test_datatype_one_class_per_table(gpu, flavour, device, name, position, make):
    """Every valid row is of one DataType class: a single misread row moves a count."""
    # (short strings last: they start inside the final 24 bytes of the window's heap)
    values = H.residue_grid(make, extra=[s for s in (make(5, 0), make(4, 1), make(2, 2), make(1, 3)) if s is not None])
    ot = oracle_table({"s": ["string", values]})
    want = tuple(O.datatype_state(ot, "s"))
    n_valid = sum(v is not None for v in values)
    assert want[position] == n_valid and want[0] == len(values) - n_valid and n_valid >= 16
    dt, acd = d.DataType("s"), d.ApproxCountDistinct("s")
    for off in OFFSETS:
        t = _table(values, off, flavour, device)
        assert tuple(d.run_scan([dt], t)[dt].counts()) == want           # the DataType kernel alone
        st = d.run_scan([dt, acd], t)                                    # the fused string pass
        assert tuple(st[dt].counts()) == want
        assert list(st[acd].words) == list(O.approx_count_distinct_state(ot, "s").words)


# ---------------------------------------------------------------- MinLength / MaxLength
@matrix
@pytest.mark.parametrize("chars", [0, 1, 5, 16, 33])
def test_lengths_of_one_character_count(gpu, flavour, device, chars):
    """Valid strings of 1..4 bytes per character, all of `chars` characters: Min = Max = chars."""
    values = []
    for unit in ("a", "é", "日", "😀"):
        for k in range(8):
            values += [None, unit * chars]
    values.append(None)
    ot = oracle_table({"s": ["string", values]})
    an = [d.MinLength("s"), d.MaxLength("s")]
    for off in OFFSETS:
        st = d.run_scan(an, _table(values, off, flavour, device))
        for a in an:
            _check_state(a, st[a], ot)
        assert st[an[0]] == d.MinState(float(chars)) and st[an[1]] == d.MaxState(float(chars))


# ---------------------------------------------------------------- Compliance with literals
@matrix
def test_string_literals(gpu, flavour, device):
    """'k' followed by a NULL slot whose bytes read "1true0k" (or "9.e-"): equal to no longer literal."""
    unit = ["k", None, "k1", None, "k12", "k", None, "", None, "K1", "k1", None, "k1true0", None, "k19.e", None,
            "k1ÿ", None]
    values = unit * 9 + ["k", None]
    ot = oracle_table({"s": ["string", values]})
    preds = ["s = 'k1'", "s = 'k'", "s != 'k1'", "s IN ('k1', 'k1true0', 'k19.e')", "s IN ('k1true0k', 'k19.e-')",
             "s = ''", "s = 'k1ÿ'"]
    an = [d.Compliance("p%d" % i, p) for i, p in enumerate(preds)] + [d.Size("s = 'k1'"), d.Size("s = 'k'")]
    for off in OFFSETS:
        st = d.run_scan(an, _table(values, off, flavour, device))
        for a in an:
            _check_state(a, st[a], ot)


# ---------------------------------------------------------------- PatternMatch
SSN_SHAPE = r"\d{3}-\d{2}-\d{4}"
DECIMAL = r"\d+\.\d+"
ALL_DIGITS = r"^\d+$"
_PM = {}


def _pattern_case():
    if not _PM:
        assert {SSN_SHAPE, DECIMAL, ALL_DIGITS} <= {p for p, _ in C.PATTERNS}
        near = ["111-05-113", None, "10.", None, "111-05-1130", None, "x10.5y", None, "12", None, "078-05-", None,
                "7", "3.", None]
        rng = np.random.default_rng(91)
        seeds = [s for p, ss in C.PATTERNS if p in (SSN_SHAPE, DECIMAL, ALL_DIGITS) for s in ss]
        values = near * 8
        for k, s in enumerate(C.make_strings(seeds, 400, rng)):
            values += [s] if k % 3 else [None, s]
        values.append(None)
        _PM.update(values=values, want={p: sum(C.oracle(p, s) for s in values if s is not None)
                                        for p in (SSN_SHAPE, DECIMAL, ALL_DIGITS)})
        for p, m in _PM["want"].items():
            assert 20 <= m <= len(values) - 20, p
    return _PM["values"], _PM["want"]


@matrix
def test_pattern_match(gpu, flavour, device):
    """"111-05-113" + a NULL slot reading "1true0k" would match the SSN shape, "10." + "1" the decimal."""
    values, want = _pattern_case()
    an = [d.PatternMatch("s", p) for p in want]
    for off in OFFSETS:
        t = _table(values, off, flavour, device)
        got = run_plan(d, an, [t], t.schema)
        for p, g in zip(want, got):
            assert g == (14, 1, want[p], len(values)), (p, off, g)


# ---------------------------------------------------------------- string -> long / double casts
def _number(ln, k):
    if k % 4 == 2 and ln >= 3:
        return _digits(ln // 2, k) + "." + _digits(ln - ln // 2 - 1, k + 1)
    if k % 4 == 3 and ln >= 4:
        return _digits(ln - 2, k) + "e" + _digits(1, k)
    return _integral(ln, k)


def _same_cast(got, want, what):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        if g is None or w is None:
            assert g is None and w is None, (what, i, g, w)
        elif isinstance(w, float) and math.isnan(w):
            assert math.isnan(g), (what, i, g)
        elif isinstance(w, float):
            assert struct.pack("<d", g) == struct.pack("<d", w), (what, i, g, w)
        else:
            assert g == w, (what, i, g, w)


@pytest.mark.parametrize("device", [True, False], ids=["device", "host"])
def test_casts_row_by_row(gpu, device):
    """"digits" guards: a number read one byte too far is another number."""
    values = H.residue_grid(_number, extra=["9223372036854775807", "-9223372036854775808", "9223372036854775808",
                                            "1e308", "1.7976931348623157e308", "4.9e-324", "-0", "+5", "-", ".", "e"])
    want_long = [None if v is None else _spark_to_long(v) for v in values]
    want_double = [None if v is None else O.java_parse_double(v) for v in values]
    assert sum(w is not None for w in want_long) > 100 and sum(w is not None for w in want_double) > 200
    for off in OFFSETS:
        col = H.hostile_column("string", values, offset=off, flavour="digits", device=device)
        _same_cast(cast_string_column(col, "int64").to_pylist(), want_long, "long")
        _same_cast(cast_string_column(col, "float64").to_pylist(), want_double, "double")
        other = H.hostile_column("string", values, offset=off + 3, flavour="digits", device=device)
        as_long, as_double = cast_string_columns([col, other], ["int64", "float64"])
        _same_cast(as_long.to_pylist(), want_long, "batch long")
        _same_cast(as_double.to_pylist(), want_double, "batch double")


# ---------------------------------------------------------------- dq_profile_few_strings
@matrix
def test_profile_few_strings(gpu, flavour, device):
    rng = np.random.default_rng(17)
    pool = ["", "true", "tru", "12", "1", "k", "k1", "é", "x" * 15, "0123456789abcde", "3.", "NullValue"]
    cols = {"a": [None if rng.random() < 0.3 else pool[int(i)] for i in rng.integers(0, len(pool), 2049)],
            "b": [None if rng.random() < 0.5 else pool[int(i)] for i in rng.integers(0, 4, 2049)]}
    ot = oracle_table({c: ["string", v] for c, v in cols.items()})
    table = d.Table({c: H.hostile_column("string", v, offset=off, flavour=flavour, device=device)
                     for (c, v), off in zip(cols.items(), OFFSETS)})
    got = _batched_few(table, list(cols))
    for c, vals in cols.items():
        ok, groups, nulls, comp, hll, dt = got[c]
        assert ok == 1, c
        assert groups == dict(collections.Counter(v.encode("utf-8") for v in vals if v is not None)), c
        assert nulls == sum(v is None for v in vals)
        assert (comp.numMatches, comp.count) == (len(vals) - nulls, len(vals))
        assert list(hll.words) == list(O.approx_count_distinct_state(ot, c).words), c
        assert tuple(dt.counts()) == tuple(O.datatype_state(ot, c)), c


# ---------------------------------------------------------------- a whole profile
def _profile_spec(n=2049, seed=23):
    rng = np.random.default_rng(seed)

    def nulls(vals):
        return [None if rng.random() < 0.1 else v for v in vals]
    return {
        "s_int": ["string", nulls([str(int(x)) for x in rng.integers(-10 ** 9, 10 ** 12, n)])],
        "s_few": ["string", nulls([str(int(x)) for x in rng.integers(0, 40, n)])],
        "s_frac": ["string", nulls(["%d.%02d" % (x, x % 100) for x in rng.integers(0, 10 ** 7, n)])],
        "s_cat": ["string", nulls(["cat_%02d" % x for x in rng.integers(0, 50, n)])],
        "s_bool": ["string", nulls(["true" if x else "false" for x in rng.integers(0, 2, n)])],
        "s_id": ["string", nulls(["%016d" % x if x % 97 else "n/a" for x in rng.integers(0, 10 ** 15, n)])],
        "l": ["int64", nulls([int(x) for x in rng.integers(-10 ** 6, 10 ** 9, n)])],
        "l_few": ["int64", nulls([int(x) for x in rng.choice([0, 1, -7, 2147483647, -2 ** 40], n)])],
        "f": ["float64", nulls([float(x) for x in rng.normal(1000.0, 100.0, n)])],
        "b": ["bool", nulls([bool(x) for x in rng.integers(0, 2, n)])],
    }


def _exact(vals):
    fr = [Fraction(float(v)) for v in vals]
    n = len(fr)
    s1 = sum(fr)
    m2 = sum(x * x for x in fr) - s1 * s1 / n
    return float(s1), float(s1 / n), math.sqrt(float(m2 / n))


def _close(got, want):
    return abs(got - want) <= 1e-12 * max(1.0, abs(want))


@matrix
def test_whole_profile_matches_oracle(gpu, flavour, device):
    """As test_gpu_profiles_c5 compares a profile with O.column_profiles: every pass of the
    profiler (string pass / few-groups, casts of numeric strings, histograms) on hostile columns."""
    spec = _profile_spec()
    offsets = {name: H.OFFSETS[(3 + j) % len(H.OFFSETS)] for j, name in enumerate(spec)}
    profiles = ColumnProfilerRunner().onData(H.hostile_table(spec, offset=offsets, flavour=flavour, device=device)).run()
    want = O.column_profiles(oracle_table(spec))
    assert profiles.numRecords == want["__numRecords__"] == 2049
    assert list(profiles.profiles) == list(spec)
    n_hist = n_numeric_str = 0
    for name, p in profiles.profiles.items():
        w = want[name]
        assert p.completeness == w["completeness"], name
        assert p.approximateNumDistinctValues == w["approx"], name
        assert p.dataType == w["dataType"], name
        assert p.isDataTypeInferred == w["inferred"], name
        assert p.typeCounts == w["typeCounts"], name
        assert isinstance(p, NumericColumnProfile) == ("mean" in w), name
        if isinstance(p, NumericColumnProfile):
            n_numeric_str += spec[name][0] == "string"
            assert p.minimum == w["minimum"] and p.maximum == w["maximum"], name
            vals = w["numeric_values"]
            if all(isinstance(v, int) for v in vals):
                assert p.sum == w["sum"] and p.mean == w["mean"], name
                assert _close(p.stdDev, _exact(vals)[2]), (name, p.stdDev)
            else:
                s, m, sd = _exact(vals)
                assert _close(p.sum, s) and _close(p.mean, m) and _close(p.stdDev, sd), (name, p.sum, s, p.stdDev, sd)
        if w["histogram"] is None:
            assert p.histogram is None, name
        else:
            n_hist += 1
            assert p.histogram is not None, name
            assert p.histogram.numberOfBins == len(w["histogram"]), name
            assert {k: (v.absolute, v.ratio) for k, v in p.histogram.values.items()} == w["histogram"], name
    assert n_hist >= 5 and n_numeric_str >= 3
