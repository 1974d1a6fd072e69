"""Decimal columns on the GPU: the fused decimal scan (dq_scan_dec.hip), dq_cast_decimal and the
analyzers that ride on it, the profiler, and what decimal columns decline.

Every reference is Python's exact arithmetic (tests/decimal_cases.py), independent of the library:
sums / minima / maxima are Python ints converted once by `float(Fraction(u, 10 ** s))` (Spark's
sum(col).cast(DoubleType), BigDecimal.doubleValue) and compared bit for bit; StandardDeviation's n is
exact and its mean and m2 lie within 1e-12 (relative) of the exact rational moments of the converted
doubles (the bar of tests/test_gpu_moments.py); ApproxCountDistinct's words equal hll_pack of
registers computed from Spark's decimal hash.  Row counts sit around the wave (64), the 2048-row
chunk and several workgroups."""
import decimal
import struct
from collections import OrderedDict
from fractions import Fraction

import numpy as np
import pyarrow as pa
import pytest

import deequ_amd as d
from deequ_amd import _lib as L
from deequ_amd.engine import OpUnsupported, op_spec_for, run_scan_raw
from deequ_amd.states import state_from_dq

import decimal_cases as C

pytestmark = pytest.mark.gpu

REL_TOL = 1e-12
SIZES = (1, 63, 64, 65, 2047, 2048, 2049, 20001)
DTYPES = ((9, 2), (18, 0), (19, 4), (38, 10), (38, 38))


def _bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def _column(values, p, s):
    valid = np.array([v is not None for v in values], dtype=bool)
    return d.Column.from_numpy(C.le_words(values), valid, "decimal(%d,%d)" % (p, s))


def _moderate(n, seed):
    """Random decimal(38,10) values of at most 30 digits (NULLs among them): their sums stay below
    10^38, so Sum and Mean answer."""
    return C.column_values("random", n, 30, 10, seed=seed)


def _scan(analyzers, data):
    """States (None = Spark's NULL) or OpUnsupported per analyzer, from one fused pass."""
    raw = run_scan_raw([op_spec_for(a, data.schema) for a in analyzers], data)
    return [r if isinstance(r, OpUnsupported) else state_from_dq(r) for r in raw]


def _stats(c, where=None):
    return [d.Size(where), d.Completeness(c, where), d.Sum(c, where), d.Mean(c, where), d.Minimum(c, where),
            d.Maximum(c, where), d.StandardDeviation(c, where), d.ApproxCountDistinct(c, where)]


def _expect(n_rows, sel, p, s):
    """What the eight analyzers of _stats must give for the selected non-NULL unscaled values `sel`
    among n_rows rows in scope (computed once per case and shared by the residencies)."""
    e = {"n_rows": n_rows, "n": len(sel), "hll": C.hll_words(sel, p)}
    if sel:
        total = sum(sel)
        e["overflow"] = sum(abs(u) for u in sel) >= 10 ** min(38, p + 10)
        e["sum"] = C.exact_double(total, s)
        e["min"] = C.exact_double(min(sel), s)
        e["max"] = C.exact_double(max(sel), s)
        xs = [Fraction(C.exact_double(u, s)) for u in sel]
        s1 = sum(xs)
        e["mean"] = s1 / len(xs)
        e["m2"] = sum(x * x for x in xs) - s1 * s1 / len(xs)
    return e


def _check(states, e, what):
    size, comp, sm, mean, mn, mx, sd, acd = states
    assert size == d.NumMatches(e["n_rows"]), what
    if e["n_rows"] == 0:
        assert comp is None, what
    else:
        assert comp == d.NumMatchesAndCount(e["n"], e["n_rows"]), (what, comp)
    assert list(acd.words) == list(e["hll"]), what
    if e["n"] == 0:
        assert sm is None and mean is None and mn is None and mx is None and sd is None, what
        return
    if e["overflow"]:  # declined per op, never approximated
        for st in (sm, mean):
            assert isinstance(st, OpUnsupported) and isinstance(st.error, L.UnsupportedOnGpu), what
            assert "SPARK-28067" in str(st.error), what
    else:
        assert _bits(sm.sum_value) == _bits(e["sum"]), (what, sm.sum_value, e["sum"])
        assert _bits(mean.sum_value) == _bits(e["sum"]) and mean.count == e["n"], what
    assert _bits(mn.minValue) == _bits(e["min"]), (what, mn.minValue, e["min"])
    assert _bits(mx.maxValue) == _bits(e["max"]), (what, mx.maxValue, e["max"])
    assert sd.n == float(e["n"]), what
    want_mean, want_m2 = float(e["mean"]), float(e["m2"])
    print("%s: mean %r (exact %r) m2 %r (exact %r)" % (what, sd.avg, want_mean, sd.m2, want_m2))
    assert abs(sd.avg - want_mean) <= REL_TOL * abs(want_mean), (what, sd.avg, want_mean)  # (0: equality)
    assert abs(sd.m2 - want_m2) <= REL_TOL * abs(want_m2), (what, sd.m2, want_m2)


# every kind on every type, but "ties" only where the type can hold an exact tie of the cast
# (C.tie_pool: decimal(9,2) and decimal(38,38) hold none); the issue's own tie values, whose scales
# are 1, 10, 22, 0 and 3, run in columns of their own types in test_issue_ties_on_the_device
CASES = [(ps, kind) for ps in DTYPES for kind in C.KINDS if kind != "ties" or C.tie_pool(*ps)]


@pytest.mark.parametrize("ps,kind", CASES, ids=["decimal(%d,%d)-%s" % (ps + (k,)) for ps, k in CASES])
def test_scan_states_match_exact_arithmetic(gpu, ps, kind):
    p, s = ps
    for n in SIZES:
        values = C.column_values(kind, n, p, s)
        e = _expect(n, [v for v in values if v is not None], p, s)
        host = d.Table({"m": _column(values, p, s)})
        for name, table in (("host", host), ("device", host.to_device(0))):
            _check(_scan(_stats("m"), table), e, (ps, kind, n, name))


def test_hash_case_follows_the_column_precision(gpu):
    """decimal(18,0) hashes the unscaled long, decimal(19,0) BigInteger.toByteArray of the same
    values: chosen by the type, so the registers differ."""
    values = C.column_values("random", 2049, 18, 0, seed=3)
    words = []
    for p in (18, 19):
        acd, = _scan([d.ApproxCountDistinct("m")], d.Table({"m": _column(values, p, 0)}).to_device(0))
        assert list(acd.words) == list(C.hll_words(values, p)), p
        words.append(list(acd.words))
    assert words[0] != words[1]


def test_where_filters_and_null_tests(gpu):
    p, s, n = 19, 4, 2049
    values = C.column_values("random", n, p, s, seed=5)
    rng = np.random.default_rng(5)
    ints = [int(x) if ok else None for x, ok in zip(rng.integers(-50, 50, n), rng.random(n) > 0.2)]
    host = d.Table(OrderedDict([("m", _column(values, p, s)), ("i", d.Column.from_pylist(ints, "int64"))]))
    for table in (host, host.to_device(0)):
        for where, keep in (("i > 3", lambda i, v: i is not None and i > 3),
                            ("i IS NULL OR i < -20", lambda i, v: i is None or i < -20),
                            ("m IS NOT NULL", lambda i, v: v is not None),
                            ("m IS NULL", lambda i, v: v is None),
                            ("m IS NOT NULL AND i >= 0", lambda i, v: v is not None and i is not None and i >= 0)):
            rows = [v for i, v in zip(ints, values) if keep(i, v)]
            e = _expect(len(rows), [v for v in rows if v is not None], p, s)
            _check(_scan(_stats("m", where), table), e, where)
        comp, = _scan([d.Compliance("nulls", "m IS NULL")], table)
        assert comp == d.NumMatchesAndCount(sum(v is None for v in values), n)
        with pytest.raises(d.predicates.UnsupportedPredicate):
            _scan([d.Size("m > 1")], table)


def test_two_batches_equal_one(gpu):
    p, s = 38, 10
    values = _moderate(2049 + 65, 9)
    one = d.Table({"m": _column(values, p, s)})
    two = d.PartitionedTable([d.Table({"m": _column(values[:2049], p, s)}), d.Table({"m": _column(values[2049:], p, s)})])
    a, b = _scan(_stats("m"), one), _scan(_stats("m"), two)
    for x, y in zip(a[:6] + a[7:], b[:6] + b[7:]):
        assert x == y, (x, y)
    _check(b, _expect(len(values), [v for v in values if v is not None], p, s), "two batches")
    # a sum that rounds differently when converted per batch: batch totals 2^53, 1 and 1 -- adding
    # their doubles gives 2^53 twice over (2^53 + 1 is a tie that rounds back to even), the exact
    # sum 2^53 + 2 is the next double; and the same totals twice, whose exact sum is 2^54 + 4
    for parts, exact in (([[2 ** 52, 2 ** 52], [1], [1]], 2 ** 53 + 2),
                         ([[2 ** 52, 2 ** 52], [1], [1], [2 ** 53 - 5, 5], [1], [1]], 2 ** 54 + 4)):
        data = d.PartitionedTable([d.Table({"m": _column(v, 18, 0)}).to_device(0) for v in parts])
        sm, mean = _scan([d.Sum("m"), d.Mean("m")], data)
        naive = 0.0
        for v in parts:
            naive += float(sum(v))
        assert naive != float(exact)
        assert sm.sum_value == float(exact), (sm.sum_value, exact)
        assert mean.sum_value == float(exact) and mean.count == sum(len(v) for v in parts)


def test_sum_overflow_is_declined_per_op(gpu):
    """Three rows of 5e37 in decimal(38,0): the sum of |x| reaches 10^38, where Spark 2.2's result
    depends on the row order (SPARK-28067) -- Sum and Mean are declined, Maximum still answers.
    Two such rows sum exactly."""
    x = 5 * 10 ** 37
    three = d.Table({"m": _column([x, x, x], 38, 0)}).to_device(0)
    sm, mean, mx = _scan([d.Sum("m"), d.Mean("m"), d.Maximum("m")], three)
    assert isinstance(sm, OpUnsupported) and isinstance(mean, OpUnsupported)
    assert isinstance(sm.error, L.UnsupportedOnGpu) and sm.error.status == L.DQ_ERR_UNSUPPORTED
    assert mx.maxValue == float(x)
    ctx = d.AnalysisRunner.onData(three).addAnalyzers([d.Sum("m"), d.Maximum("m")]).run()
    assert ctx.metric(d.Sum("m")).value.isFailure and ctx.metric(d.Maximum("m")).value.get() == float(x)
    # two such rows: their sum, 10^38 itself, is the first value decimal(38,0) cannot hold, so the
    # stated bound (sum of |x| >= 10^38) declines them as well; just below it the sum is exact
    two = d.Table({"m": _column([x, x], 38, 0)}).to_device(0)
    sm, mean, mx = _scan([d.Sum("m"), d.Mean("m"), d.Maximum("m")], two)
    assert isinstance(sm, OpUnsupported) and isinstance(mean, OpUnsupported) and mx.maxValue == float(x)
    under = d.Table({"m": _column([x, x - 1], 38, 0)}).to_device(0)
    sm, mean, mx = _scan([d.Sum("m"), d.Mean("m"), d.Maximum("m")], under)
    assert sm.sum_value == C.exact_double(10 ** 38 - 1, 0) and mean.count == 2 and mx.maxValue == float(x)
    # alternating signs: the sum is small, the sum of |x| is not
    alt = d.Table({"m": _column([x, -x, x, -x], 38, 0)})
    sm, mn = _scan([d.Sum("m"), d.Minimum("m")], alt)
    assert isinstance(sm, OpUnsupported) and mn.minValue == float(-x)


def test_sliced_arrow_columns(gpu):
    p, s = 19, 4
    values = C.column_values("random", 2052, p, s, seed=13)
    arr = pa.array([None if v is None else decimal.Decimal(v).scaleb(-s) for v in values], pa.decimal128(p, s))
    ints = pa.array(list(range(2052)), pa.int64())
    e = _expect(2049, [v for v in values[3:] if v is not None], p, s)
    sliced = pa.record_batch([arr.slice(3), ints.slice(3)], names=["m", "i"])
    table = d.Table.from_arrow(sliced)
    assert table.columns["m"].offset == 3
    _check(_scan(_stats("m"), table), e, "from_arrow host")
    _check(_scan(_stats("m"), table.to_device(0)), e, "from_arrow device")
    # a sliced record batch: the children keep the batch's offset
    whole = d.Table.from_arrow(pa.record_batch([arr, ints], names=["m", "i"]).slice(3))
    assert whole.columns["m"].offset == 3
    _check(_scan(_stats("m"), whole), e, "sliced batch")
    # a slice whose first row is not on a validity byte boundary nor at row 0 of the device buffer
    from deequ_amd.decimals import cast_to_float64
    got = cast_to_float64(table.to_device(0).columns["m"], 0).to_pylist()
    assert [None if x is None else _bits(x) for x in got] == \
        [None if v is None else _bits(C.exact_double(v, s)) for v in values[3:]]
    with pytest.raises(L.UnsupportedOnGpu):  # the C Data Interface route keeps declining decimals
        _scan(_stats("m"), d.ArrowTable(sliced))


def test_issue_ties_on_the_device(gpu):
    """The issue's tie values -- (2^53 + 1) 5^s for s = 1, 10, 22, 2^100 + 2^47 at scale 0,
    (2^64 + 2^11) 5^3 at scale 3 -- with u +- 1 and both signs, each group in a column of its own
    (precision, scale): through dq_cast_decimal bit for bit (the Eisel-Lemire tier at s = 1, the long
    division at s = 10, 22 and 3, the wide-integer rounding at s = 0), and through the scan, whose
    StandardDeviation casts them in the kernel."""
    from deequ_amd.decimals import cast_to_float64
    groups = C.tie_groups()
    assert sorted(s for _p, s in groups) == [0, 1, 3, 10, 22]
    for (p, s), vals in groups.items():
        vals = vals + [v for v in vals if v > 0] + [None]  # (not sign-symmetric: the mean is not 0)
        host = d.Table({"m": _column(vals, p, s)})
        for name, table in (("host", host), ("device", host.to_device(0))):
            got = cast_to_float64(table.columns["m"], 0).to_pylist()
            assert [None if x is None else _bits(x) for x in got] == \
                [None if v is None else _bits(C.exact_double(v, s)) for v in vals], (p, s, name)
            _check(_scan(_stats("m"), table), _expect(len(vals), [v for v in vals if v is not None], p, s),
                   ("issue ties", p, s, name))


def test_cast_decimal_is_correctly_rounded(gpu):
    from deequ_amd.decimals import cast_to_float64
    for p, s in DTYPES:
        values = C.column_values("random", 2049, p, s, seed=17) + C.tie_pool(p, s) + \
            C.column_values("byte_lengths", 65, p, s) + [10 ** p - 1, -(10 ** p - 1), None, 0]
        host = _column(values, p, s)
        for col in (host, host.to_device(0)):
            out = cast_to_float64(col, 0)
            assert out.dtype == "float64" and out.length == len(values)
            got = out.to_pylist()
            for u, x in zip(values, got):
                if u is None:
                    assert x is None
                else:
                    assert _bits(x) == _bits(C.exact_double(u, s)), (p, s, u, x)


def test_correlation_and_quantiles_equal_the_float64_column(gpu):
    p, s, n = 38, 10, 20001
    values = _moderate(n, 21)
    rng = np.random.default_rng(21)
    other = [float(x) if ok else None for x, ok in zip(rng.normal(0, 1e6, n), rng.random(n) > 0.1)]
    doubles = [None if v is None else C.exact_double(v, s) for v in values]
    o = d.Column.from_pylist(other, "float64")
    dec = d.Table(OrderedDict([("m", _column(values, p, s)), ("f", o)]))
    flt = d.Table(OrderedDict([("m", d.Column.from_pylist(doubles, "float64")), ("f", o)]))
    batches = d.PartitionedTable([d.Table(OrderedDict([("m", _column(values[a:b], p, s)),
                                                       ("f", d.Column.from_pylist(other[a:b], "float64"))]))
                                  for a, b in ((0, 2049), (2049, n))])
    fbatches = d.PartitionedTable([d.Table(OrderedDict([("m", d.Column.from_pylist(doubles[a:b], "float64")),
                                                        ("f", d.Column.from_pylist(other[a:b], "float64"))]))
                                   for a, b in ((0, 2049), (2049, n))])
    analyzers = [d.Correlation("m", "f"), d.Correlation("f", "m", "f > 0"), d.Correlation("m", "m"),
                 d.ApproxQuantile("m", 0.5), d.ApproxQuantile("m", 0.99, 0.005),
                 d.ApproxQuantiles("m", (0.1, 0.5, 0.9)), d.Mean("f")]
    for a_data, b_data in ((dec, flt), (dec.to_device(0), flt.to_device(0)), (batches, fbatches)):
        got = d.AnalysisRunner.onData(a_data).addAnalyzers(analyzers).run()
        want = d.AnalysisRunner.onData(b_data).addAnalyzers(analyzers).run()
        for a in analyzers:
            g, w = got.metric(a).value.get(), want.metric(a).value.get()
            if isinstance(g, dict):
                assert {k: _bits(v) for k, v in g.items()} == {k: _bits(v) for k, v in w.items()}, a
            else:
                assert _bits(g) == _bits(w), (a, g, w)
        assert d.Correlation("m", "f").computeStateFrom(a_data).fields() == \
            d.Correlation("m", "f").computeStateFrom(b_data).fields()
    bad = d.AnalysisRunner.onData(dec).addAnalyzer(d.Correlation("m", "f", "m > 1")).run()
    assert bad.metric(d.Correlation("m", "f", "m > 1")).value.isFailure


def test_kll_sketch_of_a_decimal_column_fails_as_the_reference(gpu):
    """KLLRunner.scala:142-143: isNumeric passes, then `Cannot handle DecimalType(p,s)`."""
    t = d.Table(OrderedDict([("m", _column([1, 2, None], 10, 2)), ("i", d.Column.from_pylist([1, 2, 3], "int64"))]))
    ctx = d.AnalysisRunner.onData(t).addAnalyzers([d.KLLSketch("m"), d.KLLSketch("i")]).run()
    m = ctx.metric(d.KLLSketch("m"))
    assert m.value.isFailure and "Cannot handle DecimalType(10,2)" in str(m.value.exception)
    assert ctx.metric(d.KLLSketch("i")).value.isSuccess
    single = d.KLLSketch("m").calculate(t)
    assert single.value.isFailure and "Cannot handle DecimalType(10,2)" in str(single.value.exception)


def test_analysis_run_beside_other_columns(gpu):
    p, s, n = 9, 2, 2049
    values = C.column_values("random", n, p, s, seed=25)
    big = _moderate(n, 26)
    rng = np.random.default_rng(25)
    ints = [int(x) for x in rng.integers(-1000, 1000, n)]
    strs = [("k%d" % (x % 7)) if x % 11 else None for x in ints]
    t = d.Table(OrderedDict([("m", _column(values, p, s)), ("i", d.Column.from_pylist(ints, "int64")),
                             ("b", _column(big, 38, 10)), ("s", d.Column.from_pylist(strs, "string"))])).to_device(0)
    analyzers = _stats("m") + _stats("b", "i > 0")[1:] + [
        d.Sum("i"), d.Minimum("i"), d.Completeness("s"), d.ApproxCountDistinct("s"), d.Uniqueness(["s"]),
        d.Compliance("pos", "i > 0"), d.Correlation("m", "i"), d.ApproxQuantile("b", 0.5), d.KLLSketch("m"),
        d.DataType("s"), d.Histogram("i")]
    ctx = d.AnalysisRunner.onData(t).addAnalyzers(analyzers).run()
    sel = [v for v in values if v is not None]
    assert ctx.metric(d.Sum("m")).value.get() == C.exact_double(sum(sel), s)
    assert ctx.metric(d.Mean("m")).value.get() == C.exact_double(sum(sel), s) / len(sel)
    assert ctx.metric(d.Maximum("m")).value.get() == C.exact_double(max(sel), s)
    assert ctx.metric(d.Completeness("m")).value.get() == len(sel) / n
    bsel = [v for v, i in zip(big, ints) if v is not None and i > 0]
    assert ctx.metric(d.Sum("b", "i > 0")).value.get() == C.exact_double(sum(bsel), 10)
    assert ctx.metric(d.Minimum("b", "i > 0")).value.get() == C.exact_double(min(bsel), 10)
    assert ctx.metric(d.Sum("i")).value.get() == float(sum(ints))
    assert ctx.metric(d.Minimum("i")).value.get() == float(min(ints))
    assert ctx.metric(d.Compliance("pos", "i > 0")).value.get() == sum(i > 0 for i in ints) / n
    for a in (d.Correlation("m", "i"), d.ApproxQuantile("b", 0.5), d.Uniqueness(["s"]), d.DataType("s"),
              d.Histogram("i"), d.StandardDeviation("m"), d.ApproxCountDistinct("m")):
        assert ctx.metric(a).value.isSuccess, a
    assert ctx.metric(d.KLLSketch("m")).value.isFailure


def test_profiler_with_decimal_columns(gpu):
    n = 2049
    price = C.column_values("random", n, 12, 2, seed=31)
    wide = _moderate(n, 32)
    rng = np.random.default_rng(31)
    ints = [int(x) for x in rng.integers(0, 5, n)]
    t = d.Table(OrderedDict([("price", _column(price, 12, 2)), ("qty", d.Column.from_pylist(ints, "int64")),
                             ("wide", _column(wide, 38, 10)),
                             ("name", d.Column.from_pylist(["n%d" % (i % 3) for i in range(n)], "string")),
                             ("f", d.Column.from_pylist([float(i) for i in ints], "float64"))])).to_device(0)
    from deequ_amd.profiles import ColumnProfilerRunner
    profiles = ColumnProfilerRunner().onData(t).run().profiles
    for c, vals, s, prec in (("price", price, 2, 12), ("wide", wide, 10, 38)):
        pr = profiles[c]
        sel = [v for v in vals if v is not None]
        assert pr.dataType == d.DataTypeInstances.Fractional and pr.isDataTypeInferred is False
        assert pr.histogram is None
        assert pr.completeness == len(sel) / n
        assert pr.approximateNumDistinctValues == int(d.ApproxCountDistinctState(C.hll_words(sel, prec)).metricValue())
        assert pr.minimum == C.exact_double(min(sel), s) and pr.maximum == C.exact_double(max(sel), s)
        assert pr.sum == C.exact_double(sum(sel), s)
        assert pr.mean == C.exact_double(sum(sel), s) / len(sel)
        xs = [Fraction(C.exact_double(u, s)) for u in sel]
        m2 = float(sum(x * x for x in xs) - sum(xs) ** 2 / len(xs))
        assert abs(pr.stdDev - (m2 / len(xs)) ** 0.5) <= 1e-12 * (m2 / len(xs)) ** 0.5
    assert profiles["qty"].histogram is not None and profiles["qty"].sum == float(sum(ints))
    assert profiles["name"].histogram is not None


def test_excluded_cases_raise_unsupported(gpu):
    """refused with UnsupportedOnGpu naming the column, never answered."""
    from deequ_amd.frequencies import compute_frequencies
    from deequ_amd.schema import RowLevelSchema, RowLevelSchemaValidator
    t = d.Table(OrderedDict([("m", _column([1, 2, 2, None], 10, 2)),
                             ("s", d.Column.from_pylist(["a", "b", "b", None], "string"))])).to_device(0)
    for fn in (lambda: compute_frequencies(t, ["m"]), lambda: compute_frequencies(t, ["s", "m"]),
               lambda: compute_frequencies(t, ["m"], histogram=True),
               lambda: RowLevelSchemaValidator.validate(t, RowLevelSchema().withStringColumn("s")),
               lambda: _scan([d.DataType("m")], t)):
        with pytest.raises(L.UnsupportedOnGpu) as e:
            fn()
        assert "decimal(10,2)" in str(e.value), str(e.value)
    for a in (d.Uniqueness(["m"]), d.CountDistinct(["m"]), d.Entropy("m"), d.Histogram("m")):
        m = d.AnalysisRunner.onData(t).addAnalyzer(a).run().metric(a)
        assert m.value.isFailure and "column m" in str(m.value.exception), a
    with pytest.raises(d.predicates.UnsupportedPredicate):
        _scan([d.Compliance("c", "m >= 1.00")], t)
    import datetime
    for arr in (pa.array([datetime.date(2020, 1, 1)]), pa.array([datetime.datetime(2020, 1, 1)]),
                pa.array([decimal.Decimal(1)], pa.decimal256(40, 2))):
        with pytest.raises(L.UnsupportedOnGpu):
            d.AnalysisRunner.onData(d.ArrowTable(pa.table({"c": arr}))).addAnalyzer(d.Completeness("c")).run()
