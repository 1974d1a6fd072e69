"""correlation_matrix on the GPU (dq_corrmat.hip: the fp64 matrix cores) against the exact rational
state of every pair i <= j, at the bar of corrmatrix_cases.py (test_gpu_correlation.py's), and next
to the host mirror: equal n and equal fall-back flags on every case.

Shapes: slabs are 1024 rows, chunks 64, an MFMA step takes 4 rows; tiles are 16 x 16 columns.  The
row counts run over 5 mixed-dtype columns (NULLs from 63 rows on: with a handful of rows a pair whose
columns' shift rows are NULL in the other column has nothing ordinary about it, and the guard may
rightly hand it to the pair kernel), the column counts over 3 slabs + 5 rows, 33 columns once more
over 2^18 rows with NULLs.  The metric's NaN rule is checked against the exact state (NaN exactly
when xMk * yMk = 0), which test_corrmatrix.py ties to pyoracle.correlation_state on a host-sized case;
the non-finite cases, where no exact state exists, ask the oracle itself."""
import math
import zlib
from collections import OrderedDict
from fractions import Fraction

import numpy as np
import pytest

import decimal_cases as C
import deequ_amd as d
import pyoracle as O
from corrmatrix_cases import (COLUMN_COUNTS, NULL_PATTERNS, REL_TOL, ROW_COUNTS, SLAB, Case, _errors, case_host_mirror,
                              check_state, host_corrmat, pair_index)

pytestmark = pytest.mark.gpu


def _check(case, table, keep=None, where=None, fallback=0, label=""):
    """The matrix of `table` against the exact state of every pair, and against the host mirror."""
    m = d.correlation_matrix(table, case.names, where)
    for i, j in case.pairs():
        check_state("%s n=%d k=%d (%d,%d)" % (label, case.n, case.k, i, j), m.state(case.names[i], case.names[j]),
                    case.exact(i, j, keep))
    assert m.fallback_pairs == fallback, m.fallback_pairs
    states, flags = case_host_mirror(case, keep)
    assert np.array_equal(states[:, 0], m.counts()[np.triu_indices(case.k)]), label
    if fallback == 0:
        assert not flags.any(), np.nonzero(flags)
    return m, flags


@pytest.mark.parametrize("n", ROW_COUNTS)
def test_row_counts(gpu, n):
    nulls = "five_percent" if n >= 63 and n % 2 else "none"
    case = Case(5, n, 100 + n, nulls)
    _check(case, case.table(d), label="host " + nulls)
    _check(case, case.table(d).to_device(0), label="device " + nulls)


@pytest.mark.parametrize("k", COLUMN_COUNTS)
def test_column_counts_mixed_dtypes(gpu, k):
    case = Case(k, 3 * SLAB + 5, 200 + k)
    assert k < 6 or {"int8", "int16", "int32", "int64", "float32", "float64"} <= set(case.dtypes)
    _check(case, case.table(d).to_device(0), label="fast")
    masked = Case(k, 3 * SLAB + 5, 200 + k, "five_percent")
    _check(masked, masked.table(d).to_device(0), label="masked")


def test_33_columns_2_18_rows_with_nulls(gpu):
    case = Case(33, 1 << 18, 33, "five_percent")
    _check(case, case.table(d).to_device(0), label="2^18")


@pytest.mark.parametrize("nulls", NULL_PATTERNS)
def test_null_patterns(gpu, nulls):
    case = Case(4, 3 * 4096 + 5, 300, nulls)
    m, _ = _check(case, case.table(d), label=nulls)
    if nulls == "all_null_column":
        assert m.state("c1", "c1") is None and m.state("c0", "c1") is None and m.state("c1", "c3") is None
        assert m.counts()[0, 2] == float(case.n)
    if nulls == "last_row_only":
        assert m.state("c1", "c1").fields() == (1.0, case.values[1][-1], case.values[1][-1], 0.0, 0.0, 0.0)


def test_sliced_arrow_columns_with_bit_offsets(gpu):
    """Record batches sliced at rows 3 and 1501 (validity at bit offsets 3 and 5), and a device column
    handed over with an offset of 5 rows into its buffers."""
    import pyarrow as pa
    case = Case(4, 3000, 55, "five_percent")
    pat = {"int8": pa.int8(), "int16": pa.int16(), "int32": pa.int32(), "int64": pa.int64(), "float32": pa.float32(),
           "float64": pa.float64()}
    full = pa.record_batch({nm: pa.array(case.numpy_column(i), pat[case.dtypes[i]], mask=~case.valid[i])
                            for i, nm in enumerate(case.names)})
    cuts = [0, 3, 1501, 3000]
    _check(case, d.ArrowTable([full.slice(a, b - a) for a, b in zip(cuts, cuts[1:])]), label="arrow slices")
    dev = case.table(d).to_device(0)
    tail = Case(4, 3000, 55, "five_percent")
    tail.n = 2995
    tail.values = [v[5:] for v in case.values]
    tail.valid = [v[5:] for v in case.valid]
    cols = OrderedDict((nm, d.Column(c.dtype, 2995, c.values, c.validity, offset=5, device=True))
                       for nm, c in dev.columns.items())
    _check(tail, d.Table(cols), label="device offset 5")


@pytest.mark.parametrize("where", ["half", "none", "compound"])
def test_where(gpu, where):
    """The filter's mask comes from launch_predicates; the reference is the same table filtered on the
    host."""
    case = Case(5, 2 * 4096 + 77, 61, "five_percent")
    n = case.n
    rng = np.random.default_rng(61)
    g = rng.integers(0, 2, n)
    h_valid = rng.random(n) >= 0.3
    text, keep = {"half": ("g > 0", g > 0), "none": ("g > 5", np.zeros(n, dtype=bool)),
                  "compound": ("g > 0 AND h IS NOT NULL OR c0 > 16780000", ((g > 0) & h_valid) | (case.valid[0] & (case.values[0] > 16780000)))}[where]
    table = case.table(d)
    cols = OrderedDict(table.columns)
    cols["g"] = d.Column.from_numpy(g.astype(np.int64))
    cols["h"] = d.Column.from_numpy(np.ones(n, dtype=np.int64), h_valid, "int64")
    m, _ = _check(case, d.Table(cols), keep=keep, where=text, label="where " + where)
    if where == "none":
        assert all(s is None for s in m.states().values())
    assert list(m.states())[1] == d.Correlation("c0", "c1", text)


def test_three_batches_with_an_empty_middle_one(gpu):
    case = Case(6, 3 * 4096 + 9, 71, "five_percent")
    cuts = [0, 4096 + 3, 4096 + 3, case.n]
    parts = d.PartitionedTable([case.table(d, slice(a, b)) for a, b in zip(cuts, cuts[1:])])
    assert parts.batches()[1].num_rows == 0
    m = d.correlation_matrix(parts, case.names)
    for i, j in case.pairs():
        check_state("3 batches (%d,%d)" % (i, j), m.state(case.names[i], case.names[j]), case.exact(i, j))
    again = d.correlation_matrix(parts, case.names)
    assert m.fallback_pairs == 0 and again.states() == m.states()


def test_pair_path_bits_unchanged_around_a_matrix_call(gpu):
    case = Case(4, 5000, 81, "five_percent")
    table = case.table(d).to_device(0)
    analyzers = [d.Correlation(case.names[i], case.names[j]) for i, j in case.pairs()]
    before = d.run_scan(analyzers, table)
    d.correlation_matrix(table, case.names)
    after = d.run_scan(analyzers, table)
    assert all(before[a] == after[a] for a in analyzers)


def _flagged(k, col):
    return sorted(pair_index(min(i, col), max(i, col), k) for i in range(k))


def test_outlier_shift_falls_back_for_exactly_that_column(gpu):
    case = Case(5, 4 * SLAB + 17, 41)
    rows = np.arange(0, case.n, SLAB)
    case.values[2] = np.rint(case.values[2] / 2.0 ** 24 * 1024) / 1024  # values near 1: 1e8 is far out
    case.values[2][rows] = np.where((rows // SLAB) % 3 != 0, 1e8, -1e8)
    case.dtypes[2] = "float64"
    _, flags = _check(case, case.table(d).to_device(0), fallback=5, label="outlier")
    assert sorted(np.nonzero(flags)[0].tolist()) == _flagged(5, 2)


def _oracle(case, values, i, j):
    def col(c):
        return O.OColumn("float64", [float(v) if ok else None for v, ok in zip(values[c], case.valid[c])])
    return O.correlation_state({"x": col(i), "y": col(j)} if i != j else {"x": col(i)}, "x", "y" if i != j else "x")


def _non_finite_case(what):
    case = Case(4, 2 * SLAB + 3, 43, "five_percent")
    v = case.values[1].copy()
    if what == "non_finite":
        rows = np.nonzero(~case.valid[2])[0][:6]  # rows where another column is NULL
        v[rows] = [np.inf, -np.inf, np.nan, np.inf, np.nan, -np.inf]
        case.valid[1][rows] = True
    else:
        v[5::97] = 1e200
        v[6::97] = -1e200
    values = list(case.values)
    values[1] = v
    cols = OrderedDict()
    for i, nm in enumerate(case.names):
        arr = values[i] if i == 1 else case.numpy_column(i)
        cols[nm] = d.Column.from_numpy(arr, case.valid[i] if case.has_nulls(i) else None, "float64" if i == 1 else case.dtypes[i])
    return case, values, d.Table(cols)


def _check_non_finite(what):
    case, values, table = _non_finite_case(what)
    m = d.correlation_matrix(table.to_device(0), case.names)
    assert m.fallback_pairs == 4
    valid = [case.valid[i] if case.has_nulls(i) else None for i in range(4)]
    states, flags = host_corrmat(values, valid)
    assert sorted(np.nonzero(flags)[0].tolist()) == _flagged(4, 1)
    assert np.array_equal(states[:, 0], m.counts()[np.triu_indices(4)])
    for i, j in case.pairs():
        got = m.state(case.names[i], case.names[j])
        if 1 in (i, j):
            o = _oracle(case, values, i, j)
            print(what, (i, j), got, o.metric_value())
            assert got.n == o.n, (i, j)
            assert math.isnan(got.metricValue()) == math.isnan(o.metric_value()), (i, j, got, o.metric_value())
        else:
            check_state("%s (%d,%d)" % (what, i, j), got, case.exact(i, j))


def test_non_finite_values_fall_back(gpu):
    """+-Inf and NaN in one column at rows where another column is NULL.  That column's pairs fall back
    (the pair kernel answers them): n and whether the metric is NaN are the oracle's for every pair,
    and the pairs without the column meet the bar with no fall-back."""
    _check_non_finite("non_finite")


def test_overflowing_squares_fall_back(gpu):
    """+-1e200 (finite) in one column, whose squared deviations overflow to Inf: that column's pairs
    fall back, and n and the metric's NaN-ness are the oracle's.  The pair kernel's Sxx - Sx² / n is
    Inf - Inf there (yMk NaN, metric NaN, where Spark has yMk = Inf and the metric 0.0), so pairs whose
    sums of finite values were not finite are answered by Spark's per-row update instead
    (dq_corrmat_rows_kernel); only the diagonal pair is NaN (Inf / Inf), as Spark's."""
    _check_non_finite("overflowing_squares")


def test_decimal_column_beside_a_float64_one(gpu):
    """decimal(12,2) goes through dq_cast_decimal as Correlation's does: the matrix against
    Correlation of the same pairs, at the bar."""
    n = 3000
    price = C.column_values("random", n, 12, 2, seed=31)
    rng = np.random.default_rng(zlib.crc32(b"decimal"))
    f = np.rint(rng.normal(100, 10, n) * 1024) / 1024
    valid = np.array([v is not None for v in price], dtype=bool)
    table = d.Table(OrderedDict([("m", d.Column.from_numpy(C.le_words(price), valid, "decimal(12,2)")),
                                 ("f", d.Column.from_numpy(f))]))
    m = d.correlation_matrix(table, ["m", "f"], where="f > 90")
    assert m.fallback_pairs == 0
    for x, y in (("m", "m"), ("m", "f"), ("f", "f")):
        want = d.Correlation(x, y, "f > 90").computeStateFrom(table)
        got = m.state(x, y)
        err = _errors(got, tuple([want.n] + [Fraction(v) for v in want.fields()[1:]]))
        print("decimal", x, y, err)
        assert got.n == want.n and all(v <= REL_TOL for v in err.values()), (x, y, err)
