"""correlation_matrix without a GPU: the preconditions and declines, the pair indexing, the result
object (keys, mirrored states, persistence), and the algorithm itself through its host mirror
dq_diag_corrmat_host (deequ_amd/csrc/dq_corrmat.h: the kernel's slabs, shifts, guard, flags and merge
order with plain fp64 loops), held to the bar of corrmatrix_cases.py against the exact rational
state.  The sums of a pair cost O(rows) on the host, so the 2^18-row cases take 2 and 17 columns and
the 33- and 64-column cases one slab + 1 rows."""
import math

import numpy as np
import pytest

import deequ_amd as d
import pyoracle as O
from corrmatrix_cases import (COLUMN_COUNTS, NULL_PATTERNS, ROW_COUNTS, SLAB, Case, case_host_mirror, check_state,
                              host_corrmat, host_state, pair_index)
from deequ_amd import _lib as L
from deequ_amd.analyzers import NoSuchColumnException, WrongColumnTypeException
from deequ_amd.correlation import CorrelationMatrix, check_columns
from deequ_amd.distributed import ShardedTable


def _table():
    return d.Table.from_pydict({"a": ("int64", [1, 2, 3]), "b": ("float64", [1.0, 2.5, None]),
                                "s": ("string", ["x", "y", "z"]), "m": ("decimal(12,2)", [None, None, None])})


# ---------------------------------------------------------------- preconditions and declines
def test_unknown_and_non_numeric_columns_raise_correlations_messages():
    t = _table()
    with pytest.raises(NoSuchColumnException) as e:
        d.correlation_matrix(t, ["a", "nope"])
    assert str(e.value) == "Input data does not include column nope!"
    with pytest.raises(WrongColumnTypeException) as e:
        d.correlation_matrix(t, ["a", "s"])
    with pytest.raises(WrongColumnTypeException) as want:
        for cond in d.Correlation("a", "s").additionalPreconditions():
            cond(t.schema)
    assert str(e.value) == str(want.value) and "Expected type of column s" in str(e.value)


def test_empty_and_repeated_column_lists_raise_value_error():
    t = _table()
    with pytest.raises(ValueError, match="at least one column"):
        d.correlation_matrix(t, [])
    with pytest.raises(ValueError, match="column a is listed twice"):
        d.correlation_matrix(t, ["a", "b", "a"])


def test_sharded_table_is_declined():
    with pytest.raises(L.UnsupportedOnGpu, match="correlation_matrix over a ShardedTable"):
        d.correlation_matrix(ShardedTable(_table()), ["a", "b"])


def test_more_than_64_columns_is_declined_naming_the_cap():
    schema = {"c%d" % i: "float64" for i in range(65)}
    check_columns(schema, list(schema)[:64])
    with pytest.raises(L.UnsupportedOnGpu, match="65 columns: one matrix holds at most 64"):
        check_columns(schema, list(schema))
    t = d.Table({n: d.Column.from_numpy(np.zeros(2)) for n in schema})
    with pytest.raises(L.UnsupportedOnGpu, match="at most 64"):
        d.correlation_matrix(t, list(schema))


def test_declined_where_keeps_the_compilers_error():
    from deequ_amd.predicates import compile_predicate
    from deequ_amd.engine import schema_index
    t = _table()
    with pytest.raises(Exception) as want:
        compile_predicate("upper(s) = 'A'", schema_index(t.schema))
    with pytest.raises(type(want.value)) as e:
        d.correlation_matrix(t, ["a", "b"], where="upper(s) = 'A'")
    assert str(e.value) == str(want.value)


# ---------------------------------------------------------------- indexing and the result object
@pytest.mark.parametrize("k", [1, 2, 3, 16, 17, 64])
def test_pair_index_is_the_row_major_upper_triangle(k):
    brute = [(i, j) for i in range(k) for j in range(i, k)]
    assert [pair_index(i, j, k) for i, j in brute] == list(range(k * (k + 1) // 2))
    from deequ_amd.correlation import pair_index as lib_index
    assert [lib_index(i, j, k) for i, j in brute] == list(range(len(brute)))


def _small_matrix(where=None):
    case = Case(3, 40, 7, "five_percent")
    states, flags = case_host_mirror(case)
    assert not flags.any()
    return case, CorrelationMatrix(case.names, where, states, 0)


def test_states_keys_are_the_correlation_analyzers():
    case, m = _small_matrix("c0 > 0")
    assert m.columns == ("c0", "c1", "c2") and m.fallback_pairs == 0
    assert list(m.states()) == [d.Correlation(x, y, "c0 > 0") for x, y in
                                [("c0", "c0"), ("c0", "c1"), ("c0", "c2"), ("c1", "c1"), ("c1", "c2"), ("c2", "c2")]]
    for a, s in m.states().items():
        assert s == m.state(a.firstColumn, a.secondColumn)
        got, want = m.metric(a.firstColumn, a.secondColumn), a.computeMetricFrom(s)
        assert got.value.get() == want.value.get() and got.instance == want.instance
    assert m.matrix().shape == (3, 3) and np.array_equal(m.matrix(), m.matrix().T)
    assert m.counts()[0, 1] == float((case.valid[0] & case.valid[1]).sum())
    with pytest.raises(KeyError):
        m.state("c0", "nope")


def test_state_mirrors_and_diagonal_is_one_sum():
    _, m = _small_matrix()
    s, t = m.state("c0", "c2"), m.state("c2", "c0")
    assert t.fields() == (s.n, s.yAvg, s.xAvg, s.ck, s.yMk, s.xMk)
    for c in m.columns:
        s = m.state(c, c)
        assert s.xAvg == s.yAvg and s.ck == s.xMk == s.yMk


def test_empty_pair_is_none_and_its_metric_is_the_analyzers():
    case = Case(3, 50, 3, "all_null_column")
    states, _ = case_host_mirror(case)
    m = CorrelationMatrix(case.names, None, states, 0)
    assert m.state("c1", "c1") is None and m.state("c0", "c1") is None and m.state("c0", "c2") is not None
    assert m.metric("c0", "c1").value.isFailure == d.Correlation("c0", "c1").computeMetricFrom(None).value.isFailure
    assert math.isnan(m.matrix()[0, 1]) and m.counts()[1, 2] == 0.0


def test_persist_and_load_round_trip(tmp_path):
    _, m = _small_matrix("c1 > 0")
    provider = d.HdfsStateProvider(str(tmp_path / "states"))
    for a, s in m.states().items():
        provider.persist(a, s)
    for a, s in m.states().items():
        assert provider.load(a) == s
    other = d.CorrelationState(5.0, 1.0, 2.0, 0.5, 3.0, 4.0)
    assert m.state("c0", "c1").sum(other).n == m.state("c0", "c1").n + 5.0


# ---------------------------------------------------------------- the host mirror at the bar
def _check_mirror(case, keep=None, max_ranges=0):
    states, flags = case_host_mirror(case, keep, max_ranges)
    assert not flags.any(), np.nonzero(flags)
    for i, j in case.pairs():
        check_state("n=%d k=%d (%d,%d)" % (case.n, case.k, i, j), host_state(d, states, i, j, case.k),
                    case.exact(i, j, keep), who="mirror")
    return states


@pytest.mark.parametrize("n", ROW_COUNTS)
def test_mirror_row_counts(n):
    # (NULLs from 63 rows on: with a handful of rows a pair whose columns' shift rows are NULL in the
    # other column has nothing "ordinary" about it, and the guard may rightly send it to the pair kernel)
    _check_mirror(Case(2 if n > 4096 else 5, n, 100 + n, "five_percent" if n >= 63 and n % 2 else "none"))


@pytest.mark.parametrize("k", COLUMN_COUNTS)
def test_mirror_column_counts(k):
    _check_mirror(Case(k, SLAB + 1, 200 + k))


@pytest.mark.parametrize("nulls", NULL_PATTERNS)
def test_mirror_null_patterns(nulls):
    n = 3 * 4096 + 5
    case = Case(4, n, 300, nulls)
    _check_mirror(case)
    _check_mirror(case, keep=np.arange(n) % 2 == 0, max_ranges=3)


def test_mirror_2_18_rows_17_columns_and_ranges():
    case = Case(17, 1 << 18, 18, "five_percent")
    a = _check_mirror(case, max_ranges=0)
    b = case_host_mirror(case, max_ranges=512)[0]
    assert np.array_equal(a[:, 0], b[:, 0])  # n; the other fields depend on the merge tree


def test_mirror_small_case_against_the_oracle():
    """What the bar's NaN rule stands on: on a host-sized case the oracle's metric is NaN exactly where
    the exact state's is."""
    case = Case(4, 65, 11, "five_percent")
    case.values[2] = np.full(65, 7.0)  # a constant column: xMk = 0, the metric NaN
    case._centred = [None] * 4
    states = _check_mirror(case)
    for i, j in case.pairs():
        def col(c):
            return O.OColumn("float64", [float(v) if ok else None for v, ok in zip(case.values[c], case.valid[c])])
        o = O.correlation_state({"x": col(i), "y": col(j)} if i != j else {"x": col(i)}, "x", "y" if i != j else "x")
        got = host_state(d, states, i, j, 4)
        assert got.n == o.n and math.isnan(got.metricValue()) == math.isnan(o.metric_value()), (i, j)


# ---------------------------------------------------------------- fallback flags
def _flagged_pairs(k, col):
    return sorted(pair_index(min(i, col), max(i, col), k) for i in range(k))


def test_mirror_flags_exactly_the_outlier_columns_pairs():
    """+-1e8 on the first row of every slab of one column: its shift is an outlier, its k pairs (the
    diagonal included) fall back and still meet the bar; no other pair is flagged."""
    case = Case(5, 4 * SLAB + 17, 41)
    rows = np.arange(0, case.n, SLAB)
    case.values[2] = np.rint(case.values[2] / 2.0 ** 24 * 1024) / 1024  # values near 1: 1e8 is far out
    case.values[2][rows] = np.where((rows // SLAB) % 3 != 0, 1e8, -1e8)
    case.dtypes[2] = "float64"
    states, flags = case_host_mirror(case)
    assert sorted(np.nonzero(flags)[0].tolist()) == _flagged_pairs(5, 2)
    for i, j in case.pairs():
        check_state("outlier (%d,%d)" % (i, j), host_state(d, states, i, j, 5), case.exact(i, j), who="mirror")


@pytest.mark.parametrize("what", ["non_finite", "overflowing_squares"])
def test_mirror_flags_exactly_the_non_finite_columns_pairs(what):
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
    valid = [case.valid[i] if case.has_nulls(i) else None for i in range(4)]
    states, flags = host_corrmat(values, valid)
    assert sorted(np.nonzero(flags)[0].tolist()) == _flagged_pairs(4, 1)
    for i, j in case.pairs():
        got = host_state(d, states, i, j, 4)
        if 1 in (i, j):
            assert got.n == float((case.valid[i] & case.valid[j]).sum())
            if what == "overflowing_squares":  # finite values: Spark's per-row update answers, xMk = +Inf, no NaN but (1, 1)
                def col(c):
                    return O.OColumn("float64", [float(a) if ok else None for a, ok in zip(values[c], case.valid[c])])
                o = O.correlation_state({"x": col(i), "y": col(j)} if i != j else {"x": col(i)}, "x", "y" if i != j else "x")
                assert math.isnan(got.metricValue()) == math.isnan(o.metric_value()), (i, j, got, o.metric_value())
        else:
            check_state("%s (%d,%d)" % (what, i, j), got, case.exact(i, j), who="mirror")
