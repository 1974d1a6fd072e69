"""Row-level outcomes on the GPU (deequ_amd/rowlevel.py; dq_freq_probe_rows_kernel,
dq_rows_combine_kernel, dq_rows_select_*) against the independent restatement of
rowlevel_restated.py.  Every comparison is exact: outcomes row by row, the ascending indices of the
FALSE rows, the (TRUE, FALSE, NULL) counts, and both invariants -- count(TRUE) and count(non-NULL)
against the state AnalysisRunner saves for the same analyzer over the same data.  Every case runs
on host tables and on device-resident ones."""
import ctypes
import uuid

import numpy as np
import pytest

import deequ_amd as d
import pattern_cases as P
import rowlevel_restated as R
from deequ_amd import _lib as L
from deequ_amd.frequencies import FrequenciesAndNumRows, FrequencyTable
from helpers import oracle_table

pytestmark = pytest.mark.gpu

WHERE = "q > 0"  # TRUE, FALSE and NULL on some rows of every table below


# ---------------------------------------------------------------- helpers
def _cuts(n, batches):
    """Uneven batch bounds (5 : 3 : 4 for three batches), so that batches start inside a word."""
    if batches == 1 or n < batches:
        return [0, n]
    w = [5, 3, 4, 2, 6][:batches]
    acc, out = 0, [0]
    for x in w[:-1]:
        acc += x
        out.append(n * acc // sum(w))
    return sorted(set(out + [n]))


def _data(spec, batches=1, device=False):
    n = len(next(iter(spec.values()))[1])
    cuts = _cuts(n, batches)
    parts = [d.Table.from_pydict({c: (t, v[a:b]) for c, (t, v) in spec.items()}) for a, b in zip(cuts, cuts[1:])]
    if device:
        parts = [p.to_device(0) for p in parts]
    return parts[0] if len(parts) == 1 else d.PartitionedTable(parts)


def _restate(a, ot, state=None):
    if type(a) is d.Completeness:
        return R.completeness(ot, a.column, a.where)
    if type(a) is d.Compliance:
        return R.compliance(ot, a.predicate, a.where)
    if type(a) is d.PatternMatch:
        expected = [0 if s is None else P.oracle(a.pattern, s) for s in ot[a.column].values]
        return R.pattern_match(ot, a.column, expected, a.where)
    return R.uniqueness(ot, list(a.columns), a.where, state)


def _assert_outcome(res, a, want, device):
    assert res.to_pylist(a) == want, a
    assert res.counts(a) == R.counts(want), a
    failing = res.failing_rows(a)
    assert str(failing.dtype) == "torch.int64" and failing.is_cuda == device
    assert failing.tolist() == R.rows(want, False), a
    col = res.column(a)
    assert col.dtype == "bool" and col.device == device and col.length == len(want)
    assert col.to_pylist() == want, a


def _assert_invariants(res, analyzers, data):
    """The analyzer's state recomputed from .counts() equals the one AnalysisRunner saves."""
    saved = d.InMemoryStateProvider()
    d.AnalysisRunner.onData(data).addAnalyzers(analyzers).saveStatesWith(saved).run()
    for a in analyzers:
        t, f, _ = res.counts(a)
        st = saved.load(a)
        if type(a) is d.Uniqueness:
            assert (t, t + f) == (st.summary().num_unique, st.numRows), a
        elif st is None:  # (the aggregation over no selected row is NULL)
            assert t + f == 0, a
        else:
            assert d.NumMatchesAndCount(t, t + f) == st, (a, t, f, st)


def _check(spec, analyzers, batches=(1,), states=None, restate_state=None, invariants=True):
    ot = oracle_table(spec)
    wants = {a: _restate(a, ot, restate_state) for a in analyzers}
    for device in (False, True):
        for nb in batches:
            data = _data(spec, nb, device)
            res = d.row_level_results(data, analyzers, states=states)
            assert res.num_rows == len(next(iter(wants.values())))
            for a in analyzers:
                _assert_outcome(res, a, wants[a], device)
            if invariants:
                _assert_invariants(res, analyzers, data)


def _mixed_spec(n, seed=0):
    rng = np.random.default_rng(seed)
    ids = rng.integers(0, max(2, n // 2), n)
    words = ["abc", "abbbc", "ac", "xabcx", "", "é例abc", "nothing here", "ab"]
    return {
        "id": ("int64", [None if rng.random() < 0.1 else int(x) for x in ids]),
        "s": ("string", [None if rng.random() < 0.15 else words[int(k)] for k in rng.integers(0, len(words), n)]),
        "q": ("int64", [None if rng.random() < 0.2 else int(x) for x in rng.integers(-3, 6, n)]),
    }


ALL_FOUR = [d.Completeness("s"), d.Completeness("s", WHERE),
            d.Compliance("c", "q >= 3"), d.Compliance("c", "q >= 3", "id IS NOT NULL"),
            d.PatternMatch("s", r"ab+c"), d.PatternMatch("s", r"ab+c", WHERE),
            d.Uniqueness(["id"]), d.Uniqueness(["id"], WHERE)]


# ---------------------------------------------------------------- row counts
@pytest.mark.parametrize("n", [1, 63, 64, 65, 2047, 2048, 2049])
def test_row_counts_all_analyzers_with_and_without_where(gpu, n):
    """Completeness, Compliance, PatternMatch and Uniqueness, each with and without a `where` that
    is TRUE, FALSE and NULL on some rows; one batch, and three that start inside a word."""
    _check(_mixed_spec(n, seed=n), ALL_FOUR, batches=(1, 3))


def test_second_grid_stride_trip_of_the_probe_and_the_scatter(gpu):
    """2048 blocks x 4 words x 64 rows = 524 288 rows per trip of dq_freq_probe_rows_kernel's and of
    dq_rows_select_scatter_kernel's loop: 65 more rows give the first block's first two waves a
    second word (the last one ragged)."""
    n = 524_288 + 65
    rng = np.random.default_rng(7)
    ids = rng.integers(0, n, n).tolist()
    null = (rng.random(n) < 0.05).tolist()
    spec = {"id": ("int64", [None if z else x for x, z in zip(ids, null)])}
    _check(spec, [d.Uniqueness(["id"]), d.Completeness("id")])


def test_select_second_grid_stride_trip_of_the_count(gpu):
    """dq_rows_select_count_kernel takes one word per thread, 2048 x 256 words = 33 554 432 rows per
    trip: a bitmap pair of 65 rows more, checked against numpy for all three outcomes."""
    import torch
    n = 2048 * 256 * 64 + 65
    words = (n + 63) // 64
    g = torch.Generator(device="cuda").manual_seed(3)
    rnd = lambda: torch.randint(-2 ** 63, 2 ** 63 - 1, (words,), dtype=torch.int64, device="cuda", generator=g)  # noqa: E731
    value, valid = rnd(), rnd() & rnd() & rnd() & rnd()  # (sparse valid: short index lists)
    value[-1] = -1  # set bits past n in the last word must not be picked
    t = np.unpackbits(value.cpu().numpy().view(np.uint8), bitorder="little")[:n].astype(bool)
    v = np.unpackbits(valid.cpu().numpy().view(np.uint8), bitorder="little")[:n].astype(bool)
    torch.cuda.synchronize()
    ctx = L.Context.get(0).handle
    for which, want in ((L.DQ_ROWS_FALSE, np.flatnonzero(~t & v)), (L.DQ_ROWS_TRUE, np.flatnonzero(t & v)),
                        (L.DQ_ROWS_FALSE | L.DQ_ROWS_TRUE, np.flatnonzero(v))):
        got_n = ctypes.c_int64()
        st = L.lib().dq_rows_select(ctx, value.data_ptr(), valid.data_ptr(), n, which, None, 0, ctypes.byref(got_n))
        assert st == L.DQ_ERR_SPACE and got_n.value == len(want)
        out = torch.empty(len(want), dtype=torch.int64, device="cuda")
        L.check(L.lib().dq_rows_select(ctx, value.data_ptr(), valid.data_ptr(), n, which, out.data_ptr(), len(want),
                                       ctypes.byref(got_n)))
        assert got_n.value == len(want) and np.array_equal(out.cpu().numpy(), want)
    got_n = ctypes.c_int64()
    st = L.lib().dq_rows_select(ctx, value.data_ptr(), valid.data_ptr(), n, L.DQ_ROWS_NULL, None, 0, ctypes.byref(got_n))
    assert st == L.DQ_ERR_SPACE and got_n.value == int((~v).sum())


# ---------------------------------------------------------------- keys
def _nan(payload):
    import struct
    return struct.unpack("<d", struct.pack("<Q", 0x7FF8000000000000 | payload))[0]


def _key_spec(kind, n=300, seed=11):
    rng = np.random.default_rng(seed)
    pick = rng.integers(0, n // 2, n)  # about half the keys repeat
    null = lambda p=0.1: rng.random(n) < p  # noqa: E731
    q = ("int64", [None if z else int(x) for x, z in zip(rng.integers(-3, 6, n), null(0.2))])

    def col(dtype, make, nulls):
        return (dtype, [None if z else make(int(k)) for k, z in zip(pick, nulls)])
    floats = [0.0, -0.0, _nan(0), _nan(1), 1.5, -1.5, float("inf"), 2.0 ** -1074]
    makers = {
        "int64": ("int64", lambda k: k * 1_000_000_007 - 5),
        "int32": ("int32", lambda k: k - 40),
        "bool": ("bool", lambda k: k % 2 == 0),
        "float64": ("float64", lambda k: floats[k % len(floats)] if k % 3 else float(k)),
        "short": ("string", lambda k: ("", "a", "k%d" % k, "exactly-16-bytes", "é例%d" % k)[k % 5]),
        "long": ("string", lambda k: "a-grouping-key-longer-than-sixteen-bytes-%d" % k + "x" * (k % 40)),
        "digits12": ("string", lambda k: "%012d" % (k * 7919)),
        "uuid": ("string", lambda k: str(uuid.UUID(int=k * 0x9E3779B97F4A7C15 % 2 ** 128))),
    }
    if kind in makers:
        t, make = makers[kind]
        return {"k": col(t, make, null()), "q": q}, ["k"]
    if kind == "int64,int64":
        return {"a": col("int64", lambda k: k % 7, null()), "b": col("int64", lambda k: -k, null()), "q": q}, ["a", "b"]
    assert kind == "int64,utf8"
    return {"a": col("int64", lambda k: k % 5, null()),
            "b": col("string", lambda k: ("k%d" % k, "a-string-part-that-makes-the-key-long-%d" % k)[k % 2], null()),
            "q": q}, ["a", "b"]


KEY_KINDS = ["int64", "int32", "bool", "float64", "short", "long", "digits12", "uuid", "int64,int64", "int64,utf8"]


@pytest.mark.parametrize("kind", KEY_KINDS)
def test_key_types_null_keys_and_filters(gpu, kind):
    """Every key encoding, NULLs in each key column, with and without `where`; two batches."""
    spec, cols = _key_spec(kind)
    _check(spec, [d.Uniqueness(cols), d.Uniqueness(cols, WHERE)], batches=(1, 2))


@pytest.mark.parametrize("kind", ["int64", "long", "int64,utf8"])
def test_key_counts_per_row(gpu, kind):
    spec, cols = _key_spec(kind)
    ot = oracle_table(spec)
    groups = R.frequencies(ot, cols)
    want = [0 if k is None else groups[k] for k in R.keys_of(ot, cols)]
    a = d.Uniqueness(cols)
    for device in (False, True):
        res = d.row_level_results(_data(spec, 2, device), [a], key_counts=True)
        kc = res.key_counts(a)
        assert kc.is_cuda == device and kc.tolist() == want


@pytest.mark.parametrize("env", [{"DQ_FREQ_PATH": "sorted"}, {"DQ_FREQ_PATH": "atomic"},
                                 {"DQ_FREQ_PATH": "sorted", "DQ_FREQ_STAGE_BUDGET": "700"},
                                 {"DQ_FREQ_PATH": "atomic", "DQ_FREQ_STAGE_BUDGET": "700"},
                                 {"DQ_FREQ_PATH": "sorted", "DQ_FREQ_PART_MIN": "1"}],
                         ids=["sorted", "atomic", "sorted-budget", "atomic-budget", "partition"])
@pytest.mark.parametrize("kind", ["short", "long", "digits12", "uuid", "int64,int64", "int64,utf8"])
def test_every_group_by_path(gpu, monkeypatch, env, kind):
    """The table the probe reads, built by each group-by path: the sorted buckets, the per-row
    inserts, an aggregation in the middle of the batches, and the partition path with its packed
    digit, UUID, 16-byte and hashed records, chosen by the knobs test_gpu_freq_partition.py and
    test_gpu_freq_hashed.py use (a compacted table is expanded before the probe)."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    # (the partition path's record forms are chosen from samples of a large staging)
    spec, cols = _key_spec(kind, n=200_000 if "DQ_FREQ_PART_MIN" in env else 3000, seed=5)
    a = d.Uniqueness(cols)
    ot = oracle_table(spec)
    want = _restate(a, ot)
    data = _data(spec, 3, device=True)
    state = a.computeStateFrom(data)
    res = d.row_level_results(data, [a], states={a: state})
    _assert_outcome(res, a, want, True)
    t, f, _ = res.counts(a)
    assert (t, t + f) == (state.summary().num_unique, state.numRows)


# ---------------------------------------------------------------- layouts
def test_sliced_arrow_buffers_with_bit_offsets(gpu):
    """Arrow arrays sliced at rows that are no multiple of 8: validity and bool bitmaps start inside
    a byte, offsets and values past their first entry.  As host Tables, device Tables and through
    the Arrow C Data Interface's batches."""
    import pyarrow as pa
    spec = _mixed_spec(500, seed=2)
    rng = np.random.default_rng(4)
    spec["b"] = ("bool", [None if rng.random() < 0.1 else bool(x) for x in rng.integers(0, 2, 500)])
    types = {"int64": pa.int64(), "string": pa.string(), "bool": pa.bool_()}
    full = pa.table({c: pa.array(v, type=types[t]) for c, (t, v) in spec.items()})
    analyzers = ALL_FOUR + [d.Uniqueness(["b"]), d.Uniqueness(["id", "s"]), d.Compliance("b", "b")]
    for cuts in ([3, 500], [3, 77, 203, 497]):
        rows = cuts[-1] - cuts[0]
        sub = {c: (t, v[cuts[0]:cuts[-1]]) for c, (t, v) in spec.items()}
        ot = oracle_table(sub)
        wants = {a: _restate(a, ot) for a in analyzers}
        slices = [full.slice(a, b - a) for a, b in zip(cuts, cuts[1:])]
        host = [d.Table.from_arrow(s) for s in slices]
        assert all(c.offset % 8 for p in host for c in p.columns.values())
        for device, data in ((False, d.PartitionedTable(host)),
                             (True, d.PartitionedTable([p.to_device(0) for p in host])),
                             (False, d.ArrowTable([b for s in slices for b in s.to_batches()]))):
            res = d.row_level_results(data, analyzers)
            assert res.num_rows == rows
            for a in analyzers:
                _assert_outcome(res, a, wants[a], device)
            _assert_invariants(res, analyzers, data)


def test_column_without_validity_bitmap(gpu):
    spec = {"id": ("int64", [1, 2, 2, 3, 4, 4, 5] * 30), "s": ("string", ["abc", "x", "abbc", "", "c", "ab", "abc"] * 30),
            "q": ("int64", [1, -1, 2, 0, 3, -2, 4] * 30)}
    assert all(c.validity is None for c in _data(spec).columns.values())
    _check(spec, ALL_FOUR, batches=(1, 2))


def test_key_unique_in_each_batch_duplicated_across_batches(gpu):
    spec = {"id": ("int64", [1, 2, 3, 3, 4, 5])}
    a = d.Uniqueness(["id"])
    for device in (False, True):
        parts = [d.Table.from_pydict({"id": ("int64", v)}) for v in ([1, 2, 3], [3, 4, 5])]
        data = d.PartitionedTable([p.to_device(0) for p in parts] if device else parts)
        res = d.row_level_results(data, [a])
        assert res.to_pylist(a) == [True, True, False, False, True, True] == _restate(a, oracle_table(spec))
        assert res.failing_rows(a).tolist() == [2, 3]


# ---------------------------------------------------------------- other states
def test_merged_and_loaded_states(gpu):
    """"Unique within the union of partitions": partition A probed against State.sum of A's and B's
    states, and against the same state loaded through import_flat (export_flat's columns)."""
    a_spec, cols = _key_spec("short", n=400, seed=21)
    b_spec, _ = _key_spec("short", n=350, seed=22)
    a = d.Uniqueness(cols)
    union = R.frequencies(oracle_table(a_spec), cols) + R.frequencies(oracle_table(b_spec), cols)
    sa, sb = a.computeStateFrom(_data(a_spec, device=True)), a.computeStateFrom(_data(b_spec, device=True))
    merged = sa.sum(sb)
    counts, offs, blob = merged.table.export_flat()
    loaded = FrequencyTable(cols, {"k": "string"})
    loaded.import_flat(counts, offs, blob, merged.numRows)
    for state in (merged, FrequenciesAndNumRows(loaded)):
        _check(a_spec, [a], batches=(1, 2), states={a: state}, restate_state=union, invariants=False)
    # a key the state does not hold is FALSE: B's state alone, probed with A's rows
    _check(a_spec, [a], states={a: sb}, restate_state=R.frequencies(oracle_table(b_spec), cols), invariants=False)
    # a state loader (StateLoader.load) is taken like a dict
    saved = d.InMemoryStateProvider()
    saved.persist(a, merged)
    _check(a_spec, [a], states=saved, restate_state=union, invariants=False)


def test_empty_state_and_empty_selection(gpu):
    spec = {"id": ("int64", [None, None, None]), "q": ("int64", [1, None, -1])}
    _check(spec, [d.Uniqueness(["id"]), d.Uniqueness(["id"], WHERE), d.Completeness("id", "q > 100"),
                  d.Compliance("c", "id > 0", "q > 100")])


# ---------------------------------------------------------------- PatternMatch
@pytest.mark.parametrize("index", [0, 9, 14, 24, 25, 31])
def test_pattern_match_generated_inputs(gpu, index):
    pattern, strings = P.pattern_inputs(index, n=700)
    rng = np.random.default_rng(index)
    spec = {"s": ("string", [None if rng.random() < 0.1 else s for s in strings]),
            "q": ("int64", [None if rng.random() < 0.2 else int(x) for x in rng.integers(-3, 6, len(strings))])}
    _check(spec, [d.PatternMatch("s", pattern), d.PatternMatch("s", pattern, WHERE)], batches=(1, 3))


def test_pattern_match_java_line_terminator_cases(gpu):
    """The per-row answers pattern_cases.JAVA_LINE_CASES carries by hand (Python's re differs there)."""
    by_pattern = {}
    for pattern, text, want in P.JAVA_LINE_CASES:
        by_pattern.setdefault(pattern, []).append((text, want))
    for pattern, cases in by_pattern.items():
        texts = [t for t, _ in cases] + [None]
        ot = oracle_table({"s": ("string", texts)})
        want = R.pattern_match(ot, "s", [w for _, w in cases] + [1])
        a = d.PatternMatch("s", pattern)
        for device in (False, True):
            res = d.row_level_results(_data({"s": ("string", texts)}, device=device), [a])
            _assert_outcome(res, a, want, device)


# ---------------------------------------------------------------- refusals at the C-ABI
def test_histogram_table_and_unknown_ops_are_invalid(gpu):
    data = _data({"id": ("int64", [1, 1, None])}, device=True)
    hist = d.Histogram("id").computeStateFrom(data)
    a = d.Uniqueness(["id"])
    with pytest.raises(L.DeequAmdError) as e:
        d.row_level_results(data, [a], states={a: hist})
    assert e.value.status == L.DQ_ERR_INVALID
    import torch
    from deequ_amd.table import dq_columns
    out = torch.zeros(2, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    st = L.lib().dq_freq_probe_rows(hist.table.handle, dq_columns(data, hist.table.names), len(hist.table.names), 3,
                                    None, 0, out.data_ptr(), out[1:].data_ptr(), None)
    assert st == L.DQ_ERR_INVALID
    for kind in (L.DQ_OP_SIZE, L.DQ_OP_SUM, L.DQ_OP_APPROX_COUNT_DISTINCT, L.DQ_OP_DATATYPE, L.DQ_OP_MIN_LENGTH):
        op = (L.DqOp * 1)()
        op[0].kind, op[0].column, op[0].column2 = kind, 0, -1
        h = ctypes.c_void_p()
        types = (ctypes.c_int32 * 1)(L.DQ_T_INT64)
        assert L.lib().dq_rows_create(L.Context.get(0).handle, op, 1, types, 1, ctypes.byref(h)) == L.DQ_ERR_INVALID
        assert not h.value
