"""Cross-table checks on the GPU (deequ_amd/comparison.py; dq_freq_index_rows_kernel,
dq_freq_match_rows_kernel) against the independent restatement of match_restated.py.  Every
comparison is exact: outcomes row by row, the four counts, the ascending failing rows, the reference
rows, and both invariants -- count(TRUE) and count(non-NULL) are the state's numerator and
denominator.  Host and device-resident primary tables are both covered."""
import uuid
from collections import OrderedDict

import numpy as np
import pytest

import deequ_amd as d
import match_cases as C
import match_restated as M
import rowlevel_restated as R
from deequ_amd import _lib as L
from deequ_amd import comparison
from deequ_amd.frequencies import FrequenciesAndNumRows, FrequencyTable
from helpers import oracle_table

pytestmark = pytest.mark.gpu

WHERE = "q > 0"  # TRUE, FALSE and NULL on some rows of every primary table below


# ---------------------------------------------------------------- helpers
def _cuts(n, batches):
    """Uneven batch bounds (5 : 3 : 4 for three batches), so that batches start inside a word."""
    if batches == 1 or n < batches:
        return [0, n]
    w = [5, 3, 4][:batches]
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


def _assert_result(res, want, device, counts=None, ref_rows=None):
    n = len(want)
    assert res.num_rows == n
    assert res.to_pylist() == want
    t, f, _ = R.counts(want)
    assert res.state == (d.NumMatchesAndCount(t, t + f) if t + f else None)  # both invariants
    assert res.ratio == (t / (t + f) if t + f else None)
    c = res.counts
    assert c.matched == t and c.selected == t + f
    assert c.matched + c.key_null + c.key_absent + c.cells_differ == c.selected
    if counts is not None:
        assert c._asdict() == counts
    failing = res.failing_rows()
    assert str(failing.dtype) == "torch.int64" and failing.is_cuda == device
    assert failing.tolist() == R.rows(want, False)
    assert res.rows("true").tolist() == R.rows(want, True) and res.rows("null").tolist() == R.rows(want, None)
    col = res.column()
    assert col.dtype == "bool" and col.device == device and col.length == n and col.to_pylist() == want
    if ref_rows is not None:
        got = res.reference_rows()
        assert got.is_cuda == device and got.tolist() == ref_rows


def _check_match(a_spec, b_spec, keys, compare=(), where=None, batches=(1,), devices=(False, True)):
    pairs = comparison._pairs(keys, "keys")
    cmp_pairs = comparison._pairs(compare, "compare")
    a, b = oracle_table(a_spec), oracle_table(b_spec)
    want, counts = M.evaluate(a, b, pairs, cmp_pairs, where)
    refs = M.reference_rows(a, [x for x, _ in pairs], b, [y for _, y in pairs])
    for device in devices:
        for nb in batches:
            res = d.dataset_match(_data(a_spec, nb, device), _data(b_spec, 1, device), keys, compare, where=where,
                                  reference_rows=True)
            _assert_result(res, want, device, counts, refs)
    return want


def _check_ri(a_spec, b_spec, a_keys, b_keys=None, where=None, batches=(1,), devices=(False, True), b_batches=1):
    a, b = oracle_table(a_spec), oracle_table(b_spec)
    want = M.referential_integrity(a, a_keys, b, b_keys or a_keys, where)
    for device in devices:
        for nb in batches:
            res = d.referential_integrity(_data(a_spec, nb, device), a_keys, _data(b_spec, b_batches, device), b_keys,
                                          where=where)
            _assert_result(res, want, device)
    return want


def _int_tables(n_a, n_b=97, seed=0):
    """int64 keys: B's are unique (some rows have a NULL key); A's are B's, absent ones and NULLs."""
    rng = np.random.default_rng(seed)
    b_ids = [int(x) * 1_000_003 - 7 for x in rng.permutation(n_b)]
    b_null = rng.random(n_b) < 0.08
    b_v = [int(x) for x in rng.integers(-5, 5, n_b)]
    b_s = [("s%d" % x) * (1 + x % 4) for x in rng.integers(0, 9, n_b)]
    b = {"id": ("int64", [None if z else x for x, z in zip(b_ids, b_null)]),
         "v": ("int64", [None if rng.random() < 0.1 else x for x in b_v]),
         "s": ("string", [None if rng.random() < 0.1 else x for x in b_s])}
    pick = rng.integers(0, n_b + n_b // 4 + 1, n_a)  # (the top fifth names no row of B)
    a_ids, a_v, a_s = [], [], []
    for p in pick.tolist():
        if p < n_b:
            a_ids.append(b_ids[p])
            a_v.append(b["v"][1][p] if rng.random() < 0.8 else 99)
            a_s.append(b["s"][1][p] if rng.random() < 0.8 else "other")
        else:
            a_ids.append(-p)
            a_v.append(1)
            a_s.append("x")
    a = {"id": ("int64", [None if rng.random() < 0.1 else x for x in a_ids]), "v": ("int64", a_v), "s": ("string", a_s),
         "q": ("int64", [None if rng.random() < 0.2 else int(x) for x in rng.integers(-3, 6, n_a)])}
    return a, b


# ---------------------------------------------------------------- the worked example
def test_worked_example(gpu):
    T, F, N = True, False, None
    assert _check_ri(M.EXAMPLE_A, M.EXAMPLE_B, ["id"]) == [T, T, T, F, F, T]
    assert _check_match(M.EXAMPLE_A, M.EXAMPLE_B, ["id"], ["v", "s"]) == [T, T, T, F, F, F]
    assert _check_match(M.EXAMPLE_A, M.EXAMPLE_B, [("id", "id")], [("v", "v"), ("s", "s")], where="id < 9") == \
        [T, T, T, N, N, F]
    res = d.dataset_match(_data(M.EXAMPLE_A), _data(M.EXAMPLE_B), ["id"], ["v", "s"], reference_rows=True)
    assert res.state == d.NumMatchesAndCount(3, 6) and res.reference_rows().tolist() == [3, 2, 1, -1, -1, 0]
    assert res.counts == d.MatchCounts(3, 1, 1, 1, 6)
    assert d.referential_integrity(_data(M.EXAMPLE_A), ["id"], _data(M.EXAMPLE_B)).state == d.NumMatchesAndCount(4, 6)


# ---------------------------------------------------------------- row counts and batches
@pytest.mark.parametrize("n", [1, 63, 64, 65, 2049])
def test_row_counts_one_batch_and_three_inside_a_word(gpu, n):
    a, b = _int_tables(n, seed=n)
    for where in (None, WHERE):
        _check_match(a, b, ["id"], ["v", "s"], where=where, batches=(1, 3))
        _check_ri(a, b, ["id"], where=where, batches=(1, 3))


def test_second_grid_stride_trip_of_the_index_and_the_match(gpu):
    """2048 blocks x 4 words x 64 rows = 524 288 rows per trip of either kernel's loop: 65 more rows
    in A and in B give the first waves a second word, the last one ragged."""
    n = 524_288 + 65
    rng = np.random.default_rng(9)
    b_ids = (rng.permutation(n) * 3 + 1).tolist()
    b_v = rng.integers(0, 1000, n).tolist()
    pick = rng.integers(0, n, n)
    a_ids = np.where(rng.random(n) < 0.02, -1 - pick, np.asarray(b_ids)[pick]).tolist()
    a_v = np.where(rng.random(n) < 0.02, -5, np.asarray(b_v)[pick]).tolist()
    a = {"id": ("int64", [None if z else x for x, z in zip(a_ids, (rng.random(n) < 0.01).tolist())]), "v": ("int64", a_v)}
    b = {"id": ("int64", b_ids), "v": ("int64", b_v)}
    _check_match(a, b, ["id"], ["v"], devices=(True,))


# ---------------------------------------------------------------- key kinds
def _key_tables(kind, n_b=400, n_a=500, seed=3):
    rng = np.random.default_rng(seed)
    makers = {
        "int32": (["int32"], lambda k: (k * 37 - 4000,)),
        "int64": (["int64"], lambda k: (k * 1_000_000_007 - 5,)),
        "int64,int64": (["int64", "int64"], lambda k: (k % 7, -k)),
        "int64,utf8": (["int64", "string"],
                       lambda k: (k % 5, ("k%d" % k, "a-string-part-that-makes-the-key-long-%d" % k)[k % 2])),
        "digits12": (["string"], lambda k: ("%012d" % (k * 7919),)),
        "k11": (["string"], lambda k: ("k%011d" % (k * 7919),)),
        "uuid": (["string"], lambda k: (str(uuid.UUID(int=(k + 1) * 0x9E3779B97F4A7C15 % 2 ** 128)),)),
        "bytes40": (["string"], lambda k: (("%040d" % (k * 104729))[::-1],)),
        "empty": (["string"], lambda k: ("" if k == 0 else "e%d" % k,)),
    }
    dtypes, make = makers[kind]
    names = ["k%d" % i for i in range(len(dtypes))]
    order = rng.permutation(n_b).tolist()
    b_keys = [make(k) for k in order]
    b_null = (rng.random(n_b) < 0.05).tolist()
    b = {n: (t, [None if z and i == 0 else key[i] for key, z in zip(b_keys, b_null)])
         for i, (n, t) in enumerate(zip(names, dtypes))}
    b["v"] = ("int64", order)
    pick = rng.integers(0, n_b + n_b // 4, n_a).tolist()
    pick[0] = 0  # (the empty-string key is asked for)
    a_keys = [make(k) for k in pick]
    a = {n: (t, [None if rng.random() < 0.05 else key[i] for key in a_keys]) for i, (n, t) in enumerate(zip(names, dtypes))}
    a["v"] = ("int64", [k if rng.random() < 0.9 else -1 for k in pick])
    a["q"] = ("int64", [None if rng.random() < 0.2 else int(x) for x in rng.integers(-3, 6, n_a)])
    return a, b, names


KEY_KINDS = ["int32", "int64", "int64,int64", "int64,utf8", "digits12", "k11", "uuid", "bytes40", "empty"]


@pytest.mark.parametrize("env", [{"DQ_FREQ_PATH": "sorted"}, {"DQ_FREQ_PATH": "atomic"}], ids=["sorted", "atomic"])
@pytest.mark.parametrize("kind", KEY_KINDS)
def test_key_kinds_on_both_group_by_paths(gpu, monkeypatch, env, kind):
    """Every key encoding make_key has, the reference grouped by the sorted buckets (a compacted
    table, expanded before it is indexed) and by the per-row inserts (heap keys)."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    a, b, names = _key_tables(kind)
    _check_match(a, b, names, ["v"], batches=(2,))
    _check_match(a, b, names, ["v"], where=WHERE, devices=(True,))
    _check_ri(a, b, names, batches=(2,), b_batches=2)


@pytest.mark.parametrize("kind", ["digits12", "uuid", "int64,int64", "int64,utf8"])
def test_key_kinds_on_the_partition_path(gpu, monkeypatch, kind):
    """The partition path's packed, UUID, 16-byte and hashed records.  The record forms are chosen
    from samples of a large staging, and the slices are aggregated in LDS from 2^20 slots on: 300 000
    reference rows."""
    monkeypatch.setenv("DQ_FREQ_PATH", "sorted")
    monkeypatch.setenv("DQ_FREQ_PART_MIN", "1")
    a, b, names = _key_tables(kind, n_b=300_000, n_a=2000, seed=5)
    _check_match(a, b, names, ["v"], devices=(True,))
    table, _ = comparison._reference_table(_data(b, device=True), names, "test")  # (the table dataset_match builds)
    table.summary()
    paths = table.paths()
    flavour = {"digits12": "compacted", "uuid": "uuid_runs", "int64,int64": "raw16_runs", "int64,utf8": "hashed_runs"}
    assert paths[flavour[kind]] >= 1, sorted(paths.items())


def test_key_columns_of_other_names_and_order(gpu):
    """A's key columns are handed over in the order of B's, whatever they are called."""
    a, b, names = _key_tables("int64,utf8", n_b=120, n_a=150)
    a2 = OrderedDict([("q", a["q"]), ("text", a["k1"]), ("v", a["v"]), ("num", a["k0"])])
    want = M.dataset_match(oracle_table(a), oracle_table(b), [("k0", "k0"), ("k1", "k1")], [("v", "v")])
    for device in (False, True):
        res = d.dataset_match(_data(a2, 2, device), _data(b, 1, device), [("num", "k0"), ("text", "k1")], [("v", "v")])
        _assert_result(res, want, device)
        res = d.dataset_match(_data(a2, 2, device), _data(b, 1, device), [("text", "k1"), ("num", "k0")], ["v"])
        _assert_result(res, want, device)


# ---------------------------------------------------------------- compare columns
@pytest.mark.parametrize("dtype", C.DTYPES)
def test_compare_columns_every_pair_of_boundary_cells(gpu, dtype):
    """Row (i, j) of A holds cell i, the row of B with its key holds cell j: every pair of
    match_cases' boundary cells, NULLs on either side and on both.  B's rows are permuted, and its
    last row ends exactly at the end of its value buffer."""
    values = C.cells(dtype)
    m = len(values)
    n = m * m
    rng = np.random.default_rng(1)
    perm = rng.permutation(n).tolist()
    if dtype == "string":  # (the last row of B: a non-empty string)
        last = next(r for r in range(n) if values[r % m])
        perm.remove(last)
        perm.append(last)
    a_vals = [values[r // m] for r in range(n)]
    b_vals = [values[r % m] for r in perm]
    a_spec = {"k": ("int64", list(range(n))), "c": (dtype, a_vals)}
    b_spec = {"k": ("int64", perm), "c": (dtype, b_vals)}
    want = M.dataset_match(oracle_table(a_spec), oracle_table(b_spec), [("k", "k")], [("c", "c")])
    assert want == [M.cell_equal(values[r // m], values[r % m], dtype) for r in range(n)]
    bc = C.column(dtype, b_vals)
    if dtype == "string":
        end = int(bc.offsets[-1])
        bc = d.Column("string", n, np.ascontiguousarray(bc.values[:end]), bc.validity, offsets=bc.offsets)
        assert len(bc.values) == end and bc.offsets[n] - bc.offsets[n - 1] > 0
    a_tab = d.Table(OrderedDict([("k", d.Column.from_pylist(list(range(n)), "int64")), ("c", C.column(dtype, a_vals))]))
    b_tab = d.Table(OrderedDict([("k", d.Column.from_pylist(perm, "int64")), ("c", bc)]))
    inverse = {r: j for j, r in enumerate(perm)}
    for device in (False, True):
        res = d.dataset_match(a_tab.to_device(0) if device else a_tab, b_tab.to_device(0) if device else b_tab,
                              ["k"], ["c"], reference_rows=True)
        _assert_result(res, want, device, ref_rows=[inverse[r] for r in range(n)])


def test_several_compare_pairs_and_the_pair_limit(gpu):
    a, b = _int_tables(300, seed=4)
    _check_match(a, b, ["id"], ["s", "v", "s"], batches=(2,))
    _check_match(a, b, ["id"], ["v"] * 32, devices=(True,))


# ---------------------------------------------------------------- hostile buffers
@pytest.mark.parametrize("offset", [1, 7, 61])
def test_hostile_buffers_sliced_at_odd_offsets(gpu, offset):
    """NULL slots and rows outside the window hold NaN, extremes, set bits and non-empty strings; no
    verdict changes."""
    from hostile import hostile_table
    rng = np.random.default_rng(offset)
    n_b, n_a = 97, 203
    order = rng.permutation(n_b).tolist()
    nul = lambda vals, p=0.2: [None if rng.random() < p else v for v in vals]  # noqa: E731
    words = ["", "a", "seven..", "eight...", "nine.....", "exactly-16-bytes", "seventeen bytes..", "é例", "x" * 64]
    b_cols = {"k": order, "i": [k * 3 for k in order], "f": [float(k) if k % 5 else float("nan") for k in order],
              "b": [k % 2 == 0 for k in order], "s": [words[k % len(words)] for k in order]}
    pick = rng.integers(0, n_b + 20, n_a).tolist()
    a_cols = {"k": pick, "i": [k * 3 if k % 11 else -1 for k in pick],
              "f": [float(k) if k % 5 else float("nan") for k in pick],
              "b": [k % 2 == 0 for k in pick], "s": [words[(k + (k % 13 == 0)) % len(words)] for k in pick]}
    types = {"k": "int64", "i": "int32", "f": "float64", "b": "bool", "s": "string"}
    b_spec = {c: (types[c], nul(v, 0.05 if c == "k" else 0.2)) for c, v in b_cols.items()}
    a_spec = {c: (types[c], nul(v, 0.05 if c == "k" else 0.2)) for c, v in a_cols.items()}
    cmp_pairs = [(c, c) for c in ("i", "f", "b", "s")]
    a, b = oracle_table(a_spec), oracle_table(b_spec)
    want = M.dataset_match(a, b, [("k", "k")], cmp_pairs)
    counts = M.counts(a, b, [("k", "k")], cmp_pairs)
    refs = M.reference_rows(a, ["k"], b, ["k"])
    offs = {c: (offset, 7, 61, 1, offset)[i] for i, c in enumerate(types)}
    for device in (False, True):
        for flavour in ("digits", "high"):
            at = hostile_table({c: list(v) for c, v in a_spec.items()}, offset=offs, device=device, flavour=flavour)
            bt = hostile_table({c: list(v) for c, v in b_spec.items()}, offset=offs, device=device, flavour=flavour)
            res = d.dataset_match(at, bt, ["k"], ["i", "f", "b", "s"], reference_rows=True)
            _assert_result(res, want, device, counts, refs)
            _assert_result(d.referential_integrity(at, ["k"], bt), M.referential_integrity(a, ["k"], b), device)


def test_arrow_batches_sliced_inside_a_byte(gpu):
    import pyarrow as pa
    a, b = _int_tables(500, seed=6)
    types = {"int64": pa.int64(), "string": pa.string()}
    full = pa.table({c: pa.array(v, type=types[t]) for c, (t, v) in a.items()})
    cuts = [3, 77, 203, 497]
    sub = {c: (t, v[3:497]) for c, (t, v) in a.items()}
    data = d.ArrowTable([x for lo, hi in zip(cuts, cuts[1:]) for x in full.slice(lo, hi - lo).to_batches()])
    want = M.dataset_match(oracle_table(sub), oracle_table(b), [("id", "id")], [("v", "v"), ("s", "s")], WHERE)
    res = d.dataset_match(data, _data(b), ["id"], ["v", "s"], where=WHERE)
    _assert_result(res, want, False)


# ---------------------------------------------------------------- reference-side conditions
def test_duplicate_and_null_keys_in_the_reference(gpu):
    a = {"k": ("int64", [1, 2, None, 3])}
    dup = {"k": ("int64", [1, 1, 2, None, None, 5, 5, 5])}
    for device in (False, True):
        with pytest.raises(ValueError, match="2 keys"):
            d.dataset_match(_data(a, 1, device), _data(dup, 1, device), ["k"])
    _check_ri(a, dup, ["k"])
    nulls = {"k": ("int64", [None, 2, None, None])}  # (NULL-key rows are unreachable, and allowed)
    assert _check_match(a, nulls, ["k"]) == [False, True, False, False]


def test_empty_tables(gpu):
    a = {"k": ("int64", [1, None, 3]), "v": ("string", ["a", "b", None])}
    empty = {"k": ("int64", []), "v": ("string", [])}
    assert _check_match(a, empty, ["k"], ["v"]) == [False, False, False]
    assert _check_ri(a, empty, ["k"]) == [False, False, False]
    assert _check_match(empty, a, ["k"], ["v"]) == []
    assert _check_ri(empty, a, ["k"]) == []
    res = d.dataset_match(_data(a), _data(a), ["k"], ["v"], where="k > 100")  # (no row selected)
    assert res.state is None and res.ratio is None and res.to_pylist() == [None] * 3


def test_loaded_and_merged_reference_states(gpu):
    """referential_integrity against the keys alone: a state merged from two partitions (State.sum)
    and the same state loaded through import_flat; no reference table is at hand."""
    a, b1, names = _key_tables("int64,utf8", n_b=150, n_a=300, seed=8)
    _, b2, _ = _key_tables("int64,utf8", n_b=220, n_a=1, seed=9)
    ob = oracle_table({c: (t, v + b2[c][1]) for c, (t, v) in b1.items()})
    groups = R.frequencies(ob, names)
    an = d.Uniqueness(names)
    merged = an.computeStateFrom(_data(b1, device=True)).sum(an.computeStateFrom(_data(b2, device=True)))
    counts, offs, blob = merged.table.export_flat()
    loaded = FrequencyTable(names, {"k0": "int64", "k1": "string"})
    loaded.import_flat(counts, offs, blob, merged.numRows)
    for where in (None, WHERE):
        want = M.referential_integrity(oracle_table(a), names, state=groups, where=where)
        assert want == M.referential_integrity(oracle_table(a), names, ob, names, where)
        for state in (merged, FrequenciesAndNumRows(loaded)):
            for device in (False, True):
                res = d.referential_integrity(_data(a, 2, device), names, reference_state=state, where=where)
                _assert_result(res, want, device)


def test_histogram_state_and_table_are_invalid(gpu):
    import torch
    from deequ_amd.table import dq_columns
    data = _data({"id": ("int64", [1, 1, None])}, device=True)
    hist = d.Histogram("id").computeStateFrom(data)
    with pytest.raises(L.DeequAmdError) as e:
        d.referential_integrity(data, ["id"], reference_state=hist)
    assert e.value.status == L.DQ_ERR_INVALID
    out = torch.zeros(2, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    cols = dq_columns(data, hist.table.names)
    lib = L.lib()
    assert lib.dq_freq_index_rows(hist.table.handle, cols, len(hist.table.names), 3, 0) == L.DQ_ERR_INVALID
    assert lib.dq_freq_match_rows(hist.table.handle, cols, len(hist.table.names), 3, None, 0, out.data_ptr(),
                                  out[1:].data_ptr(), None, None, 0, 0, None, None) == L.DQ_ERR_INVALID


def test_consume_drops_the_index_and_the_next_one_answers_right(gpu):
    """The index belongs to the table as it was: after another consume a match that follows it is
    DQ_ERR_STATE until the rows are indexed again, and then answers for the grown table.  A batch
    the table was not built from is DQ_ERR_STATE too."""
    from deequ_amd.table import dq_columns
    a, b, _ = _key_tables("digits12", n_b=300, n_a=400, seed=12)
    half = {c: (t, v[:150]) for c, (t, v) in b.items()}
    first, whole = _data(half, device=True), _data(b, device=True)
    a_dev = _data(a, device=True)
    table, on_dev = comparison._reference_table(first, ["k0"], "test")
    comparison._index(table, comparison._as_table(on_dev, ["k0"]))
    args = (a_dev, table, ["k0"], ["k0"], [("v", "v")])
    res = comparison._match(*args, on_dev, None, True)
    oa = oracle_table(a)
    _assert_result(res, M.dataset_match(oa, oracle_table(half), [("k0", "k0")], [("v", "v")]), True,
                   ref_rows=M.reference_rows(oa, ["k0"], oracle_table(half), ["k0"]))
    rest = _data({c: (t, v[150:]) for c, (t, v) in b.items()}, device=True)
    keys_only = comparison._as_table(whole, ["k0"])
    # (the second half is not in the table yet: indexing the whole reference is refused)
    st = L.lib().dq_freq_index_rows(table.handle, dq_columns(keys_only, table.names), 1, keys_only.num_rows, 0)
    assert st == L.DQ_ERR_STATE
    comparison._index(table, comparison._as_table(on_dev, ["k0"]))
    table.consume(comparison._as_table(rest, ["k0"]))
    with pytest.raises(L.DeequAmdError) as e:
        comparison._match(*args, whole, None, True)
    assert e.value.status == L.DQ_ERR_STATE
    comparison._index(table, keys_only)
    res = comparison._match(*args, whole, None, True)
    _assert_result(res, M.dataset_match(oa, oracle_table(b), [("k0", "k0")], [("v", "v")]), True,
                   ref_rows=M.reference_rows(oa, ["k0"], oracle_table(b), ["k0"]))


# ---------------------------------------------------------------- equivalence with the row-level probe
@pytest.mark.parametrize("kind", ["int64", "int64,utf8", "bytes40"])
def test_referential_integrity_is_key_count_above_zero(gpu, kind):
    a, b, names = _key_tables(kind, seed=14)
    an = d.Uniqueness(names)
    for device in (False, True):
        data = _data(a, 2, device)
        state = an.computeStateFrom(_data({c: b[c] for c in names}, device=True))
        probe = d.row_level_results(data, [an], states={an: state}, key_counts=True)
        res = d.referential_integrity(data, names, reference_state=state)
        assert res.to_pylist() == [c > 0 for c in probe.key_counts(an).tolist()]
