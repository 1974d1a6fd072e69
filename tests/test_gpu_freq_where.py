"""`where` on the frequency group-by (dq_freq_set_filter) on the GPU.

`A(columns, where=w)` has the state `A(columns)` has on `data.filter(w)`.  The independent
reference is the unchanged oracle on physically filtered rows:

    keep = [v is True for v in O.eval_predicate(w, ot)]
    want = O.frequencies_state(<ot restricted to keep>, cols)

(`LIKE` / `RLIKE` verdicts come from like_cases.verdict, the suite's reference for them: the
oracle's predicate grammar has neither.)  Groups, counts, numRows, #groups, #unique and the grouped
rows are compared exactly, entropy as test_gpu_frequencies.py compares it (1e-12 relative).

A filtered-out row is a NULL key to every stage and to the probes that sample a batch's keys (the
packed-digit probe, the key-length probe, the UUID probe: each skips the rows whose bit is clear in
the first key column's validity, which is the folded bitmap), so a dropped row steers no probe: the
path test asserts per case the record form an unfiltered run over the kept rows alone would take.
"""
import ctypes
import os
import socket
import uuid

import numpy as np
import pytest

import deequ_amd as d
import hostile as H
import like_cases as K
import pyoracle as O
from deequ_amd import _lib as L
from deequ_amd.engine import _fill_pred, _pred_array, schema_index
from deequ_amd.frequencies import FrequenciesAndNumRows, FrequencyTable, encode_key
from deequ_amd.predicates import UnsupportedPredicate, compile_predicate
from helpers import oracle_metric, oracle_table, rel_err
from test_gpu_frequencies import TOL, _product_freqs
from test_gpu_pred_generated import NAMES, SCHEMA, _spec, _texts, _verdicts

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NS = (1, 63, 64, 65, 2049)
_LIKE = {"s LIKE 'k%'": ("like", "k%"), "s LIKE '%.%'": ("like", "%.%"), "s RLIKE '^[0-9]+$'": ("rlike", "^[0-9]+$")}
HAND = [
    "l > 3",                             # the form the fused scan evaluates inline
    "l > 0 AND (d < 2.5 OR i IS NULL)",  # three terms
    "COALESCE(i, 4) >= 4",
    "i <= 3", "s > '3'",                 # a filter on a key column itself (groupings i, s and l, s)
    "s LIKE 'k%'", "s LIKE '%.%'", "s RLIKE '^[0-9]+$'",
    "d > 0.5", "b",                      # NULL verdicts on the rows where d / b is NULL
    "FALSE", "TRUE",
]
GROUPINGS = (["i"], ["s"], ["l", "s"], ["d"])


def _generated():
    texts = [t for t, _ in _texts("numeric")[:40]]
    assert len(texts) == 40
    return texts


def _keep(key, where, ot):
    """The rows `where` selects: its verdict is TRUE (FALSE and NULL drop the row)."""
    if where in _LIKE:
        kind, pattern = _LIKE[where]
        return [K.verdict(kind, pattern, v) is True for v in ot["s"].values]
    return [v is True for v in _verdicts(key, where, ot)]


def _restrict(ot, keep):
    return {k: O.OColumn(c.dtype, [v for v, kp in zip(c.values, keep) if kp]) for k, c in ot.items()}


def _check(table, ostate):
    state = FrequenciesAndNumRows(table)
    s = state.summary()
    assert s.num_rows == ostate.num_rows
    assert _product_freqs(state) == ostate.frequencies
    assert s.num_groups == len(ostate.frequencies)
    assert s.num_unique == sum(1 for c in ostate.frequencies.values() if c == 1)
    assert s.grouped_rows == sum(ostate.frequencies.values())
    if ostate.frequencies:
        assert rel_err(s.entropy, O.entropy_exact(ostate)) <= TOL


def _table(spec):
    return d.Table.from_pydict({k: (v[0], v[1]) for k, v in spec.items()})


# ---------------------------------------------------------------- 1. verdict shapes
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("n", NS)
def test_filtered_state_is_the_state_of_the_filtered_rows(gpu, n, device):
    spec, ot = _spec(n)
    batch = _table(spec).to_device(0) if device else _table(spec)
    cases = [(w, cols) for w in HAND + _generated() for cols in GROUPINGS] + [("l IS NULL", ["l"])]
    for where, cols in cases:
        want = O.frequencies_state(_restrict(ot, _keep(n, where, ot)), cols)
        t = FrequencyTable(cols, SCHEMA, where=where)
        try:
            t.consume(batch)
            _check(t, want)
        except AssertionError as e:
            raise AssertionError("where=%r cols=%r: %s" % (where, cols, e))
        finally:
            t.close()
    if n >= 64:  # everything selected by `l IS NULL` has a NULL key: rows, no groups
        want = O.frequencies_state(_restrict(ot, _keep(n, "l IS NULL", ot)), ["l"])
        assert want.num_rows > 0 and not want.frequencies


# ---------------------------------------------------------------- 2. every group-by path
N_PATH = 20000


def _path_data(shape):
    """(schema, {column: values}, key columns, where): the filter `v > 0` keeps about half of the
    rows; among the dropped ones are keys that would change the path's own probes."""
    rng = np.random.default_rng(41)
    v = [None if i % 29 == 0 else int(x) for i, x in enumerate(rng.integers(-1000, 1000, N_PATH))]
    a = rng.integers(0, N_PATH // 3, N_PATH)
    dropped = [x is None or x <= 0 for x in v]
    odd = [dr and i % 7 == 0 for i, dr in enumerate(dropped)]  # dropped rows with a key of another kind
    cols = {"v": ("int64", v)}
    if shape == "int64":
        cols["k"] = ("int64", [None if i % 19 == 0 else int(a[i]) for i in range(N_PATH)])
        keys = ["k"]
    elif shape == "digits12":  # dropped: a non-digit string among digit keys
        cols["k"] = ("string", ["id-%d-x" % a[i] if odd[i] else None if i % 19 == 0 else "%012d" % a[i]
                                for i in range(N_PATH)])
        keys = ["k"]
    elif shape == "kdigits":  # dropped: a key of 16 or more bytes among short keys
        cols["k"] = ("string", ["k%d-%s" % (a[i], "y" * 20) if odd[i] else None if i % 19 == 0 else "k%d" % a[i]
                                for i in range(N_PATH)])
        keys = ["k"]
    elif shape == "uuid":  # dropped: a malformed UUID among canonical UUIDs
        ids = [str(uuid.UUID(int=int(x) * 0x9E3779B97F4A7C15 % (1 << 128))) for x in range(N_PATH // 3)]
        cols["k"] = ("string", [ids[a[i]][:-1] + "g" if odd[i] else None if i % 19 == 0 else ids[a[i]]
                                for i in range(N_PATH)])
        keys = ["k"]
    elif shape == "int64x2":
        cols["k"] = ("int64", [None if i % 19 == 0 else int(a[i] % 500) for i in range(N_PATH)])
        cols["k2"] = ("int64", [None if i % 23 == 0 else int(a[i] % 37) for i in range(N_PATH)])
        keys = ["k", "k2"]
    elif shape == "int64_longstr":
        cols["k"] = ("int64", [None if i % 19 == 0 else int(a[i] % 500) for i in range(N_PATH)])
        cols["k2"] = ("string", [None if i % 23 == 0 else "a-long-string-side-%04d" % (a[i] % 37) for i in range(N_PATH)])
        keys = ["k", "k2"]
    else:  # strings longer than 15 bytes
        cols["k"] = ("string", [None if i % 19 == 0 else "long-key-value-%07d" % a[i] for i in range(N_PATH)])
        keys = ["k"]
    return cols, keys, "v > 0"


_PATH_REF = {}


def _path_ref(shape):
    if shape not in _PATH_REF:
        cols, keys, where = _path_data(shape)
        ot = {k: O.OColumn(t, list(vals)) for k, (t, vals) in cols.items()}
        keep = [x is True for x in O.eval_predicate(where, ot)]
        assert 0.4 < sum(keep) / N_PATH < 0.6
        _PATH_REF[shape] = (cols, keys, where, O.frequencies_state(_restrict(ot, keep), keys))
    return _PATH_REF[shape]


# (shape, environment, the paths() counter that says the intended path ran)
# _WIDE: a table of 2^20 slots, one slice per level-1 region, at which the partition passes
# aggregate the regions' records -- packed digits, hashed, UUID, raw 16-byte -- in LDS (as
# tests/test_gpu_freq_hashed.py and tests/test_gpu_hostile_freq.py force it); a smaller table lays
# the regions out contiguously again before it aggregates, whatever their records
_WIDE = {"DQ_FREQ_PATH": "sorted", "DQ_FREQ_PART_MIN": "1", "DQ_FREQ_PART_SLOTS": str(1 << 20)}
PATH_CASES = [
    ("int64", {"DQ_FREQ_PATH": "sorted", "DQ_FREQ_PART": "0"}, "sort_records"),
    ("int64", {"DQ_FREQ_PATH": "sorted", "DQ_FREQ_PART": "0", "DQ_FREQ_STAGE_BUDGET": "3000"}, "sort_records"),
    ("int64", {"DQ_FREQ_PATH": "sorted", "DQ_FREQ_PART_MIN": "1"}, "partition_runs"),
    ("int64", {"DQ_FREQ_PATH": "sorted", "DQ_FREQ_PART_MIN": "1", "DQ_FREQ_STAGE_BUDGET": "3000"}, "partition_runs"),
    ("int64", {"DQ_FREQ_PATH": "atomic"}, None),
    ("int64x2", {"DQ_FREQ_PATH": "atomic"}, None),
    ("kdigits", {"DQ_FREQ_PATH": "sorted", "DQ_FREQ_PART": "0"}, "sort_records"),
    ("kdigits", {"DQ_FREQ_PATH": "sorted", "DQ_FREQ_PART_MIN": "1"}, "partition_runs"),
    ("digits12", dict(_WIDE), "packed_runs"),
    ("uuid", dict(_WIDE), "uuid_runs"),
    ("int64x2", dict(_WIDE), "raw16_runs"),
    ("int64_longstr", dict(_WIDE), "hashed_runs"),
    ("longstr", dict(_WIDE), "hashed_runs"),
    ("longstr", {"DQ_FREQ_PATH": "sorted", "DQ_FREQ_PART": "0"}, None),
]


@pytest.mark.parametrize("shape,env,counter", PATH_CASES,
                         ids=["%s-%s" % (c[0], "-".join(v for v in c[1].values())) for c in PATH_CASES])
def test_filter_on_every_path(gpu, monkeypatch, shape, env, counter):
    """20 000 rows in 4 batches, `v > 0`.  The counter named per case must show the intended path.
    A dropped row is invalid in the folded bitmap, and the probes and stages skip invalid rows, so
    the dropped keys of another kind steer nothing: the non-digit keys leave the packed 8-byte
    records of `digits12` (packed_runs), the malformed UUIDs the UUID records (uuid_runs), the keys
    of 36 bytes the 16-byte records of `kdigits` (sort_records / partition_runs, no hashed run and
    no roll-back to the general path)."""
    for k, val in env.items():
        monkeypatch.setenv(k, val)
    cols, keys, where, want = _path_ref(shape)
    schema = {k: t for k, (t, _) in cols.items()}
    t = FrequencyTable(keys, schema, where=where)
    try:
        step = N_PATH // 4
        for s in range(0, N_PATH, step):
            t.consume(d.Table.from_pydict({k: (ty, vals[s:s + step]) for k, (ty, vals) in cols.items()}))
        _check(t, want)
        p = t.paths()
        assert p["wait_timeouts"] == 0, p
        if shape == "kdigits":
            assert p["hashed_runs"] == 0 and p["hashed_inserts"] == 0, p
        if counter:
            assert p[counter] >= 1, p
        elif env.get("DQ_FREQ_PATH") == "atomic":
            assert p["sort_records"] == 0 and p["partition_runs"] == 0 and p["hashed_runs"] == 0, p
    finally:
        t.close()


def test_filter_on_the_few_groups_path(gpu):
    """The few-groups kernel (dq_freq_expect_groups): 37 groups, and a DQ_FREQ_FEW_ONLY table whose
    dropped rows alone hold more keys than the kernel takes -- it must not fail."""
    rng = np.random.default_rng(43)
    v = [None if i % 29 == 0 else int(x) for i, x in enumerate(rng.integers(-1000, 1000, N_PATH))]
    k = [None if i % 19 == 0 else (int(i) + 1000 if (x is None or x <= 0) else int(i % 37)) for i, x in enumerate(v)]
    cols = {"k": ("int64", k), "v": ("int64", v)}
    ot = {c: O.OColumn(t, list(vals)) for c, (t, vals) in cols.items()}
    want = O.frequencies_state(_restrict(ot, [x is True for x in O.eval_predicate("v > 0", ot)]), ["k"])
    assert len(want.frequencies) == 37
    schema = {"k": "int64", "v": "int64"}
    for few_only in (False, True):
        t = FrequencyTable(["k"], schema, few_only=few_only, where="v > 0")
        try:
            t.expect_groups(64)
            for s in range(0, N_PATH, N_PATH // 4):
                t.consume(d.Table.from_pydict({c: (ty, vals[s:s + N_PATH // 4]) for c, (ty, vals) in cols.items()}))
            _check(t, want)
            assert t.paths()["small_runs"] >= 4, t.paths()
        finally:
            t.close()


# ---------------------------------------------------------------- 3. second grid-stride trip
def test_filter_kernel_second_grid_stride_trip(gpu):
    """2048 blocks x 4 words x 64 rows = 524 288 rows per trip of dq_freq_filter_kernel's loop: 65
    more rows give the first block's first two waves a second word (the last one ragged)."""
    n = 524_288 + 65
    rng = np.random.default_rng(47)
    k = np.arange(n, dtype=np.int64) % 1000
    v = rng.integers(-50, 50, n).astype(np.int64)
    valid = rng.random(n) >= 0.03
    table = d.Table({"k": d.Column.from_numpy(k, None, "int64"),
                     "v": d.Column.from_numpy(v, valid, "int64")}).to_device(0)
    keep = valid & (v >= 0)
    uniq, counts = np.unique(k[keep], return_counts=True)
    t = FrequencyTable(["k"], {"k": "int64", "v": "int64"}, where="v >= 0")
    try:
        t.consume(table)
        s = t.summary()
        assert s.num_rows == int(keep.sum()) and s.grouped_rows == int(keep.sum())
        assert s.num_groups == len(uniq) and s.num_unique == int((counts == 1).sum())
        got_counts, got_keys = t.export()
        got = {int.from_bytes(key, "little", signed=True): int(c) for key, c in zip(got_keys, got_counts.tolist())}
        assert got == {int(a): int(c) for a, c in zip(uniq, counts)}
    finally:
        t.close()


# ---------------------------------------------------------------- 4. hostile buffers
@pytest.mark.parametrize("flavour,shift", [("digits", 0), ("high", 1), ("text", 2)])
def test_filter_on_hostile_sliced_columns(gpu, flavour, shift):
    """2049 rows on the device, every column sliced at one of the offsets 1, 7, 61, 2051 in hostile
    buffers: NULL slots -- and so the rows the filter drops through a NULL verdict -- hold NaN,
    +-Inf, INT_MAX and non-empty strings, and the filtered-out valid rows hold real values that
    must reach no group either."""
    spec, ot = _spec(2049)
    offs = (1, 7, 61, 2051)
    offsets = {nm: offs[(j + shift) % 4] for j, nm in enumerate(NAMES)}
    batch = H.hostile_table(spec, offset=offsets, device=True, flavour=flavour)
    for nm in NAMES:
        assert batch.columns[nm].offset == offsets[nm] and batch.columns[nm].validity is not None
    for where in ("d > 0.5", "l > 0 AND (d < 2.5 OR i IS NULL)", "s > '3'", "s LIKE '%.%'", "COALESCE(i, 4) >= 4", "b"):
        for cols in GROUPINGS:
            want = O.frequencies_state(_restrict(ot, _keep(2049, where, ot)), cols)
            t = FrequencyTable(cols, SCHEMA, where=where)
            try:
                t.consume(batch)
                _check(t, want)
            finally:
                t.close()


def test_filter_when_the_first_key_has_no_bitmap(gpu):
    """The fold writes the TRUE word alone: key columns without validity (host and device, a key
    column sliced at an odd offset), the filter column hostile."""
    spec, ot = _spec(2049)
    keys = {"k": ["int64", [int(v % 97) for v in range(2049)]], "k2": ["string", ["g%d" % (v % 11) for v in range(2049)]]}
    ot2 = dict(ot, **oracle_table(keys))
    schema = dict(SCHEMA, k="int64", k2="string")
    for device in (False, True):
        cols = dict(H.hostile_table(spec, offset=7, device=device, flavour="digits").columns)
        whole = np.arange(-5, 2049 + 5, dtype=np.int64) % 97  # row r at index r + 5
        kc = d.Column("int64", 2049, whole, None, None, offset=5, device=False)
        data = [v.encode() for v in keys["k2"][1]]
        k2offs = np.zeros(2049 + 1, dtype=np.int32)
        np.cumsum([len(x) for x in data], out=k2offs[1:])
        k2 = d.Column("string", 2049, np.frombuffer(b"".join(data) + b"\0" * 8, dtype=np.uint8), None, offsets=k2offs)
        assert k2.validity is None and kc.validity is None
        cols["k"] = kc.to_device(0) if device else kc
        cols["k2"] = k2.to_device(0) if device else k2
        batch = d.Table(cols)
        for where in ("d > 0.5", "b", "l IS NULL"):
            for group in (["k"], ["k", "k2"], ["k2"]):
                want = O.frequencies_state(_restrict(ot2, _keep(2049, where, ot)), group)
                t = FrequencyTable(group, schema, where=where)
                try:
                    t.consume(batch)
                    _check(t, want)
                finally:
                    t.close()


# ---------------------------------------------------------------- 5. two batches, one table, reset
def test_two_batches_then_reset(gpu):
    (s1, o1), (s2, o2) = _spec(65), _spec(2049)
    both = oracle_table({k: [s1[k][0], s1[k][1] + s2[k][1]] for k in NAMES})
    t1, t2 = _table(s1), _table(s2).to_device(0)
    for where in ("l > 3", "d > 0.5", "s RLIKE '^[0-9]+$'"):
        keep = _keep(65, where, o1) + _keep(2049, where, o2)
        for cols in GROUPINGS:
            want = O.frequencies_state(_restrict(both, keep), cols)
            t = FrequencyTable(cols, SCHEMA, where=where)
            try:
                for _ in range(2):  # the filter survives dq_freq_reset
                    t.consume(t1)
                    t.consume(t2)
                    _check(t, want)
                    t.reset()
                    assert t.summary().num_rows == 0 and t.summary().num_groups == 0
            finally:
                t.close()


# ---------------------------------------------------------------- 6. through the public API
def _metric(ctx, a):
    v = ctx.metric(a).value
    return v.get() if v.is_success() else "failure"


def _oracle_value(a, ot, key):
    name = type(a).__name__
    sub = _restrict(ot, _keep(key, a.where, ot)) if a.where else ot
    cols = [a.column] if name == "Entropy" else list(a.columns)
    return oracle_metric(O.frequencies_state(sub, cols), name, [cols])


def _close(got, want):
    if isinstance(want, float) and isinstance(got, float):
        return got == want or rel_err(got, want) <= TOL
    return got == want


def test_runner_shares_tables_by_columns_and_where(gpu, monkeypatch):
    spec, ot = _spec(2049)
    table = _table(spec).to_device(0)
    analyzers = [d.Uniqueness(["s"]), d.Uniqueness(["s"], "l > 0"), d.Distinctness(["s"], "l > 0"),
                 d.Entropy("s", "l > 0"), d.CountDistinct(["s"], "l <= 0"),
                 d.MutualInformation(["s", "i"], where="l > 0"), d.Histogram("s")]
    lib = L.lib()
    real, created = lib.dq_freq_create, []

    def counting(*args):
        created.append(args)
        return real(*args)

    monkeypatch.setattr(lib, "dq_freq_create", counting)
    ctx = d.AnalysisRunner.onData(table).addAnalyzers(analyzers).run()
    monkeypatch.setattr(lib, "dq_freq_create", real)
    # exactly three tables over `s`: (s, None) -- which the Histogram shares --, (s, l > 0) and
    # (s, l <= 0); MutualInformation groups two columns, so its joint table (i s, l > 0) is one more
    assert [c[2] for c in created].count(1) == 3 and len(created) == 4, [c[2] for c in created]
    for a in analyzers[:-1]:
        want = _oracle_value(a, ot, 2049)
        assert _close(_metric(ctx, a), want), (str(a), _metric(ctx, a), want)
    # the unfiltered metrics are what they were: the oracle's over the whole table
    hist = ctx.metric(d.Histogram("s")).value.get()
    whole = O.histogram_metric(O.histogram_state(ot, "s"))
    assert hist.numberOfBins == whole["number_of_bins"]
    assert {k: (v.absolute, v.ratio) for k, v in hist.values.items()} == whole["values"]


def test_aggregated_states_of_filtered_partitions(gpu):
    (s1, o1), (s2, o2) = _spec(65), _spec(2049)
    both = oracle_table({k: [s1[k][0], s1[k][1] + s2[k][1]] for k in NAMES})
    analyzers = [d.Uniqueness(["s"]), d.Uniqueness(["s"], "l > 0"), d.Distinctness(["s"], "l > 0"),
                 d.Entropy("s", "l > 0"), d.CountDistinct(["s"], "l <= 0")]
    providers = []
    for spec in (s1, s2):
        p = d.InMemoryStateProvider()
        d.AnalysisRunner.onData(_table(spec).to_device(0)).addAnalyzers(analyzers).saveStatesWith(p).run()
        providers.append(p)
    ctx = d.AnalysisRunner.runOnAggregatedStates(SCHEMA, d.Analysis(analyzers), providers)
    one_shot = d.AnalysisRunner.onData(_table({k: [s1[k][0], s1[k][1] + s2[k][1]] for k in NAMES}).to_device(0)) \
        .addAnalyzers(analyzers).run()
    _VERD = {w: _keep(65, w, o1) + _keep(2049, w, o2) for w in ("l > 0", "l <= 0")}
    for a in analyzers:
        sub = _restrict(both, _VERD[a.where]) if a.where else both
        name = type(a).__name__
        cols = [a.column] if name == "Entropy" else list(a.columns)
        want = oracle_metric(O.frequencies_state(sub, cols), name, [cols])
        assert _close(_metric(ctx, a), want), (str(a), _metric(ctx, a), want)
        assert _close(_metric(one_shot, a), want), (str(a), _metric(one_shot, a), want)


# ---------------------------------------------------------------- 7. ABI rules
def _predicate(where, schema):
    packed = _pred_array(compile_predicate(where, schema_index(schema)))
    pred = L.DqPredicate()
    _fill_pred(pred, packed)
    return pred, packed  # (packed keeps the buffers alive)


def test_abi_rules(gpu):
    lib = L.lib()
    schema = {"k": "int64", "v": "int64"}
    pred, keep = _predicate("v > 0", schema)
    batch = d.Table.from_pydict({"k": ("int64", [1, 2, 2]), "v": ("int64", [1, -1, 1])})
    t = FrequencyTable(["k"], schema)
    try:
        t.consume(batch)
        assert lib.dq_freq_set_filter(t.handle, ctypes.byref(pred)) == L.DQ_ERR_STATE
        t.reset()  # an empty table again: the filter is accepted, and applies
        assert lib.dq_freq_set_filter(t.handle, ctypes.byref(pred)) == L.DQ_OK
        t.consume(batch)
        s = t.summary()
        assert (s.num_rows, s.num_groups, s.num_unique, s.grouped_rows) == (2, 2, 2, 2)
        assert t.lookup(encode_key([2], ["int64"])) == 1
    finally:
        t.close()
    h = FrequencyTable(["k"], schema, histogram=True)
    try:
        assert lib.dq_freq_set_filter(h.handle, ctypes.byref(pred)) == L.DQ_ERR_UNSUPPORTED
        assert "DQ_FREQ_NULL_AS_KEY" in lib.dq_last_error().decode()
    finally:
        h.close()
    with pytest.raises(L.DeequAmdError) as e:
        FrequencyTable(["k"], schema, histogram=True, where="v > 0")
    assert e.value.status == L.DQ_ERR_UNSUPPORTED


def test_abi_declines_what_a_plan_declines(gpu):
    """A comparison over a decimal column: dq_freq_set_filter's status and message are those of
    dq_op_supported for a Size with the same `where`."""
    lib = L.lib()
    types = (ctypes.c_int32 * 2)(L.TYPE_CODES["int64"], L.decimal_type(10, 2))
    code = (L.DqPredInsn * 3)()
    for ins, (op, arg, i64) in zip(code, ((L.DQ_P_COLUMN, 1, 0), (L.DQ_P_LIT_INT, 0, 1), (L.DQ_P_GT, L.DQ_CMP_AS_INT64, 0))):
        ins.opcode, ins.arg, ins.i64, ins.f64 = op, arg, i64, 0.0
    pred = L.DqPredicate()
    pred.code, pred.n_insns = code, 3
    key = (ctypes.c_int32 * 1)(0)
    h = ctypes.c_void_p()
    L.check(lib.dq_freq_create(L.Context.get(0).handle, key, 1, types, 2, 0, ctypes.byref(h)))
    try:
        assert lib.dq_freq_set_filter(h, ctypes.byref(pred)) == L.DQ_ERR_UNSUPPORTED
        mine = lib.dq_last_error().decode()
    finally:
        lib.dq_freq_destroy(h)
    op = L.DqOp()
    op.kind, op.column, op.column2 = L.DQ_OP_SIZE, -1, -1
    op.where = pred
    assert lib.dq_op_supported(ctypes.byref(op), types, 2) == L.DQ_ERR_UNSUPPORTED
    assert mine == lib.dq_last_error().decode() and "decimal" in mine


def test_unsupported_predicate_is_the_predicate_modules(gpu):
    with pytest.raises(UnsupportedPredicate) as e:
        FrequencyTable(["l"], SCHEMA, where="l + 1 > 2")
    assert "arithmetic (+) is not GPU-eligible" in str(e.value)


# ---------------------------------------------------------------- 8. ShardedTable
def _sharded_worker(port, q):
    import sys
    sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
    import torch.distributed as dist
    import deequ_amd as dd
    from deequ_amd.distributed import ShardedTable
    from deequ_amd.frequencies import compute_frequencies
    from predicate_cases import table as make
    dd.set_device(0)
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=0, world_size=1)
    t = dd.Table.from_pydict({k: (ty, v) for k, (ty, v) in make(2049, 7000 + 2049).items()})
    out = {}
    for cols in (["s"], ["l", "s"]):
        sharded = compute_frequencies(ShardedTable(t), cols, where="l > 3")
        plain = compute_frequencies(t, cols, where="l > 3")
        out[tuple(cols)] = (sharded.numRows, sharded.frequencies(raw=True), plain.numRows, plain.frequencies(raw=True))
    an = [dd.Uniqueness(["s"], "l > 3"), dd.Entropy("s", "l > 3"), dd.Distinctness(["l", "s"], "d > 0.5")]
    a = dd.AnalysisRunner.onData(ShardedTable(t)).addAnalyzers(an).run()
    b = dd.AnalysisRunner.onData(t).addAnalyzers(an).run()
    out["metrics"] = [(str(x), a.metric(x).value.get(), b.metric(x).value.get()) for x in an]
    q.put(out)
    dist.barrier()
    dist.destroy_process_group()


def test_sharded_filtered_state_equals_unsharded(gpu):
    import torch.multiprocessing as mp
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_sharded_worker, args=(port, q))
    p.start()
    out = q.get(timeout=240)
    p.join(timeout=60)
    assert p.exitcode == 0
    spec, ot = _spec(2049)
    for cols in (["s"], ["l", "s"]):
        n_sh, f_sh, n_pl, f_pl = out[tuple(cols)]
        want = O.frequencies_state(_restrict(ot, _keep(2049, "l > 3", ot)), cols)
        assert n_sh == n_pl == want.num_rows
        assert f_sh == f_pl
        assert f_pl == {encode_key(list(k), [SCHEMA[c] for c in cols]): c for k, c in want.frequencies.items()}
    for name, sharded, plain in out["metrics"]:
        assert sharded == plain, (name, sharded, plain)
