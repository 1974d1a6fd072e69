"""Every Python entry point that hands device-resident inputs to the library, called while the
kernel that writes those inputs is still queued on torch's current stream (the harness:
async_inputs.py; the contract: DESIGN.md, "Stream ordering at the Python boundary").

Each test runs its API three times: on the real data uploaded synchronously (the expected result --
that path is pinned against the oracle by the rest of the suite), on the sentinel data uploaded
synchronously (its result must differ, so the data can tell a premature read), and on tensors that
hold the sentinel until a delayed copy of the real data lands.  Device-resident outputs are cloned by
a torch op on the current stream right after the call, and the clones are compared: they must be
complete for the caller's next kernel, not only after a device-wide wait.

Every test runs with torch's default stream as the current stream and with a stream of torch's
pool: the library's null-stream launches (KLL, quantiles, schema, take) are ordered behind the first
by the runtime, behind the second by nothing.

Measured on an MI355X: the calibrated 150 ms `_sleep` lasts 147 to 148 ms; the longest undelayed call
is the whole ColumnProfilerRunner run, 5.0 ms, so the default delay is 30 times the longest call
(`_delay_for` raises it to 20 times a slower call; one that the 500 ms cap cannot cover fails).

Before the waits of `_lib.after_current_stream` were added, run_scan and the string casts returned the
sentinel's results here.  FrequencyTable.consume, the sketchers, the schema validator and the
few-groups call already returned the real data's, and take, correlation_matrix, row_level_results and
the cross-table checks still do with their `synchronize` removed: their C entry points allocate and
copy with blocking calls before their first launch, which waits for the device on this runtime.  So
these tests fail for a missing wait only in the scan and the casts; for the other entry points they
document the contract and would catch a library change that drops the accidental wait (DESIGN.md
lists both groups)."""
from collections import OrderedDict
import time

import numpy as np
import pytest

import async_inputs as A
import deequ_amd as d
from deequ_amd import kll, quantiles
from deequ_amd.engine import Plan, op_spec_for
from deequ_amd.profiles import (ColumnProfilerRunner, ColumnProfiles, _few_group_strings, cast_string_column,
                                cast_string_columns)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(params=["default_stream", "pool_stream"])
def current(request, gpu):
    """torch's current stream for the test: the default one, or one from torch's pool."""
    import torch
    if request.param == "default_stream":
        yield request.param
        return
    stream = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(stream):
        yield request.param
    stream.synchronize()


def _delay_for(call_ms):
    """The delay of a test whose undelayed call takes `call_ms`: 20 times the call, so that a
    premature read lands wholly inside the sleep; at least the default, at most the cap."""
    return min(A.MAX_MS, max(A.DEFAULT_MS, 20.0 * call_ms))


def _timed(call, arg):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = call(arg)
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def _report(label, call_ms, delay_ms):
    """Prints both figures and holds the delay to 20 times the undelayed call: a call so slow that
    the 500 ms cap cannot give it that margin fails here, it does not run with a smaller one."""
    assert delay_ms >= 20.0 * call_ms, ("%s: the undelayed call takes %.1f ms, so the delay must be %.0f ms, above the "
                                         "cap of %.0f ms" % (label, call_ms, 20.0 * call_ms, A.MAX_MS))
    print("async_inputs: %-44s undelayed call %8.3f ms, delay %5.0f ms" % (label, call_ms, delay_ms))


def _check_delayed(label, call, real, sentinel, to_host=lambda r: r):
    """`call(table)` over the delayed table equals `call` over the real data and not over the
    sentinel.  `to_host` turns a result (device clones) into host values once the call has returned."""
    want = to_host(call(A.synced_table(real)))  # (also warms the call: plans, code objects)
    other, call_ms = _timed(call, A.synced_table(sentinel))
    other = to_host(other)
    assert not A.same(want, other), "the sentinel's result does not differ: the data cannot tell a premature read"
    delay = _delay_for(call_ms)
    _report(label, call_ms, delay)
    table, ev = A.delayed_table(real, sentinel, delay)
    assert not ev.query(), "delay too short"
    got = call(table)
    got = to_host(got)
    assert not A.same(got, other), "%s read its input before the producer on the current stream wrote it" % label
    assert A.same(got, want), "%s\n%s" % (label, A.differences(got, want))


def test_the_calibrated_delay_lasts_as_long_as_asked(gpu):
    """Linear in the cycle count: within 20 % of the request (the timed calibration run is 1 to 20 ms
    long, its event resolution and launch overhead some 10 us)."""
    ms = A.measured_sleep_ms(DEV, A.DEFAULT_MS)
    print("async_inputs: calibrated_sleep(%g ms) lasts %.1f ms" % (A.DEFAULT_MS, ms))
    assert 0.8 * A.DEFAULT_MS <= ms <= 1.2 * A.DEFAULT_MS
    with pytest.raises(ValueError):
        A.calibrated_sleep(DEV, A.MAX_MS + 1)


# ---------------------------------------------------------------- the fused scan
SCAN = [d.Size(), d.Sum("i"), d.StandardDeviation("f"), d.Minimum("i"), d.Maximum("f"), d.Completeness("b"),
        d.Compliance("b is true", "b"), d.ApproxCountDistinct("s"), d.DataType("s"), d.MaxLength("s"),
        d.Completeness("s"), d.Compliance("i is not negative", "i >= 0"), d.PatternMatch("s", "^1")]


def test_run_scan(current):
    real, sentinel = A.tables("i", "f", "b", "s")
    _check_delayed("run_scan", lambda t: d.run_scan(SCAN, t), real, sentinel)


def test_run_scan_of_a_decimal_column(current):
    real, sentinel = A.tables("dec", "i")
    analyzers = [d.Sum("dec"), d.Minimum("dec"), d.Maximum("dec"), d.Mean("dec"), d.Completeness("dec")]
    _check_delayed("run_scan, decimal", lambda t: d.run_scan(analyzers, t), real, sentinel)


def test_plan_consume_reads_the_batch_as_it_is_at_the_call(current):
    """Point 3 of the contract: dq_plan_consume only queues the scan.  The plan's stream is held
    back by a sleep, the batch is consumed and then overwritten in place on the current stream: the
    states are those of the values at consume time."""
    import torch
    real, sentinel = A.tables("i", "f", "b", "s")
    want = d.run_scan(SCAN, A.synced_table(real))
    other = d.run_scan(SCAN, A.synced_table(sentinel))
    assert not A.same(want, other)
    buffers = A.upload([b for c in real.columns.values() for b in A._buffers(c)])
    later = A.upload([b for c in sentinel.columns.values() for b in A._buffers(c)])
    pairs = [(t, s) for t, s in zip(buffers, later) if t is not None]
    table = A.device_table(real, buffers)
    plan = Plan([op_spec_for(a, table.schema) for a in SCAN], table.schema)
    try:
        own = torch.cuda.ExternalStream(plan.stream, device=torch.device(DEV))
        A.calibrated_sleep(DEV, 1.0)  # (calibrates here, not on the plan's stream)
        with torch.cuda.stream(own):
            A.calibrated_sleep(DEV, A.DEFAULT_MS)
            ev = torch.cuda.Event()
            ev.record()
        plan.consume(table)
        for t, s in pairs:
            t.copy_(s)
        assert not ev.query(), "delay too short"
        got = dict(zip(SCAN, plan.finish()))
    finally:
        plan.close()
    assert not A.same(got, other), "the scan read the batch after the caller overwrote it"
    assert A.same(got, want), A.differences(got, want)


# ---------------------------------------------------------------- the frequency family
def _frequencies(key):
    def call(table):
        t = d.FrequencyTable([key], dict(table.schema))
        try:
            t.consume(table)
            s = t.summary()
            return (s.num_rows, s.num_groups, s.num_unique, s.grouped_rows), d.FrequenciesAndNumRows(t).frequencies(raw=True)
        finally:
            t.close()
    return call


@pytest.mark.parametrize("key", ["i", "s"])
def test_frequency_table_consume(current, key):
    real, sentinel = A.tables(key, "f")
    _check_delayed("FrequencyTable.consume, %s key" % key, _frequencies(key), real, sentinel)


@pytest.mark.parametrize("offsets_dtype", ["int64", "int32"])
def test_import_flat_of_device_tensors(current, offsets_dtype):
    """The flat groups are written by a delayed producer; with int32 offsets import_flat itself
    queues the widening on the current stream and hands the library the fresh buffer."""
    groups = 5000
    rng = np.random.default_rng(5)
    flat = {False: (rng.integers(1, 100, groups), np.arange(groups, dtype=np.int64)),
            True: (rng.integers(100, 200, groups), np.arange(groups, dtype=np.int64) + 10 ** 6)}
    offsets = np.arange(groups + 1, dtype=offsets_dtype) * 8  # (the same for both, uploaded ready-made)

    def call(tensors):
        t = d.FrequencyTable(["i"], {"i": "int64"})
        try:
            t.import_flat(tensors[0], tensors[2], tensors[1], num_rows=7)
            return t.num_rows, d.FrequenciesAndNumRows(t).frequencies(raw=True)
        finally:
            t.close()

    def up(sentinel):
        counts, keys = flat[sentinel]
        return A.upload([counts, keys.view(np.uint8), offsets])
    want = call(up(False))
    other, call_ms = _timed(call, up(True))
    assert want != other
    delay = _delay_for(call_ms)
    _report("import_flat, %s offsets" % offsets_dtype, call_ms, delay)
    dst, src = up(True), up(False)
    ev = A.delayed(src[:2], dst[:2], delay)
    assert not ev.query(), "delay too short"
    got = call(dst)
    assert got != other, "import_flat read the groups before the producer on the current stream wrote them"
    assert got == want


def test_export_flat_to_device_is_complete_for_the_next_kernel(current):
    """Point 2 for export_flat(device=True): the tensors it returns are complete for a torch op queued
    at once (the export drains the table's stream).  No producer is delayed here and no memory that
    queued work still uses is recycled into the outputs, so this test does not pin the wait that
    export_flat makes after allocating them; that wait is by construction only."""
    real, _ = A.tables("s")
    t = d.FrequencyTable(["s"], dict(real.schema))
    try:
        t.consume(A.synced_table(real))
        want = t.export_flat()
        got = [x.clone() for x in t.export_flat(device=True)]
    finally:
        t.close()
    for g, w in zip(got, want):
        assert np.array_equal(g.cpu().numpy(), w)


# ---------------------------------------------------------------- sketches
def test_kll_sketcher_consume(current):
    real, sentinel = A.tables("f", "i")

    def call(table):
        sk = kll.KLLSketcher(table.schema, [("f", 2048, 0.64), ("i", 256, 0.64)])
        try:
            sk.consume(table)
            return sk.finish()
        finally:
            sk.close()
    _check_delayed("KLLSketcher.consume", call, real, sentinel)


def test_quantile_sketcher_consume(current):
    real, sentinel = A.tables("f", "i")

    def call(table):
        sk = quantiles.QuantileSketcher(table.schema, [("f", 0.01), ("i", 0.05)])
        try:
            sk.consume(table)
            return sk.finish()
        finally:
            sk.close()
    _check_delayed("QuantileSketcher.consume", call, real, sentinel)


# ---------------------------------------------------------------- the schema validator
def test_row_level_schema_validator(current):
    real, sentinel = A.tables("s", "x")
    schema = d.RowLevelSchema().withIntColumn("s", minValue=0, maxValue=4999).withDecimalColumn("x", 5, 1)

    def call(table):
        res = d.RowLevelSchemaValidator.validate(table, schema, withRowIndices=True)
        return (res.numValidRows, res.numInvalidRows, res.validRowIndices, res.invalidRowIndices,
                A.snapshot(res.validRows), A.snapshot(res.invalidRows))

    def to_host(r):
        return r[:4] + (A.host_table(r[4]), A.host_table(r[5]))
    _check_delayed("RowLevelSchemaValidator.validate", call, real, sentinel, to_host)


# ---------------------------------------------------------------- the profiler
def _cast_to_host(col):
    """(values where valid, the valid mask): the bytes under a NULL and past the last row are not
    part of the result."""
    n = col.length
    valid = np.unpackbits(col.validity.cpu().numpy(), bitorder="little")[:n].astype(bool)
    values = col.values.cpu().numpy()[:n]
    return np.where(valid, values, 0), valid


def _cloned(col):
    return d.Column(col.dtype, col.length, col.values.clone(), col.validity.clone(), device=True)


@pytest.mark.parametrize("column,to", [("s", "int64"), ("x", "float64")])
def test_cast_string_column(current, column, to):
    real, sentinel = A.tables(column)
    _check_delayed("cast_string_column to %s" % to, lambda t: _cloned(cast_string_column(t.columns[column], to)),
                   real, sentinel, _cast_to_host)


def test_cast_string_columns(current):
    real, sentinel = A.tables("s", "x")
    _check_delayed("cast_string_columns",
                   lambda t: [_cloned(c) for c in cast_string_columns([t.columns["s"], t.columns["x"]], ["int64", "float64"])],
                   real, sentinel, lambda cols: [_cast_to_host(c) for c in cols])


def test_few_group_strings(current):
    real, sentinel = A.tables("k")

    def call(table):
        few = _few_group_strings(table, ["k"])
        return {c: (g.groups, g.nulls) for c, g in few.items()}
    want = call(A.synced_table(real))
    assert len(want["k"][0]) == 40  # (the few-groups kernel took the column)
    _check_delayed("_few_group_strings", call, real, sentinel)


def test_column_profiler_run(current):
    real, sentinel = A.tables("i", "f", "b", "s", "k", "x")
    _check_delayed("ColumnProfilerRunner.run",
                   lambda t: ColumnProfiles.toJson(list(ColumnProfilerRunner().onData(t).run().profiles.values())),
                   real, sentinel)


# ---------------------------------------------------------------- the modules that already waited
def test_correlation_matrix(current):
    real, sentinel = A.tables("i", "f", "g", "dec")
    _check_delayed("correlation_matrix", lambda t: d.correlation_matrix(t, ["i", "f", "g", "dec"]).states(), real, sentinel)


def _take_rows(sentinel):
    if sentinel:
        return np.arange(A.N - 1, -1, -1, dtype=np.int64)[:A.N - 7].copy()
    rows = np.random.default_rng(9).permutation(A.N).astype(np.int64)[:A.N - 7]
    rows[::13] = -1
    return rows


def test_take_of_delayed_data(current):
    real, sentinel = A.tables("i", "b", "s", "dec")
    rows = _take_rows(False)
    _check_delayed("take, data", lambda t: A.snapshot(d.take(t, rows)), real, sentinel, A.host_table)


def test_take_with_delayed_rows(current):
    real, _ = A.tables("i", "b", "s", "dec")
    table = A.synced_table(real)

    def call(rows):
        return A.snapshot(d.take(table, rows))
    want = A.host_table(call(A.upload([_take_rows(False)])[0]))
    other, call_ms = _timed(call, A.upload([_take_rows(True)])[0])
    other = A.host_table(other)
    assert not A.same(want, other)
    delay = _delay_for(call_ms)
    _report("take, rows", call_ms, delay)
    dst, src = A.upload([_take_rows(True)]), A.upload([_take_rows(False)])
    ev = A.delayed(src, dst, delay)
    assert not ev.query(), "delay too short"
    got = call(dst[0])
    got = A.host_table(got)
    assert not A.same(got, other), "take read the row indices before the producer on the current stream wrote them"
    assert A.same(got, want)


ROW_LEVEL = [d.Completeness("i"), d.Compliance("i is not negative", "i >= 0"), d.PatternMatch("s", "^1"),
             d.Uniqueness(("id",)), d.Uniqueness(("i",), where="i >= 0")]


def test_row_level_results(current):
    real, sentinel = A.tables("i", "s", "id")

    def call(table):
        res = d.row_level_results(table, ROW_LEVEL)
        return [A.snapshot(d.Table(OrderedDict(outcome=res.column(a)))) for a in ROW_LEVEL]
    _check_delayed("row_level_results", call, real, sentinel, lambda r: [A.host_table(t) for t in r])


def _primary(sentinel):
    """A primary table for the cross-table checks over the reference A.tables("id", "i"): about half
    of its keys are in the reference, and seven in ten of those rows carry the reference's `i`."""
    ref = A.tables("id", "i")[1 if sentinel else 0]
    rng = np.random.default_rng(20 + sentinel)
    base = A.N if sentinel else 0
    ids = rng.integers(base, base + 2 * A.N, A.N)
    row_of = np.full(2 * A.N, -1, dtype=np.int64)
    row_of[ref.columns["id"].values - base] = np.arange(A.N)
    at = row_of[ids - base]
    i = np.where((at >= 0) & (rng.random(A.N) < 0.7), ref.columns["i"].values[np.maximum(at, 0)], 7777)
    nf = 0.0 if sentinel else 0.05
    return d.Table(OrderedDict(id=d.Column("int64", A.N, ids.astype(np.int64), A._validity(rng, A.N, nf)),
                               i=d.Column("int64", A.N, i.astype(np.int64), A._validity(rng, A.N, nf))))


@pytest.mark.parametrize("which", ["primary", "reference"])
@pytest.mark.parametrize("check", ["referential_integrity", "dataset_match"])
def test_cross_table_checks(current, check, which):
    ref_real, ref_sentinel = A.tables("id", "i")
    pri_real, pri_sentinel = _primary(False), _primary(True)
    fixed = A.synced_table(ref_real if which == "primary" else pri_real)

    def call(table):
        primary, reference = (table, fixed) if which == "primary" else (fixed, table)
        if check == "referential_integrity":
            res = d.referential_integrity(primary, ["id"], reference=reference)
        else:
            res = d.dataset_match(primary, reference, ["id"], compare=["i"], reference_rows=True)
        return res, A.snapshot(d.Table(OrderedDict(outcome=res.column())))
    real, sentinel = (pri_real, pri_sentinel) if which == "primary" else (ref_real, ref_sentinel)
    _check_delayed("%s, delayed %s" % (check, which), call, real, sentinel,
                   lambda r: (tuple(r[0].counts), A.host_table(r[1])))
