"""ApproxQuantile / ApproxQuantiles on the GPU (dq_aq_count_kernel, dq_aq_plan_kernel) against the
numpy mirror of the batch summary (quantile_cases.py): the state must be equal bit for bit -- entry
values as uint64, g, delta, count.  Row counts around the wave and of two workgroup tiles with a
ragged third, relativeError 1.0 to 0.001 (15-bit to 4-bit digits, up to 14 passes), every numeric
type, special values, constant / two-valued / sorted columns, keys that differ only in their lowest
byte, NULL runs that empty whole tiles, sliced Arrow arrays, several pairs in one launch, batches;
then the analyzers through AnalysisRunner beside the fused scan and a KLLSketch."""
import numpy as np
import pytest

import deequ_amd as d
from deequ_amd import _lib as L
from deequ_amd import quantiles
from deequ_amd.states import ApproxQuantileState, PercentileDigest

import quantile_cases as Q

pytestmark = pytest.mark.gpu
ROWS = [1, 2, 63, 64, 65, Q.N]  # the counting kernel's tile is 8192 rows: 20 001 = two tiles and a ragged third
EPS = [1.0, 0.25, 0.01, 0.001]
G = Q.GOLDEN


def gpu_states(table, specs, batches=None):
    sk = quantiles.QuantileSketcher(table.schema, specs)
    try:
        for b in (batches or [table]):
            sk.consume(b)
        return sk.finish()
    finally:
        sk.close()


def assert_state(got, eps, count, entries):
    dig = got.percentileDigest
    assert dig.relativeError == eps
    assert dig.count == count
    assert Q.entries_bits(dig) == entries


@pytest.mark.parametrize("kind", Q.KINDS)
def test_state_equals_numpy_mirror(gpu, kind):
    for n in ROWS:
        vals, valid, dtype = Q.column(kind, n)
        host = d.Table({"x": d.Column.from_numpy(vals, valid, dtype)})
        want = [Q.batch_summary(vals, valid, eps) for eps in EPS]
        for table in (host, host.to_device(0)):
            got = gpu_states(table, [("x", eps) for eps in EPS])
            for eps, state, (count, entries) in zip(EPS, got, want):
                assert_state(state, eps, count, entries)
        if kind == "all_null":
            assert all(s.percentileDigest.getPercentiles([0.5]) == [] for s in got)
        if kind == "special" and n == Q.N:
            bits = [b for b, _, _ in Q.entries_bits(got[3].percentileDigest)]
            assert bits[-1] == 0x7FF8000000000000  # every NaN leaves as the canonical one, last
            assert 0x8000000000000000 in bits and 0 in bits  # -0.0 and +0.0 stay distinct


def test_more_tiles_than_workgroups(gpu):
    """Past 256 tiles of 8192 rows the workgroups stride over the batch: some take three tiles here,
    the others two, the last tile ragged."""
    n = 2 * 256 * 8192 + 8192 + 17
    rng = np.random.default_rng(3)
    vals = rng.random(n) * 2.0 - 1.0
    valid = rng.random(n) >= 0.03
    table = d.Table({"x": d.Column.from_numpy(vals, valid, "float64")}).to_device(0)
    specs = [("x", 0.001), ("x", 0.25)]
    for (_, eps), state in zip(specs, gpu_states(table, specs)):
        assert_state(state, eps, *Q.batch_summary(vals, valid, eps))


def test_sliced_arrow_arrays(gpu):
    import pyarrow as pa
    vals, valid, _ = Q.column("float64")
    arr = pa.array(np.where(valid, vals, 0.0), mask=~valid)
    specs = [("x", 0.01), ("x", 0.001)]
    for off in (3, 69):
        sliced = arr.slice(off)
        want = [Q.batch_summary(vals[off:], valid[off:], eps) for _, eps in specs]
        host = d.Table({"x": d.Column.from_arrow(sliced)})
        assert host.columns["x"].offset == off
        sources = [host, host.to_device(0), d.ArrowBatch(pa.record_batch([sliced], names=["x"]))]
        for source in sources:
            for (_, eps), state, (count, entries) in zip(specs, gpu_states(source, specs), want):
                assert_state(state, eps, count, entries)


def test_several_columns_and_errors_in_one_sketcher(gpu):
    cols = {name: Q.column(name) for name in ("special", "int64", "int16", "float32", "low_byte")}
    table = d.Table({k: d.Column.from_numpy(v, ok, t) for k, (v, ok, t) in cols.items()}).to_device(0)
    specs = [("special", 0.001), ("int64", 0.25), ("int16", 0.01), ("float32", 1.0), ("low_byte", 0.001),
             ("special", 0.01)]
    together = gpu_states(table, specs)
    for spec, state in zip(specs, together):
        (alone,) = gpu_states(table, [spec])
        assert state == alone, spec
        vals, valid, _ = cols[spec[0]]
        assert_state(state, spec[1], *Q.batch_summary(vals, valid, spec[1]))


def test_three_unequal_batches_fold_as_the_python_digest(gpu):
    vals, valid, _ = Q.column("float64")
    cuts = [(0, 7001), (7001, 7002), (7002, Q.N)]
    assert [b - a for a, b in cuts] == [7001, 1, 12_999]
    parts = [d.Table({"x": d.Column.from_numpy(vals[a:b], valid[a:b], "float64")}).to_device(0) for a, b in cuts]
    for eps in (0.01, 0.001):
        (got,) = gpu_states(parts[0], [("x", eps)], batches=parts)
        want = PercentileDigest(eps)
        for a, b in cuts:
            want.merge(Q.digest_of(eps, vals[a:b], valid[a:b]))
        assert got.percentileDigest == want
        assert Q.entries_bits(got.percentileDigest) == Q.entries_bits(want)


def known_table(dtype, values):
    return d.Table.from_pydict({"att1": (dtype, list(values)), "att2": ("float64", [float(v) for v in values])})


def test_known_answers_through_the_runner(gpu):
    for case in G["exact"]:
        table = known_table(case["dtype"], case["values"])
        q = d.ApproxQuantile("att1", case["quantile"], case["relativeError"])
        many = d.ApproxQuantiles("att1", [0.0, case["quantile"], 1.0])
        kll = d.KLLSketch("att2", d.KLLParameters(2, 0.64, 2))
        analyzers = [d.Size(), d.Mean("att1"), q, many, kll]
        ctx = d.AnalysisRunner.onData(table).addAnalyzers(analyzers).run()
        assert list(ctx.metricMap) == analyzers
        assert ctx.metric(q) == d.DoubleMetric(d.Entity.Column, "ApproxQuantile-0.5", "att1", d.Success(case["answer"]))
        assert ctx.metric(many).value.get() == {"0.0": 1.0, "0.5": case["answer"], "1.0": 6.0}
        assert ctx.metric(d.Size()).value.get() == 6.0 and ctx.metric(d.Mean("att1")).value.get() == 3.5
        assert ctx.metric(kll).value.isSuccess
        assert '"ApproxQuantiles-0.5"' in ctx.successMetricsAsJson()
    r = G["range"]
    table = known_table(r["dtype"], range(r["start"], r["stop"]))
    analyzers = [d.ApproxQuantile("att1", c["quantile"], r["relativeError"]) for c in r["cases"]]
    ctx = d.AnalysisRunner.onData(table).addAnalyzers(analyzers).run()
    for a, c in zip(analyzers, r["cases"]):
        got = ctx.metric(a).value.get()
        assert got == c["answer"] and c["above"] < got < c["below"]


def test_all_null_and_declined_errors(gpu):
    table = d.Table.from_pydict({"x": ("float64", [None, None, None]), "y": ("float64", [1.0, 2.0, 3.0])})
    empty = d.ApproxQuantile("x", 0.5)
    kept = d.ApproxQuantiles("x", [0.5])
    exact = d.ApproxQuantile("y", 0.5, 0.0)
    fine = d.ApproxQuantile("y", 0.5, 0.0005)
    ok = d.ApproxQuantile("y", 0.5)
    ctx = d.AnalysisRunner.onData(table).addAnalyzers([empty, kept, exact, fine, ok, d.Size(), d.Mean("y")]).run()
    failed = ctx.metric(empty).value
    assert isinstance(failed.exception, d.EmptyStateException)
    assert str(failed.exception) == "Empty state for analyzer ApproxQuantile(x,0.5,0.01), all input values were NULL."
    assert ctx.metric(kept).value.get() == {}
    for a, words in ((exact, "full sort"), (fine, "2048 target ranks")):
        m = ctx.metric(a).value
        assert m.isFailure and "status %d" % L.DQ_ERR_UNSUPPORTED in str(m.exception) and words in str(m.exception)
        assert isinstance(m.exception.__cause__, L.UnsupportedOnGpu)
        assert "0.001" in str(m.exception)
    assert ctx.metric(ok).value.get() == 2.0
    assert ctx.metric(d.Size()).value.get() == 3.0 and ctx.metric(d.Mean("y")).value.get() == 2.0
    with pytest.raises(L.UnsupportedOnGpu, match="relativeError >= 0.001"):
        quantiles.QuantileSketcher(table.schema, [("y", 0.0)])


def test_states_persist_load_and_aggregate(gpu, tmp_path):
    inc = G["incremental"]
    a = d.ApproxQuantile("att1", inc["quantile"], inc["relativeError"])
    halves = [known_table(inc["dtype"], inc[k]) for k in ("first", "second")]
    providers = [d.HdfsStateProvider(str(tmp_path / ("half%d" % i))) for i in range(2)]
    for table, provider in zip(halves, providers):
        assert d.AnalysisRunner.onData(table).addAnalyzer(a).saveStatesWith(provider).run().metric(a).value.isSuccess
    assert providers[0].load(a) == ApproxQuantileState(Q.digest_of(inc["relativeError"], np.array(inc["first"])))
    analysis = d.Analysis([a, d.ApproxQuantiles("att1", [0.5])])
    ctx = d.AnalysisRunner.runOnAggregatedStates(halves[0].schema, d.Analysis([a]), providers)
    assert ctx.metric(a).value.get() == inc["answer"]
    whole = known_table(inc["dtype"], inc["first"] + inc["second"])
    assert d.AnalysisRunner.run(whole, analysis).metric(a).value.get() == inc["answer"]
    # aggregateWith: the second half on top of the first half's saved state
    again = d.AnalysisRunner.onData(halves[1]).addAnalyzer(a).aggregateWith(providers[0]).run()
    assert again.metric(a).value.get() == inc["answer"]
