"""KLLSketch on the GPU (dq_kll_slab_kernel, dq_kll_merge_kernel) against the CPU mirror of the
same slab-and-tree layout (deequ_amd.states.kll_sketch_slabs): the state must be equal exactly --
compactor items bit for bit, numOfCompress, offset, min, max -- and so the buckets.  The
reference's known answers (tests/golden/kll_known_answers.json) through AnalysisRunner and the
profiler; slab sizes that are no multiple of the wave, NULL runs that empty whole slabs, special
values, several columns with different parameters in one launch, batches, and one 300 000-row
slab whose sketch holds seven levels in LDS."""
import math

import numpy as np
import pytest

import deequ_amd as d
from deequ_amd import _lib as L
from deequ_amd import kll
from deequ_amd.states import KLL_INIT_MAX, KLL_INIT_MIN, kll_sketch_slabs

import kll_cases as K

pytestmark = pytest.mark.gpu
N = 20_001
LAYOUTS = [(2, 37), (2048, 1000), (2048, 4096)]


def gpu_states(table, specs, slab_rows, batches=None):
    """KLLState per (column, k, c) of specs from one sketcher over the batches."""
    sk = kll.KLLSketcher(table.schema, specs, slab_rows)
    try:
        for b in (batches or [table]):
            sk.consume(b)
        return sk.finish()
    finally:
        sk.close()


def column_inputs(kind):
    """(numpy values, validity, dtype) of one test column: 20 001 rows, never modified."""
    vals, valid = K.seeded()
    vals, valid = vals[:N], valid[:N].copy()
    if kind == "float64":
        return vals, valid, "float64"
    if kind == "int64":
        return np.round(vals).astype(np.int64), valid, "int64"
    if kind == "null_runs":  # NULL runs that empty whole slabs of 37, 1000 and 4096 rows
        valid[100:100 + 3 * 37] = False
        valid[3000:5000] = False
        valid[8192:8192 + 4096] = False
        return vals, valid, "float64"
    if kind == "all_null":
        return vals, np.zeros(N, dtype=bool), "float64"
    if kind == "special":
        v = vals.copy()
        v[::7] = 0.0
        v[3::11] = -0.0
        v[5::13] = np.inf
        v[6::17] = -np.inf
        v[9::19] = np.nan
        return v, valid, "float64"
    if kind == "big_int64":  # beyond 2^53: Long.toDouble rounds to nearest even
        rng = np.random.default_rng(5)
        v = rng.integers(2 ** 53, 2 ** 62, N, dtype=np.int64)
        v[::2] |= 1
        v[1::5] *= -1
        return v, valid, "int64"
    if kind == "above_2_31":  # the min quirk: globalMin stays Int.MaxValue
        return np.abs(vals) + 2.0 ** 31 + 1.0, valid, "float64"
    raise KeyError(kind)


KINDS = ["float64", "int64", "null_runs", "all_null", "special", "big_int64", "above_2_31"]


@pytest.mark.parametrize("k,slab_rows", LAYOUTS, ids=lambda v: str(v))
@pytest.mark.parametrize("kind", KINDS)
def test_state_equals_cpu_mirror(gpu, kind, k, slab_rows):
    vals, valid, dtype = column_inputs(kind)
    host = d.Table({"x": d.Column.from_numpy(vals, valid, dtype)})
    want = kll_sketch_slabs(K.pylist(vals, valid), k, 0.64, slab_rows)
    for table in (host, host.to_device(0)):
        (got,) = gpu_states(table, [("x", k, 0.64)], slab_rows)
        assert [len(c.buffer) for c in got.qSketch.compactors] == [len(c.buffer) for c in want.qSketch.compactors]
        assert got.qSketch.levels() == want.qSketch.levels()
        assert got == want
        assert got.qSketch.weight() == int(valid.sum())
    analyzer = d.KLLSketch("x", d.KLLParameters(k, 0.64, 20))
    assert K.dist_bits(analyzer.computeMetricFrom(got)) == K.dist_bits(analyzer.computeMetricFrom(want))
    if kind == "all_null":
        assert (got.globalMin, got.globalMax) == (KLL_INIT_MIN, KLL_INIT_MAX)
        assert [b.count for b in analyzer.computeMetricFrom(got).value.get().buckets] == [0] * 20
    if kind == "special":
        assert math.isnan(got.globalMin) and math.isnan(got.globalMax)
    if kind == "above_2_31":
        assert got.globalMin == 2147483647.0
    if kind == "big_int64":
        assert got.globalMax == float(int(vals[valid].max()))


@pytest.mark.parametrize("k,slab_rows", LAYOUTS, ids=lambda v: str(v))
def test_nonzero_arrow_offset(gpu, k, slab_rows):
    import pyarrow as pa
    vals, valid, _ = column_inputs("float64")
    arr = pa.array(np.where(valid, vals, 0.0), mask=~valid)
    for off in (3, 64 + 5):
        sliced = arr.slice(off)
        want = kll_sketch_slabs(K.pylist(vals[off:], valid[off:]), k, 0.64, slab_rows)
        host = d.Table({"x": d.Column.from_arrow(sliced)})
        assert host.columns["x"].offset == off
        for table in (host, host.to_device(0)):
            assert gpu_states(table, [("x", k, 0.64)], slab_rows)[0] == want
        batch = d.ArrowBatch(pa.record_batch([sliced], names=["x"]))  # ... and through the C Data Interface
        assert gpu_states(batch, [("x", k, 0.64)], slab_rows)[0] == want


def test_three_columns_with_different_parameters_in_one_launch(gpu):
    f, fv, _ = column_inputs("special")
    i, iv, _ = column_inputs("int64")
    s = (np.arange(N) % 251 - 125).astype(np.int16)
    table = d.Table({"f": d.Column.from_numpy(f, fv, "float64"), "i": d.Column.from_numpy(i, iv, "int64"),
                     "s": d.Column.from_numpy(s, None, "int16"),
                     "f32": d.Column.from_numpy(f.astype(np.float32), fv, "float32")}).to_device(0)
    specs = [("f", 2048, 0.64), ("i", 2, 0.64), ("s", 64, 0.5), ("f32", 200, 0.7)]
    got = gpu_states(table, specs, 1000)
    cols = {"f": (f, fv), "i": (i, iv), "s": (s, None), "f32": (f.astype(np.float32), fv)}
    for (name, k, c), state in zip(specs, got):
        vals, valid = cols[name]
        assert state == kll_sketch_slabs(K.pylist(vals, valid), k, c, 1000), name


def test_two_batches_then_sum_with_a_cpu_state(gpu):
    vals, valid, _ = column_inputs("float64")
    cut = 12_345
    parts = [d.Table({"x": d.Column.from_numpy(vals[a:b], valid[a:b], "float64")}).to_device(0)
             for a, b in ((0, cut), (cut, N))]
    (got,) = gpu_states(parts[0], [("x", 2048, 0.64)], 1000, batches=parts)
    first = kll_sketch_slabs(K.pylist(vals[:cut], valid[:cut]), 2048, 0.64, 1000)
    second = kll_sketch_slabs(K.pylist(vals[cut:], valid[cut:]), 2048, 0.64, 1000)
    assert got == first.sum(second)  # batches merge in arrival order (KLLState.sum)
    other_vals, other_valid = K.seeded()
    cpu = kll_sketch_slabs(K.pylist(other_vals[N:N + 5000], other_valid[N:N + 5000]), 2048, 0.64, 1000)
    total = got.sum(cpu)
    assert total == first.sum(second).sum(cpu)
    assert total.qSketch.weight() == int(valid.sum()) + int(other_valid[N:N + 5000].sum())


def test_one_big_slab_keeps_seven_levels_in_lds(gpu):
    vals, valid = K.seeded()
    table = d.Table({"x": d.Column.from_numpy(vals, valid, "float64")}).to_device(0)
    (got,) = gpu_states(table, [("x", 2048, 0.64)], 300_000)
    want = kll_sketch_slabs(K.pylist(vals, valid), 2048, 0.64, 300_000)
    assert len(got.qSketch.compactors) >= 7
    assert got == want
    assert got.qSketch.weight() == int(valid.sum())  # weight conservation


@pytest.mark.parametrize("case", K.PROFILES, ids=lambda c: c["ref"].split(":")[-1])
def test_known_answers_through_runner_and_profiler(gpu, case):
    k, c, n_buckets = case["kllParameters"]
    params = d.KLLParameters(k, c, n_buckets)
    table = K.known_table(case)
    want = d.BucketDistribution([d.BucketValue(*b) for b in case["buckets"]], case["parameters"], case["data"])
    analyzer = d.KLLSketch(case["column"], params)
    states = d.InMemoryStateProvider()
    ctx = d.AnalysisRunner.onData(table).addAnalyzers([analyzer, d.Size()]).saveStatesWith(states).run()
    assert ctx.metric(analyzer).value.get() == want
    assert ctx.metric(d.Size()).value.get() == float(len(case["values"]))
    assert states.load(analyzer).qSketch.getCompactorItems() == case["data"]
    again = d.AnalysisRunner.onData(table).addAnalyzer(analyzer).aggregateWith(states).run()
    assert sum(b.count for b in again.metric(analyzer).value.get().buckets) == \
        2 * sum(v is not None for v in case["values"])

    from deequ_amd.profiles import ColumnProfilerRunner
    prof = ColumnProfilerRunner().onData(table).setKLLParameters(params).run().profiles[case["column"]]
    assert prof.kll == want
    assert prof.approxPercentiles == sorted(want.computePercentiles()) and len(prof.approxPercentiles) == 99
    for name in ("mean", "maximum", "minimum", "sum", "stdDev", "completeness"):
        if name in case:
            assert getattr(prof, name) == pytest.approx(case[name], rel=1e-12), name
    plain = ColumnProfilerRunner().onData(table).run().profiles[case["column"]]
    assert plain.kll is None and plain.approxPercentiles is None  # KLL stays opt-in


def test_profiler_sketches_casted_string_columns(gpu):
    table = d.Table.from_pydict({"n": ("string", [str(float(v)) for v in range(1, 31)]),
                                 "t": ("string", ["a", "b"] * 15)})
    from deequ_amd.profiles import ColumnProfilerRunner
    profiles = ColumnProfilerRunner().onData(table).setKLLParameters(d.KLLParameters(2, 0.64, 2)).run().profiles
    case = K.PROFILES[1]
    assert profiles["n"].kll.data == case["data"]
    assert [[b.lowValue, b.highValue, b.count] for b in profiles["n"].kll.buckets] == case["buckets"]
    assert not hasattr(profiles["t"], "kll")


def test_slab_rows_override_changes_only_the_partitioning(gpu):
    vals, valid, _ = column_inputs("float64")
    table = d.Table({"x": d.Column.from_numpy(vals, valid, "float64")}).to_device(0)
    analyzer = d.KLLSketch("x", d.KLLParameters(64, 0.64, 10))
    default = d.AnalysisRunner.onData(table).addAnalyzer(analyzer).run().metric(analyzer).value.get()
    assert default.data == kll_sketch_slabs(K.pylist(vals, valid), 64, 0.64).qSketch.getCompactorItems()
    with kll.slab_rows(1000):
        small = d.AnalysisRunner.onData(table).addAnalyzer(analyzer).run().metric(analyzer).value.get()
    assert small.data == kll_sketch_slabs(K.pylist(vals, valid), 64, 0.64, 1000).qSketch.getCompactorItems()
    assert small.data != default.data


def test_oversize_parameters_are_declined(gpu):
    table = d.Table.from_pydict({"x": ("float64", [1.0, 2.0, 3.0])})
    big = d.KLLSketch("x", d.KLLParameters(50_000, 0.64, 10))
    flat = d.KLLSketch("x", d.KLLParameters(2048, 1.0, 10))
    ok = d.KLLSketch("x", d.KLLParameters(2048, 0.64, 10))
    ctx = d.AnalysisRunner.onData(table).addAnalyzers([big, flat, ok]).run()
    for a in (big, flat):
        m = ctx.metric(a)
        assert m.value.isFailure and "10112 items" in str(m.value.exception) and "LDS" in str(m.value.exception)
    assert ctx.metric(ok).value.isSuccess
    with pytest.raises(L.UnsupportedOnGpu, match="bound to 10112 items per sketch"):
        kll.KLLSketcher(table.schema, [("x", 50_000, 0.64)])
