"""KLLSketch (KLLSketch.scala, QuantileNonSample.scala, NonSampleCompactor.scala) without a GPU.

The reference's sketch is deterministic, and its own tests pin compactor contents; the Python mirror
(deequ_amd.states) and the C++ host sketch (dq_diag_kll_sketch) both reproduce those known answers,
and equal each other level for level on the library's slab-and-tree layout.  The reference's rank
error criterion (KLLProbTest.scala) holds on the host sketch.  Serialization, preconditions, the
metric's bucket arithmetic, state providers and runOnAggregatedStates follow.  GPU: test_gpu_kll.py."""
import math
import struct

import numpy as np
import pytest

import deequ_amd as d
from deequ_amd import _lib as L
from deequ_amd.states import KLL_INIT_MAX, KLL_INIT_MIN, KLLState, QuantileNonSample

import kll_cases as K


# ---------------------------------------------------------------- the reference's known answers
@pytest.mark.parametrize("case", K.PROFILES, ids=lambda c: c["ref"].split(":")[-1])
@pytest.mark.parametrize("impl", ["mirror", "host"])
def test_known_answers(case, impl):
    k, c, n_buckets = case["kllParameters"]
    vals = [v for v in case["values"]]
    valid = np.array([v is not None for v in vals])
    arr = np.array([0.0 if v is None else float(v) for v in vals])
    state = (K.mirror_sketch if impl == "mirror" else K.host_sketch)(arr, valid, k, c, 1 << 16)
    assert state.qSketch.getCompactorItems() == case["data"]
    metric = d.KLLSketch(case["column"], d.KLLParameters(k, c, n_buckets)).computeMetricFrom(state)
    assert K.buckets_of(metric) == case["buckets"]
    assert metric.value.get().parameters == case["parameters"]
    want = d.BucketDistribution([d.BucketValue(*b) for b in case["buckets"]], case["parameters"], case["data"])
    assert metric.value.get() == want


def test_item_by_item_equals_bulk():
    vals, valid = K.seeded()
    rows = [v for v in K.pylist(vals[:30_000], valid[:30_000]) if v is not None]
    for k in (2, 64, 2048):
        a, b = QuantileNonSample(k, 0.64), QuantileNonSample(k, 0.64)
        for v in rows:
            a.update(v)
        b.updateAll(rows)
        assert a.levels() == b.levels()
        assert (a.compactorActualSize, a.compactorTotalSize) == (b.compactorActualSize, b.compactorTotalSize)


# ---------------------------------------------------------------- mirror == host sketch, level for level
@pytest.mark.parametrize("k,slab_rows", [(2, 37), (2, 1000), (64, 4096), (2048, 1000), (2048, 4096), (2048, 50_000)])
def test_mirror_equals_host_sketch(k, slab_rows):
    vals, valid = K.seeded()
    assert len(vals) == 300_000 and 0.04 < 1 - valid.mean() < 0.06
    a = K.mirror_sketch(vals, valid, k, 0.64, slab_rows)
    b = K.host_sketch(vals, valid, k, 0.64, slab_rows)
    assert [len(c.buffer) for c in a.qSketch.compactors] == [len(c.buffer) for c in b.qSketch.compactors]
    assert a.qSketch.levels() == b.qSketch.levels()  # items bit for bit, numOfCompress, offset
    assert a == b  # ... and min / max
    # weight conservation: every non-NULL row is in exactly one item's weight
    assert a.qSketch.weight() == int(valid.sum())
    assert sum(len(level) << i for i, level in enumerate(b.qSketch.getCompactorItems())) == int(valid.sum())
    assert (a.globalMin, a.globalMax) == (vals[valid].min(), vals[valid].max())


def test_special_values_order_and_min_max():
    nan, inf = float("nan"), float("inf")
    vals = np.array([0.0, -0.0, inf, -inf, nan, 1.5, -0.0, 0.0, nan, 2.0 ** 60, -3.0] * 40)
    for slab_rows in (7, 1000):
        a = K.mirror_sketch(vals, None, 2, 0.64, slab_rows)
        b = K.host_sketch(vals, None, 2, 0.64, slab_rows)
        assert a == b
        assert math.isnan(a.globalMin) and math.isnan(a.globalMax)  # math.min / math.max propagate NaN
    q = QuantileNonSample(8, 0.64)
    q.compactors[0].buffer = [0.0, nan, -0.0, inf, -inf, 1.0, -0.0, 0.0]
    out = q.compactors[0].compact()  # java.lang.Double.compare: -0.0 before 0.0, NaN last
    assert [struct.pack(">d", v) for v in out] == [struct.pack(">d", v) for v in (-inf, -0.0, 0.0, inf)]


def test_min_quirk_above_int_range():
    """KLLRunner.scala:28-29: min starts at Int.MaxValue, so values all above 2^31 leave it there."""
    vals = np.array([2.0 ** 31 + 5, 2.0 ** 40, 2.0 ** 33])
    for st in (K.mirror_sketch(vals, None, 2048, 0.64, 1 << 16), K.host_sketch(vals, None, 2048, 0.64, 1 << 16)):
        assert st.globalMin == 2147483647.0 == KLL_INIT_MIN and st.globalMax == 2.0 ** 40


# ---------------------------------------------------------------- the reference's own error criterion
def _rank_errors(q, n, k):
    eps = 100.0 / k
    step = int(math.ceil(max(eps * 0.2 * n, 1)))
    items = np.array([v for level in q.getCompactorItems() for v in level])
    weights = np.array([1 << i for i, level in enumerate(q.getCompactorItems()) for _ in level], dtype=np.int64)
    bad = 0
    for x in range(1, n, step):
        est = int(weights[~(items > x)].sum())
        assert est == q.getRank(float(x)) or x > 1 + 3 * step  # (the vectorised rank is getRank; spot-checked)
        if abs(est - x) >= eps * n:
            bad += 1
    return bad


@pytest.mark.parametrize("k", [100, 1000])
@pytest.mark.parametrize("stream", ["zoom-in", "shuffled", "merged"])
def test_reference_rank_criterion_on_host_sketch(stream, k):
    spec = next(s for s in K.GOLDEN["prob"]["streams"] if s["name"] == stream)
    c = K.GOLDEN["prob"]["shrinkingFactor"]
    if stream == "merged":
        plen, merges = spec["partitionLen"], spec["merges"]
        last = QuantileNonSample(k, c)
        for m in range(merges):
            i = np.arange(1, plen // 2 + 1)
            part = np.stack([i + m * plen, m * plen + plen + 1 - i], axis=1).reshape(-1).astype(np.float64)
            last = last.merge(K.host_sketch(part, None, k, c, plen).qSketch)
        n = plen * merges
        assert last.weight() == n
    else:
        n = spec["n"]
        if stream == "zoom-in":
            i = np.arange(1, n // 2 + 1)
            vals = np.stack([i, n + 1 - i], axis=1).reshape(-1).astype(np.float64)
        else:
            vals = np.random.default_rng(1).permutation(np.arange(1, n)).astype(np.float64)
        last = K.host_sketch(vals, None, k, c, len(vals)).qSketch  # one slab: the plain sequential sketch
        assert last.weight() == len(vals)
    assert _rank_errors(last, n, k) == 0


# ---------------------------------------------------------------- bytes
def test_bytes_round_trip():
    vals, valid = K.seeded()
    st = K.mirror_sketch(vals[:50_000], valid[:50_000], 64, 0.64, 4096)
    back = KLLState.from_bytes(st.to_bytes())
    assert back == st
    q, r = st.qSketch, back.qSketch
    assert (r.sketchSize, r.shrinkingFactor, r.curNumOfCompactors, r.compactorActualSize, r.compactorTotalSize) == \
        (q.sketchSize, q.shrinkingFactor, q.curNumOfCompactors, q.compactorActualSize, q.compactorTotalSize)
    assert back.to_bytes() == st.to_bytes()


def test_hand_assembled_bytes_decode():
    """KLLState.fromBytes (KLLSketch.scala:64-72): min, max, then KLLSketchSerializer.scala:83-115."""
    raw = struct.pack(">dd", 1.0, 6.0)                     # min, max
    raw += struct.pack(">id", 2, 0.64)                     # sketchSize, shrinkingFactor
    raw += struct.pack(">iii", 2, 4, 8)                    # curNumOfCompactors, actual, total
    raw += struct.pack(">i", 2)                            # compactors
    raw += struct.pack(">iii2d", 1, 0, 2, 5.0, 6.0)        # numOfCompress, offset, length, items
    raw += struct.pack(">iii2d", 0, 0, 2, 1.0, 3.0)
    st = KLLState.from_bytes(raw)
    assert (st.globalMin, st.globalMax) == (1.0, 6.0)
    assert st.qSketch.getCompactorItems() == [[5.0, 6.0], [1.0, 3.0]]
    assert [(c.numOfCompress, c.offset) for c in st.qSketch.compactors] == [(1, 0), (0, 0)]
    assert (st.qSketch.compactorActualSize, st.qSketch.compactorTotalSize) == (4, 8)
    assert st == K.mirror_sketch(np.arange(1.0, 7.0), None, 2, 0.64, 1 << 16)
    assert st.to_bytes() == raw


# ---------------------------------------------------------------- analyzer, metric, runner
def test_defaults_and_string_form():
    a = d.KLLSketch("att1")
    assert (a.sketchSize, a.shrinkingFactor, a.numberOfBuckets) == (2048, 0.64, 100)
    assert str(a) == "KLLSketch(att1,None)"
    assert str(d.KLLSketch("att1", d.KLLParameters(2, 0.64, 2))) == "KLLSketch(att1,Some(KLLParameters(2,0.64,2)))"
    assert d.KLLSketch("a", d.KLLParameters(2, 0.64, 2)) == d.KLLSketch("a", d.KLLParameters(2, 0.64, 2))
    assert len({d.KLLSketch("a"), d.KLLSketch("a"), d.KLLSketch("b")}) == 2


def test_precondition_messages():
    t = d.Table.from_pydict({"s": ("string", ["a"]), "b": ("bool", [True]), "x": ("float64", [1.0])})
    ctx = d.AnalysisRunner.onData(t).addAnalyzers([
        d.KLLSketch("x", d.KLLParameters(2048, 0.64, 101)), d.KLLSketch("s"), d.KLLSketch("b"), d.KLLSketch("nope")]).run()
    m = [ctx.metric(a) for a in ctx.metricMap]
    assert all(isinstance(x, d.KLLMetric) and x.value.isFailure for x in m)
    e = [x.value.exception for x in m]
    assert isinstance(e[0], d.IllegalAnalyzerParameterException)
    assert str(e[0]) == "Cannot return KLL Sketch related values for more than 100 values"
    assert isinstance(e[1], d.WrongColumnTypeException) and isinstance(e[2], d.WrongColumnTypeException)
    assert str(e[1]) == ("Expected type of column s to be one of (ByteType,ShortType,IntegerType,LongType,FloatType,"
                         "DoubleType,DecimalType), but found string instead!")
    assert isinstance(e[3], d.NoSuchColumnException) and str(e[3]) == "Input data does not include column nope!"
    flat = m[0].flatten()
    assert len(flat) == 1 and flat[0].name == "KLL.buckets" and flat[0].value.isFailure


def test_oversize_parameters_are_declined_with_the_bound():
    for k, c in ((50_000, 0.64), (2048, 1.0), (2048, 1.5)):
        with pytest.raises(L.UnsupportedOnGpu) as e:
            d.kll.check_parameters(k, c)
        assert "10112 items" in str(e.value) and "LDS" in str(e.value)
    d.kll.check_parameters(2048, 0.64)
    d.kll.check_parameters(2, 0.64)


def test_all_null_column_gives_zero_counts():
    st = K.mirror_sketch(np.zeros(30), np.zeros(30, dtype=bool), 2048, 0.64, 1 << 16)
    assert st == K.host_sketch(np.zeros(30), np.zeros(30, dtype=bool), 2048, 0.64, 1 << 16)
    assert (st.globalMin, st.globalMax) == (KLL_INIT_MIN, KLL_INIT_MAX)
    metric = d.KLLSketch("x", d.KLLParameters(2048, 0.64, 5)).computeMetricFrom(st)
    assert metric.value.isSuccess
    dist = metric.value.get()
    assert [b.count for b in dist.buckets] == [0] * 5 and dist.data == [[]]
    assert dist.buckets[0].lowValue == KLL_INIT_MIN and dist.buckets[-1].highValue == KLL_INIT_MAX
    flat = metric.flatten()
    assert [f.name for f in flat[:4]] == ["KLL.buckets", "KLL.low", "KLL.high", "KLL.count"] and len(flat) == 16
    assert d.KLLSketch("x").computeMetricFrom(None).value.isFailure  # no state at all: EmptyStateException


def test_metric_helpers():
    dist = d.BucketDistribution([d.BucketValue(0.0, 1.0, 3), d.BucketValue(1.0, 2.0, 7), d.BucketValue(2.0, 3.0, 7)],
                                [0.64, 2.0], [[5.0, 6.0], [1.0, 3.0]])
    assert dist.argmax() == 1 and dist[2].count == 7
    p = dist.computePercentiles()
    assert len(p) == 99 and p == sorted(p) and set(p) <= {1.0, 3.0, 5.0, 6.0}
    assert dist != d.BucketDistribution(dist.buckets, [0.64, 2.0], [[5.0, 6.0], [1.0, 4.0]])


def test_state_sum_and_run_on_aggregated_states():
    vals, valid = K.seeded()
    a = K.mirror_sketch(vals[:20_000], valid[:20_000], 64, 0.64, 4096)
    b = K.mirror_sketch(vals[20_000:45_000], valid[20_000:45_000], 64, 0.64, 4096)
    before = a.signature()
    s = a.sum(b)
    assert a.signature() == before  # (sum leaves its operands alone)
    want = a.qSketch.copy().merge(b.qSketch)
    assert s.qSketch.levels() == want.levels()
    assert s.qSketch.weight() == int(valid[:45_000].sum())
    assert (s.globalMin, s.globalMax) == (min(a.globalMin, b.globalMin), max(a.globalMax, b.globalMax))

    analyzer = d.KLLSketch("x", d.KLLParameters(64, 0.64, 10))
    p1, p2, out = d.InMemoryStateProvider(), d.InMemoryStateProvider(), d.InMemoryStateProvider()
    p1.persist(analyzer, a)
    p2.persist(analyzer, b)
    ctx = d.AnalysisRunner.runOnAggregatedStates({"x": "float64"}, d.Analysis([analyzer]), [p1, p2], saveStatesWith=out)
    metric = ctx.metric(analyzer)
    # the runner folds the loaders as merge(load(next), accumulated): the later state absorbs the
    # earlier one, and KLL's merge is not commutative (`this` keeps its numOfCompress / offset)
    folded = b.sum(a)
    assert metric.value.isSuccess and metric.value.get() == analyzer.computeMetricFrom(folded).value.get()
    assert sum(bk.count for bk in metric.value.get().buckets) == folded.qSketch.weight() == s.qSketch.weight()
    assert out.load(analyzer) == folded


def test_file_state_provider_refuses_kll(tmp_path):
    st = K.mirror_sketch(np.arange(1.0, 7.0), None, 2, 0.64, 1 << 16)
    provider = d.HdfsStateProvider(str(tmp_path / "states"))
    with pytest.raises(ValueError, match="Unable to persist state for analyzer KLLSketch"):
        provider.persist(d.KLLSketch("x"), st)
    with pytest.raises(ValueError, match="Unable to load state for analyzer KLLSketch"):
        provider.load(d.KLLSketch("x"))


def test_profile_json_carries_the_reference_kll_object():
    import json
    from deequ_amd.profiles import ColumnProfiles, NumericColumnProfile
    case = K.PROFILES[0]
    dist = d.BucketDistribution([d.BucketValue(*b) for b in case["buckets"]], case["parameters"], case["data"])
    prof = NumericColumnProfile("att1", 1.0, 6, d.DataTypeInstances.Fractional, False, {}, None, kll=dist, mean=3.5,
                                approxPercentiles=sorted(dist.computePercentiles()))
    j = json.loads(ColumnProfiles.toJson([prof]))["columns"][0]
    assert j["kll"] == {"buckets": [{"low_value": 1.0, "high_value": 3.5, "count": 4},
                                    {"low_value": 3.5, "high_value": 6.0, "count": 2}],
                        "sketch": {"parameters": {"c": 0.64, "k": 2.0}, "data": "[[5.0,6.0],[1.0,3.0]]"}}
    assert len(j["approxPercentiles"]) == 99
    plain = NumericColumnProfile("att1", 1.0, 6, d.DataTypeInstances.Fractional, False, {}, None)
    assert "kll" not in json.loads(ColumnProfiles.toJson([plain]))["columns"][0]
