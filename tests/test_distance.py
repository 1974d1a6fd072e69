"""Distance (analyzers/Distance.scala) on the host: the reference's known answers, the rank map
of a sketch, the NaN table and generated dict pairs against a restatement (distance_restated.py).
Everything is compared with `==` (NaN with NaN): the arithmetic is the reference's, operation for
operation, so there is no tolerance."""
import json
import math
import os
import random

import pytest

import deequ_amd as d
from deequ_amd import Distance
from deequ_amd._lib import UnsupportedOnGpu
from distance_restated import categorical, linf_simple, same

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "distance_known_answers.json")
with open(GOLDEN) as f:
    KNOWN = json.load(f)


def _sketch(levels, size=4, factor=0.64):
    q = d.QuantileNonSample(size, factor)
    q.reconstruct(size, factor, levels)
    return q


@pytest.mark.parametrize("case", KNOWN["numerical"], ids=lambda c: c["ref"].rsplit(":", 1)[1])
def test_known_numerical(case):
    s1 = _sketch(case["sample1"], case["sketchSize"], case["shrinkingFactor"])
    s2 = _sketch(case["sample2"], case["sketchSize"], case["shrinkingFactor"])
    assert Distance.numericalDistance(s1, s2, case["correctForLowNumberOfSamples"]) == case["expected"]
    k1, k2 = d.KLLState(s1, 4.0, 1.0), d.KLLState(s2, 5.0, 2.0)
    assert Distance.numericalDistance(k1, k2, case["correctForLowNumberOfSamples"]) == case["expected"]


@pytest.mark.parametrize("case", KNOWN["categorical"], ids=lambda c: c["ref"].rsplit(":", 1)[1])
def test_known_categorical(case):
    got = Distance.categoricalDistance(case["sample1"], case["sample2"], case["correctForLowNumberOfSamples"])
    assert got == case["expected"]
    assert categorical(case["sample1"], case["sample2"], case["correctForLowNumberOfSamples"]) == case["expected"]


def test_default_is_the_robust_variant():
    c = KNOWN["categorical"][2]
    assert Distance.categoricalDistance(c["sample1"], c["sample2"]) == 0.0
    assert Distance.categoricalDistance(c["sample1"], c["sample2"], True) == c["expected"]


# ---- the rank map (QuantileNonSample.scala:126-155, 194-205), restated here
def _rank_map(levels):
    """ListMap(output.sortBy(item)) keeps one entry per item, the last of equal ones with its own
    weight; the running ranks are accumulated over those entries."""
    output = [(float(v), 1 << i) for i, level in enumerate(levels) for v in level]
    output.sort(key=lambda iw: iw[0])  # (stable)
    kept = []
    for v, w in output:
        if kept and kept[-1][0] == v:
            kept[-1] = (v, w)
        else:
            kept.append((v, w))
    ranks, running = [], 0
    for v, w in kept:
        running += w
        ranks.append((v, running))
    return ranks


def _rank_of(item, ranks):
    cur = 0
    for v, r in ranks:
        if v > item:
            break
        cur = r
    return cur


def _grown_sketch(seed, n, distinct):
    rng = random.Random(seed)
    q = d.QuantileNonSample(8, 0.64)
    q.updateAll([float(rng.randrange(distinct)) for _ in range(n)])
    return q


def test_rank_map_of_a_worked_sketch():
    q = _sketch([[1, 1, 2], [2, 3]])
    # sorted (item, weight): (1,1) (1,1) (2,1) (2,2) (3,2); one entry per item: 1->1, 2->2, 3->2
    assert list(q.getRankMap().items()) == [(1.0, 1), (2.0, 3), (3.0, 5)]
    assert q.getCDF() == [(1.0, 1 / 5), (2.0, 3 / 5), (3.0, 5 / 5)]
    rm = q.getRankMap()
    assert [q.getRank(x, rm) for x in (0.5, 1.0, 1.5, 2.0, 2.5, 3.0, 9.0)] == [0, 1, 1, 3, 3, 5, 5]
    assert q.getRank(2.0) == 5  # (the overload without a map counts every item)


@pytest.mark.parametrize("seed,n,distinct", [(1, 200, 10 ** 6), (2, 500, 40), (3, 3000, 300), (4, 37, 5)])
def test_rank_map_matches_restatement(seed, n, distinct):
    q = _grown_sketch(seed, n, distinct)
    levels = q.getCompactorItems()
    assert len(levels) > 1 or n < 40
    if distinct < n:
        flat = [v for level in levels for v in level]
        assert len(set(flat)) < len(flat)  # duplicates present
    want = _rank_map(levels)
    assert list(q.getRankMap().items()) == want
    total = float(want[-1][1])
    assert q.getCDF() == [(v, float(r) / total) for v, r in want]
    rm = q.getRankMap()
    rng = random.Random(seed + 100)
    probes = [v for v, _ in want] + [rng.uniform(-2.0, distinct + 2.0) for _ in range(50)]
    assert [q.getRank(x, rm) for x in probes] == [_rank_of(x, want) for x in probes]


@pytest.mark.parametrize("flag", [False, True])
def test_numerical_distance_matches_restatement(flag):
    a, b = _grown_sketch(5, 2000, 500), _grown_sketch(6, 700, 650)
    ra, rb = _rank_map(a.getCompactorItems()), _rank_map(b.getCompactorItems())
    n, m = float(max(r for _, r in ra)), float(max(r for _, r in rb))
    linf = 0.0
    for key in {v for v, _ in ra} | {v for v, _ in rb}:
        linf = max(linf, abs(_rank_of(key, ra) / n - _rank_of(key, rb) / m))
    want = linf if flag else max(0.0, linf - 1.8 * math.sqrt((n + m) / (n * m)))
    assert Distance.numericalDistance(a, b, flag) == want
    assert Distance.numericalDistance(a, a.copy(), True) == 0.0


def test_numerical_distance_of_an_empty_sketch_raises():
    full, empty = _sketch([[1, 2, 3]]), d.QuantileNonSample(4, 0.64)
    for pair in ((full, empty), (empty, full), (empty, empty)):
        with pytest.raises(ValueError):
            Distance.numericalDistance(*pair)
    with pytest.raises(ValueError):
        empty.getCDF()
    assert empty.getRankMap() == {}
    with pytest.raises(TypeError):
        Distance.numericalDistance(full, {"a": 1})


# ---- the NaN table (0L / 0.0 is NaN; Math.max keeps it)
def test_nan_table():
    some = {"a": 3, "b": 1}
    for flag in (True, False):
        assert math.isnan(Distance.categoricalDistance({}, some, flag))
        assert math.isnan(Distance.categoricalDistance(some, {}, flag))
    assert Distance.categoricalDistance({}, {}, True) == 0.0
    assert math.isnan(Distance.categoricalDistance({}, {}))  # sqrt(0 / 0)
    assert math.isnan(Distance.categoricalDistance({"a": 0}, some, True))  # a total of zero


class _State:
    """Stands in for a device state (table + numRows) where no GPU is at hand."""
    table, numRows = None, 0


def test_dict_with_state_raises_type_error():
    for pair in (({"a": 1}, _State()), (_State(), {"a": 1}), ({"a": 1}, [("a", 1)]), (None, {"a": 1})):
        with pytest.raises(TypeError):
            Distance.categoricalDistance(*pair)


def test_state_that_is_not_one_table_is_unsupported():
    with pytest.raises(UnsupportedOnGpu, match="single-device"):
        Distance.categoricalDistance(_State(), _State())


# ---- generated pairs
def _pairs(seed=20240, count=300):
    rng = random.Random(seed)
    for i in range(count):
        na, nb = rng.randrange(0, 41), rng.randrange(0, 41)
        keys_a = ["k%d" % j for j in range(na)]
        if i % 3 == 0:    # no key shared
            keys_b = ["x%d" % j for j in range(nb)]
        elif i % 3 == 1:  # the same keys
            keys_b = list(keys_a)
        else:             # some shared, some only in b
            p = rng.random()
            shared = [k for k in keys_a if rng.random() < p]
            keys_b = shared + ["x%d" % j for j in range(max(0, nb - len(shared)))]
        big = i % 5 == 0
        count_of = lambda: rng.randrange(1, 2 ** 40 + 1) if big or rng.random() < 0.2 else rng.randrange(1, 50)  # noqa: E731
        yield {k: count_of() for k in keys_a}, {k: count_of() for k in keys_b}


def test_generated_pairs_match_restatement():
    sizes, overlaps, top = set(), set(), 0
    for a, b in _pairs():
        sizes.update((len(a), len(b)))
        common = len(set(a) & set(b))
        overlaps.add("none" if common == 0 else "full" if common == len(a) == len(b) else "some")
        top = max([top] + list(a.values()) + list(b.values()))
        for flag in (True, False):
            got = Distance.categoricalDistance(a, b, flag)
            want = categorical(a, b, flag)
            assert same(got, want), (a, b, flag, got, want)
        linf, n, m = linf_simple(a, b)
        assert Distance.categoricalDistance(b, a, True) == linf or (linf != linf)
    assert {0, 40} <= sizes and overlaps == {"none", "full", "some"} and top > 2 ** 39
