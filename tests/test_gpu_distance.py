"""Distance.categoricalDistance over two device states (dq_freq_linf_distance, dq_freq.hip
"Distance") against the restatement of Distance.scala:43-87 (distance_restated.py) evaluated over
`frequencies(raw=True)` of both states: linf_simple, both totals and the three group counts, all
exact.  groups_common is checked everywhere: a probe that misses a class of keys can leave the
maximum untouched.

The shapes are the smallest at which the kernel can still go wrong: every key form (inline in one
word, inline in two, heap; int64; composite) with the maximum planted on it from either side,
tables of different capacity (the slice bits differ), a table of more slots than one trip of the
grid covers, every way a table comes to be (sorted and atomic group-by, a compacted table, an
import, a merge), Histogram's NULL keys and string-keyed states, counts near 2^40 and the
declined totals above 2^53."""
import ctypes
import math
import struct

import numpy as np
import pytest

import deequ_amd as d
from deequ_amd import Distance, _lib as L
from deequ_amd.frequencies import FrequenciesAndNumRows, FrequencyTable, encode_key
from distance_restated import categorical, linf_simple, same

pytestmark = pytest.mark.gpu

# dq_internal.h: kFreqDistMaxBlocks workgroups of kBlock threads, one slot per thread and trip
GRID_CAP_BLOCKS, BLOCK = 2048, 256


def _raw(t):
    return FrequenciesAndNumRows(t).frequencies(raw=True) if isinstance(t, FrequencyTable) else t.frequencies(raw=True)


def _check(a, b, fa=None, fb=None, r=None):
    """a.linf_distance(b) (or its result `r`, taken before the export) against the restatement."""
    r = a.linf_distance(b) if r is None else r
    fa = _raw(a) if fa is None else fa
    fb = _raw(b) if fb is None else fb
    linf, n, m = linf_simple(fa, fb)
    assert (r.n, r.m) == (int(n), int(m))
    assert (r.groups_a, r.groups_b, r.groups_common) == (len(fa), len(fb), len(set(fa) & set(fb)))
    assert same(r.linf_simple, linf), (r.linf_simple, linf)
    return r


def _argmax(fa, fb):
    n, m = float(sum(fa.values())), float(sum(fb.values()))
    return max(set(fa) | set(fb), key=lambda k: abs(fa.get(k, 0) / n - fb.get(k, 0) / m))


def _imported(groups, dtypes=("string",), histogram=False):
    """A table holding {encoded key: count} (dq_freq_import_flat)."""
    cols = ["c%d" % i for i in range(len(dtypes))]
    t = FrequencyTable(cols, dict(zip(cols, dtypes)), histogram)
    t.import_groups(list(groups.values()), list(groups.keys()), sum(groups.values()))
    return t


def _consumed(keys, histogram=False, dtype="string"):
    t = FrequencyTable(["c0"], {"c0": dtype}, histogram)
    t.consume(d.Table.from_pydict({"c0": (dtype, keys)}))
    return t


def _uuid(v: int) -> str:
    x = (v * 0x9E3779B97F4A7C15 + 0x632BE59BD9B4E019) % 2 ** 64
    y = ((v ^ 0x5DEECE66D) * 0xC2B2AE3D27D4EB4F) % 2 ** 64
    h = "%016x%016x" % (x, y)
    return "%s-%s-%s-%s-%s" % (h[:8], h[8:12], h[12:16], h[16:20], h[20:32])


def _spec_keys(n, seed):
    """The string column of test_gpu_freq_paths._spec: ~n/3 distinct "k%d" keys, NULLs."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, n // 3 + 1, n)
    return [None if i % 19 == 0 else "k%d" % a[i] for i in range(n)]


# ---------------------------------------------------------------- the reference's known answers
KNOWN = [({"a": 10, "b": 20, "c": 25, "d": 10, "e": 5}, {"a": 11, "b": 20, "c": 25, "d": 10, "e": 10}, True,
          0.06015037593984962),
         ({"a": 10, "b": 20, "c": 25, "d": 10, "e": 5}, {"a": 11, "b": 20, "c": 25, "d": 10, "e": 10}, False, 0.0),
         ({"a": 10, "b": 20, "c": 25, "d": 10, "e": 5}, {"f": 11, "a": 20, "c": 25, "d": 10, "e": 10}, True,
          0.2857142857142857),
         ({"a": 10, "b": 20, "c": 25, "d": 10, "e": 5}, {"f": 11, "a": 20, "c": 25, "d": 10, "e": 10}, False, 0.0)]


@pytest.mark.parametrize("s1,s2,flag,expected", KNOWN)
def test_known_answers_as_device_states(gpu, s1, s2, flag, expected):
    a = FrequenciesAndNumRows.from_frequencies(["v"], ["string"], {(k,): c for k, c in s1.items()}, sum(s1.values()))
    b = FrequenciesAndNumRows.from_frequencies(["v"], ["string"], {(k,): c for k, c in s2.items()}, sum(s2.values()))
    assert Distance.categoricalDistance(a, b, flag) == expected
    r = _check(a.table, b.table)
    assert r.groups_common == len(set(s1) & set(s2))
    same_r = a.table.linf_distance(a.table)  # a == b is allowed
    assert (same_r.linf_simple, same_r.groups_common, same_r.n, same_r.m) == (0.0, 5, r.n, r.n)


# ---------------------------------------------------------------- key forms
def _form_tables(family):
    """~200 groups per table with every form of the family present, about two thirds shared:
    {form: [encoded keys]}, dtypes."""
    if family == "string":
        forms = {"short": [("s%d" % i).encode() for i in range(70)],                        # <= 8 bytes
                 "mid": [("middle-%06d" % i).encode() for i in range(70)],                  # 9..16 bytes
                 "digits": [("%012d" % (i * 7919)).encode() for i in range(70)],            # hashed as a packed word
                 "long": [("a-key-longer-than-sixteen-bytes-%d" % i).encode() for i in range(70)]}  # heap
        return forms, ("string",)
    if family == "int64":
        return {"int64": [struct.pack("<q", (i - 100) * 2654435761) for i in range(210)]}, ("int64",)
    forms = {"composite_inline": [encode_key([i * 7919, "ab%d" % (i % 10)], ["int64", "string"]) for i in range(105)],
             "composite_heap": [encode_key([i * 7919, "a-longer-string-part-%d" % i], ["int64", "string"])
                                for i in range(105)]}
    assert all(len(k) <= 16 for k in forms["composite_inline"]) and all(len(k) > 16 for k in forms["composite_heap"])
    return forms, ("int64", "string")


FORMS = [("string", "short"), ("string", "mid"), ("string", "digits"), ("string", "long"), ("int64", "int64"),
         ("composite", "composite_inline"), ("composite", "composite_heap")]


@pytest.mark.parametrize("where", ["only_a", "only_b", "both"])
@pytest.mark.parametrize("family,form", FORMS)
def test_key_forms_with_planted_maximum(gpu, family, form, where):
    forms, dtypes = _form_tables(family)
    rng = np.random.default_rng(7)
    fa, fb = {}, {}
    for keys in forms.values():
        for i, k in enumerate(keys):
            c = int(rng.integers(1, 20))
            if i % 3 != 1:
                fa[k] = c
            if i % 3 != 2:
                fb[k] = c + int(rng.integers(0, 2))
    planted = forms[form][{"only_a": 2, "only_b": 1, "both": 0}[where]]  # (i % 3: in a alone, b alone, both)
    assert (planted in fa, planted in fb) == {"only_a": (True, False), "only_b": (False, True), "both": (True, True)}[where]
    if where == "only_b":
        fb[planted] = 5000
    else:
        fa[planted] = 5000
    assert _argmax(fa, fb) == planted
    a, b = _imported(fa, dtypes), _imported(fb, dtypes)
    r = _check(a, b, fa, fb)
    assert 0 < r.groups_common < min(len(fa), len(fb))
    rb = _check(b, a, fb, fa)
    assert same(rb.linf_simple, r.linf_simple)


# ---------------------------------------------------------------- tables of different capacity
@pytest.fixture(scope="module")
def big_keys():
    keys = _spec_keys(20000, 1)
    want = {}
    for k in keys:
        if k is not None:
            want[k.encode()] = want.get(k.encode(), 0) + 1
    return keys, want


@pytest.mark.parametrize("small", ["inside", "disjoint", "mixed"])
def test_different_capacities(gpu, big_keys, small):
    keys, fb = big_keys
    b = _consumed(keys)
    some = sorted(fb)[:3]
    fa = {"inside": {k: 4 + i for i, k in enumerate(some)},
          "disjoint": {b"zz-1": 3, b"zz-2": 1, b"a-key-longer-than-sixteen-bytes": 2},
          "mixed": {some[0]: 9, some[1]: 1, b"zz-3": 5}}[small]
    a = _imported(fa)
    assert len(fb) > 5000
    r = _check(a, b, fa, fb)
    assert r.groups_common == {"inside": 3, "disjoint": 0, "mixed": 2}[small]
    _check(b, a, fb, fa)


@pytest.mark.parametrize("small", [3, 200])
def test_different_slice_bits(gpu, small):
    """A fresh table has 2^16 slots and keeps them up to 39 321 groups, so the 7 000-group pairs
    above share their slice bits: 45 000 groups make a table of 2^17 slots, and a key's slice
    index differs between the two tables."""
    rng = np.random.default_rng(17)
    fb = {("g%d" % i).encode() if i % 4 else ("a-group-key-beyond-16-bytes-%d" % i).encode(): int(rng.integers(1, 30))
          for i in range(45_000)}
    fa = {k: c + 2 for k, c in list(fb.items())[::45_000 // small][:small]}
    fa[b"only-in-a"] = 7
    a, b = _imported(fa), _imported(fb)
    assert a.paths()["slots"] == 1 << 16 and b.paths()["slots"] == 1 << 17
    assert _check(a, b, fa, fb).groups_common == len(fa) - 1
    assert _check(b, a, fb, fa).groups_common == len(fa) - 1


def test_identical_and_subset_pairs(gpu, big_keys):
    keys, fb = big_keys
    b = _consumed(keys)
    twin = _consumed(list(reversed(keys)))
    r = _check(b, twin, fb, fb)
    assert (r.linf_simple, r.groups_common) == (0.0, len(fb))
    sub = {k: c for i, (k, c) in enumerate(sorted(fb.items())) if i % 2 == 0}
    s = _imported(sub)
    assert _check(s, b, sub, fb).groups_common == len(sub)
    assert _check(b, s, fb, sub).groups_common == len(sub)


# ---------------------------------------------------------------- past one trip of the grid
def _two_trip_pair():
    """Two int64-keyed tables of 2^20 slots (330 000 groups each, half shared): twice the
    GRID_CAP_BLOCKS * BLOCK = 524 288 slots one trip of the capped grid covers."""
    n = 330_000
    rng = np.random.default_rng(11)
    tabs = []
    for lo in (0, n // 2):
        keys = np.arange(lo, lo + n, dtype=np.int64) * 1_000_003
        t = FrequencyTable(["v"], {"v": "int64"})
        t.import_flat(rng.integers(1, 10, n), np.arange(n + 1, dtype=np.int64) * 8, keys.view(np.uint8), 0)
        tabs.append(t)
    return tabs


@pytest.mark.parametrize("end", ["first", "last"])
def test_second_grid_stride_trip(gpu, end):
    a, b = _two_trip_pair()
    assert a.paths()["slots"] >= 2 * GRID_CAP_BLOCKS * BLOCK and b.paths()["slots"] >= 2 * GRID_CAP_BLOCKS * BLOCK
    _, order = a.export()  # slot order
    planted = order[0] if end == "first" else order[-1]
    a.import_groups([10 ** 7 if end == "first" else 10 ** 9], [planted], 0)  # (the key keeps its slot)
    fa, fb = _raw(a), _raw(b)
    assert a.export()[1][0 if end == "first" else -1] == planted and _argmax(fa, fb) == planted
    r = _check(a, b, fa, fb)
    assert r.groups_common == 165_000
    _check(b, a, fb, fa)


# ---------------------------------------------------------------- every way a table comes to be
@pytest.mark.parametrize("path", ["sorted", "atomic"])
def test_consumed_on_each_path(gpu, monkeypatch, big_keys, path):
    monkeypatch.setenv("DQ_FREQ_PATH", path)
    keys, fa = big_keys
    a = _consumed(keys)
    p = a.paths()
    if path == "sorted":
        assert p["sort_records"] > 0
    else:
        assert (p["sort_records"], p["partition_runs"], p["small_runs"]) == (0, 0, 0)
    other = _spec_keys(9000, 5)
    b = _consumed(other)
    r = _check(a, b, fa)
    assert 0 < r.groups_common < r.groups_b


def test_compacted_table(gpu, monkeypatch):
    """The shape of test_gpu_freq_hashed.test_hashed_operations_after: 600 000 UUID rows on the
    partition path leave the table compacted; the call expands it (the slot image is probed)."""
    monkeypatch.setenv("DQ_FREQ_PART_MIN", "1")
    monkeypatch.setenv("DQ_FREQ_PATH", "sorted")
    rng = np.random.default_rng(42)
    k1 = [_uuid(int(v)) for v in rng.integers(0, 600_000, 600_000)]
    t = FrequencyTable(["c0"], {"c0": "string"})
    t.reserve(len(k1))
    for s in range(0, len(k1), 300_000):
        t.consume(d.Table.from_pydict({"c0": ("string", k1[s:s + 300_000])}))
    assert t.paths()["compacted"] == 1
    fb = {_uuid(v).encode(): 1 + v % 3 for v in range(0, 600_000, 7)}
    b = _imported(fb)
    r = t.linf_distance(b)
    assert t.paths()["compacted"] == 0
    _check(t, b, None, fb, r)
    assert 0 < r.groups_common < r.groups_b
    _check(b, t, fb)


def test_from_arrow_and_merged_tables(gpu, big_keys):
    import pyarrow as pa
    keys, fa = big_keys
    names = [k.decode() for k in sorted(fa)[::3]] + ["only-in-the-arrow-state", "another-key-longer-than-16-bytes"]
    arrow = pa.table({"v": pa.array(names, pa.string()), "count": pa.array(list(range(1, len(names) + 1)), pa.int64())})
    st = FrequenciesAndNumRows.from_arrow(arrow, ["v"], ["string"], 0)
    a = _consumed(keys)
    r = _check(a, st.table, fa)
    assert r.groups_common == len(names) - 2
    merged = FrequencyTable.like(a)
    merged.merge_from(a)
    merged.merge_from(st.table)  # a table that has received a merge
    r = _check(merged, a, None, fa)
    assert (r.groups_a, r.groups_common) == (len(fa) + 2, len(fa))
    _check(st.table, merged)


# ---------------------------------------------------------------- Histogram states
def test_histogram_null_keys(gpu):
    sa = ["x", None, "y", None, "NullValue", "a-value-longer-than-sixteen-bytes", None]
    sb = ["x", "x", None, "z"]
    a, b = _consumed(sa, True), _consumed(sb, True)
    r = _check(a, b)
    assert _raw(a)[b"NullValue"] == 4 and r.groups_common == 2
    ia, ib = _consumed([1, None, 2, None, None, 7], True, "int64"), _consumed([None, 2, 2, 9], True, "int64")
    r = _check(ia, ib)
    assert _raw(ia)[b""] == 3 and r.groups_common == 2


def test_histogram_int_state_against_string_keyed_state(gpu):
    fresh = FrequenciesAndNumRows(_consumed([5, 5, None, 12, -3, 12, 5], True, "int64"))
    other = FrequenciesAndNumRows(_consumed([5, None, None, 40, -3], True, "int64")).as_string_keys()
    assert fresh.table.dtypes == ["int64"] and other.table.dtypes == ["string"]
    fa, fb = fresh.as_string_keys().frequencies(raw=True), other.frequencies(raw=True)
    assert fa[b"NullValue"] == 1 and fb[b"NullValue"] == 2
    for flag in (True, False):
        assert same(Distance.categoricalDistance(fresh, other, flag), categorical(fa, fb, flag))
    assert Distance.categoricalDistance(fresh, other, True) == 2 / 7  # "12": only in the fresh state
    plain = FrequenciesAndNumRows(_consumed([5, 12], False, "int64"))
    with pytest.raises(ValueError):
        Distance.categoricalDistance(fresh, plain)
    with pytest.raises(TypeError):
        Distance.categoricalDistance(fresh, {"5": 3})


# ---------------------------------------------------------------- large counts
def test_counts_near_2_40_are_bit_equal(gpu):
    rng = np.random.default_rng(13)
    keys = [("key-%d" % i).encode() for i in range(300)] + [("a-long-key-beyond-sixteen-bytes-%d" % i).encode() for i in range(40)]
    fa = {k: int(rng.integers(2 ** 40 - 2 ** 20, 2 ** 40 + 2 ** 20)) for k in keys[:250]}
    fb = {k: int(rng.integers(2 ** 39, 2 ** 41)) for k in keys[120:]}
    r = _check(_imported(fa), _imported(fb), fa, fb)
    assert r.n > 2 ** 47 and 0.0 < r.linf_simple < 1.0


def test_totals_at_and_above_2_53(gpu):
    small = _imported({b"x": 1, b"y": 2})
    at = {b"x": 2 ** 52, b"y": 2 ** 52}  # 2^53 exactly: still exact
    _check(_imported(at), small, at)
    over = _imported({b"x": 2 ** 52, b"y": 2 ** 52, b"z": 1})
    for pair in ((over, small), (small, over)):
        with pytest.raises(L.UnsupportedOnGpu, match="2\\^53") as e:
            pair[0].linf_distance(pair[1])
        assert e.value.status == L.DQ_ERR_UNSUPPORTED


# ---------------------------------------------------------------- the inputs stay as they were
def test_inputs_untouched(gpu, big_keys):
    keys, fa = big_keys
    a = _consumed(keys)
    fb = {k: c + 1 for k, c in list(sorted(fa.items()))[::2]}
    fb[b"a-key-only-in-b-and-longer-than-16"] = 3
    b = _imported(fb)

    def image(t):
        s = t.summary()
        counts, ks = t.export()
        probes = sorted(fa)[:20] + [b"absent", b"a-key-only-in-b-and-longer-than-16"]
        return ((s.num_rows, s.num_groups, s.num_unique, s.grouped_rows, s.entropy), counts.tolist(), ks,
                [t.lookup(k) for k in probes])

    before = image(a), image(b)
    _check(a, b, fa, fb)
    _check(b, a, fb, fa)
    assert (image(a), image(b)) == before
    more = ["k1", "k2", "fresh-key", None, "k1"]
    a.consume(d.Table.from_pydict({"c0": ("string", more)}))
    want = dict(fa)
    for k in more:
        if k is not None:
            want[k.encode()] = want.get(k.encode(), 0) + 1
    assert _raw(a) == want
    a.merge_from(b)
    for k, c in fb.items():
        want[k] = want.get(k, 0) + c
    assert _raw(a) == want and _raw(b) == fb
    _check(a, b, want, fb)


# ---------------------------------------------------------------- arguments
def test_argument_errors(gpu):
    s = _imported({b"x": 1})
    i = _imported({struct.pack("<q", 1): 1}, ("int64",))
    h = _imported({b"x": 1}, histogram=True)
    two = _imported({encode_key([1, 2], ["int64", "int64"]): 1}, ("int64", "int64"))
    for other, text in ((i, "different key types"), (h, "different keys"), (two, "different keys")):
        with pytest.raises(L.DeequAmdError, match=text) as e:
            s.linf_distance(other)
        assert e.value.status == L.DQ_ERR_INVALID
    out = L.DqFreqDistance()
    lib = L.lib()
    assert lib.dq_freq_linf_distance(None, s.handle, ctypes.byref(out)) == L.DQ_ERR_INVALID
    assert lib.dq_freq_linf_distance(s.handle, None, ctypes.byref(out)) == L.DQ_ERR_INVALID
    assert lib.dq_freq_linf_distance(s.handle, s.handle, None) == L.DQ_ERR_INVALID


def test_empty_sides(gpu):
    fa = {b"x": 3, b"a-key-longer-than-sixteen-bytes": 1}
    a, e1, e2 = _imported(fa), FrequencyTable(["c0"], {"c0": "string"}), FrequencyTable(["c0"], {"c0": "string"})
    for x, y, n, m, ga, gb in ((a, e1, 4, 0, 2, 0), (e1, a, 0, 4, 0, 2)):
        r = x.linf_distance(y)
        assert math.isnan(r.linf_simple) and (r.n, r.m, r.groups_a, r.groups_b, r.groups_common) == (n, m, ga, gb, 0)
    r = e1.linf_distance(e2)
    assert (r.linf_simple, r.n, r.m, r.groups_a, r.groups_b, r.groups_common) == (0.0, 0, 0, 0, 0, 0)
    sa, s1, s2 = FrequenciesAndNumRows(a), FrequenciesAndNumRows(e1), FrequenciesAndNumRows(e2)
    assert math.isnan(Distance.categoricalDistance(sa, s1)) and math.isnan(Distance.categoricalDistance(s1, sa, True))
    assert Distance.categoricalDistance(s1, s2, True) == 0.0
    assert math.isnan(Distance.categoricalDistance(s1, s2))  # sqrt(0 / 0)
    zero = _imported({b"x": 0, b"y": 0})  # groups, but a total of zero: 0L / 0.0 for every key
    r = zero.linf_distance(a)
    assert math.isnan(r.linf_simple) and (r.n, r.groups_a, r.groups_common) == (0, 2, 1)
