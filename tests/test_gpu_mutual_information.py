"""MutualInformation over a device state (dq_freq_mutual_information, dq_freq.hip
"MutualInformation") against the restatement of MutualInformation.scala:38-81 (mi_restated.py)
evaluated over `frequencies(raw=True)` of the state, each raw joint key split into its two fields'
bytes here in Python (the exact identity of a group: NaN, -0.0 and 0.0 stay apart).

Exact fields: num_rows, groups, groups_a and groups_b equal the restatement's in every case.

Value: |mi - fsum| <= 8 * 2^-52 * sum|t| + groups * 2^-96.  Derived, not measured: both sides
compute the same ratio bit for bit (IEEE division and multiplication in one order); the device
log is specified to 3 ulp at most and libm's to 1, and the product p * log rounds once on each side,
so a term differs by less than (3 + 1 + 1/2 + 1/2) ulp <= 8 * 2^-53 * 2 |t|; a term's fixed-point
rounding adds at most 2^-97, fsum's and the final rounding of the sum are inside the slack.

Shapes are the smallest at which the kernels can still go wrong: every key form (inline and heap
joint keys, inline and heap fields, digit strings, floats by bit pattern, an empty field) at 3
groups and at ~7 000 (the workgroups' LDS tables overflow, several workgroups), the 16 / 17 byte
boundaries of fields and joint keys, 100 000 groups onto 2 marginal groups (contention) with counts
above 2^33, tables past 2^16 slots and past one trip of the capped grid, and every refusal."""
import ctypes
import math
import struct

import numpy as np
import pytest

import deequ_amd as d
from deequ_amd import _lib as L
from deequ_amd.frequencies import (FrequenciesAndNumRows, FrequencyTable, compute_frequencies, decode_key, encode_key)
from mi_restated import restate

pytestmark = pytest.mark.gpu

# dq_internal.h: kFreqDistMaxBlocks workgroups of kBlock threads, one slot per thread and trip
GRID_CAP_BLOCKS, BLOCK = 2048, 256
_WIDTH = {"bool": 1, "int8": 1, "int16": 2, "int32": 4, "int64": 8, "float32": 4, "float64": 8}


def _bits(x: float) -> int:
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def _fields(key: bytes, dtypes):
    """A raw joint key -> its two fields' bytes (a string without its length prefix)."""
    out, pos = [], 0
    for t in dtypes:
        if t == "string":
            n = struct.unpack_from("<I", key, pos)[0]
            pos += 4
        else:
            n = _WIDTH[t]
        out.append(key[pos:pos + n])
        pos += n
    assert pos == len(key)
    return tuple(out)


def _state(dtypes, joint, num_rows=None, columns=("a", "b")):
    return FrequenciesAndNumRows.from_frequencies(list(columns), list(dtypes), joint,
                                                  sum(joint.values()) if num_rows is None else num_rows)


def _check(state, expect_raw=None, label=""):
    """state.table.mutual_information() against the restatement over the state's own raw groups."""
    r = state.table.mutual_information()
    raw = state.frequencies(raw=True)
    if expect_raw is not None:
        assert raw == expect_raw
    dtypes = state.table.dtypes
    joint = {_fields(k, dtypes): c for k, c in raw.items()}
    assert len(joint) == len(raw)
    want = restate(joint, state.numRows)
    assert (r.num_rows, r.groups, r.groups_a, r.groups_b) == (state.numRows, len(raw), want.groups_a, want.groups_b)
    if math.isnan(want.fsum):
        assert math.isnan(r.mi)
        return r, want
    bound = 8 * 2.0 ** -52 * want.sum_abs + len(raw) * 2.0 ** -96
    err = abs(r.mi - want.fsum)
    print("mi_error %-28s groups=%-7d mi=%.17g err=%.3g bound=%.3g ulps_of_sum_abs=%.3f"
          % (label, len(raw), r.mi, err, bound, err / (2.0 ** -52 * want.sum_abs) if want.sum_abs else 0.0))
    assert err <= bound, (r.mi, want.fsum, err, bound)
    return r, want


def _raw(dtypes, joint):
    return {encode_key(k, dtypes): c for k, c in joint.items()}


# ---------------------------------------------------------------- exact zero
def test_independent_dyadic_columns_are_exactly_zero(gpu):
    """cA = [1, 3, 4], cB = [2, 6, 8], joint = cA[i] * cB[j], numRows = 128: every ratio is exactly
    1.0 and mi == 0.0; one NULL-key row more (129) and the ratios round, back under the bound."""
    joint = {(i, "b%d" % j): ca * cb for i, ca in enumerate([1, 3, 4]) for j, cb in enumerate([2, 6, 8])}
    s = _state(("int32", "string"), joint, 128)
    r, want = _check(s, label="dyadic")
    assert want.fsum == 0.0 and r.mi == 0.0 and not math.copysign(1.0, r.mi) < 0
    assert (r.groups, r.groups_a, r.groups_b) == (9, 3, 3)
    s = _state(("int32", "string"), joint, 129)
    r, want = _check(s, label="dyadic+null")
    assert r.num_rows == 129 and want.fsum != 0.0


# ---------------------------------------------------------------- key forms
def _nan32():
    return struct.unpack("<f", struct.pack("<I", 0x7FC00000))[0]


FORMS = {
    "int64,int64": (("int64", "int64"), lambda i: (i - 40) * 1_000_003, lambda j: -(j * 7919) - 1),
    "int32,short-string": (("int32", "string"), lambda i: i - 50, lambda j: "s%d" % j),
    "string,string-inline": (("string", "string"), lambda i: "a%d" % i, lambda j: "b%02d" % j),
    "int64,40-byte-string": (("int64", "string"), lambda i: i * 65_537, lambda j: "forty-bytes-of-category-name-%010d" % j),
    "20-byte-string,int8": (("string", "int8"), lambda i: "twenty-byte-key-%04d" % i, lambda j: j - 64),
    "12-digit-string,bool": (("string", "bool"), lambda i: "%012d" % (i * 7919 + 100_000_000_000), lambda j: bool(j)),
    "float64,float32": (("float64", "float32"), None, None),
    "empty-string,string": (("string", "string"), lambda i: "", lambda j: "value-%d" % j),
    "same-column-twice": (("int64", "int64"), None, None),
}
# marginal sizes of the ~7 000-group cases (na * nb >= 7 000; bool and int8 bound a side)
BIG = {"int64,int64": (100, 100), "int32,short-string": (90, 110), "string,string-inline": (120, 90),
       "int64,40-byte-string": (350, 30), "20-byte-string,int8": (70, 120), "12-digit-string,bool": (3600, 2),
       "float64,float32": (100, 100), "empty-string,string": (1, 7000)}


def _float_values(n, kind):
    """Distinct bit patterns: NaN, -0.0, 0.0 first (Python's == conflates the zeros, and a NaN equals
    nothing: such keys are only ever handled as their encoded bytes)."""
    special = [float("nan"), -0.0, 0.0, float("inf")] if kind == "float64" else [_nan32(), -0.0, 0.0, 1.5]
    return special[:n] + [(i + 10) * 0.25 for i in range(max(0, n - len(special)))]


def _form_raw(form, big):
    """dtypes, {encoded joint key: count} of a form at 3 or at 7 000 groups."""
    dtypes, fa, fb = FORMS[form]
    rng = np.random.default_rng(len(form) * 31 + big)
    if form == "same-column-twice":
        vals = [(i - 3000) * 1_000_003 for i in range(7000 if big else 3)]
        return dtypes, {encode_key((v, v), dtypes): int(rng.integers(1, 60)) for v in vals}
    if form == "float64,float32" and not big:
        pairs = [(float("nan"), -0.0), (-0.0, 0.0), (0.0, _nan32())]
        return dtypes, {encode_key(k, dtypes): c for k, c in zip(pairs, (5, 2, 9))}
    na, nb = BIG[form] if big else ((1, 3) if form == "empty-string,string" else (2, 2))
    va = _float_values(na, "float64") if fa is None else [fa(i) for i in range(na)]
    vb = _float_values(nb, "float32") if fb is None else [fb(j) for j in range(nb)]
    n = 7000 if big else 3
    picks = rng.choice(na * nb, size=min(n, na * nb), replace=False)
    return dtypes, {encode_key((va[int(p) // nb], vb[int(p) % nb]), dtypes): int(rng.integers(1, 60)) for p in picks}


def _state_raw(dtypes, raw, num_rows, columns=("a", "b")):
    """from_frequencies for groups given by their encoded keys."""
    t = FrequencyTable(list(columns), dict(zip(columns, dtypes)))
    t.import_groups(list(raw.values()), list(raw.keys()), num_rows)
    return FrequenciesAndNumRows(t)


@pytest.mark.parametrize("big", [0, 1], ids=["3-groups", "7000-groups"])
@pytest.mark.parametrize("form", list(FORMS))
def test_key_forms(gpu, form, big):
    dtypes, raw = _form_raw(form, big)
    assert len(raw) == (7000 if big else 3)
    columns = ("a", "a") if form == "same-column-twice" else ("a", "b")
    s = _state_raw(dtypes, raw, sum(raw.values()) + 11, columns)  # (11 rows had a NULL key)
    r, want = _check(s, raw, label=form)
    if form == "same-column-twice":
        assert r.groups_a == r.groups_b == r.groups
    if form == "float64,float32":
        a_bits = {k[:8] for k in raw}
        assert {struct.pack("<d", -0.0), struct.pack("<d", 0.0), struct.pack("<d", float("nan"))} <= a_bits
        assert r.groups_a == len(a_bits) and r.groups_b == len({k[8:] for k in raw})
    if form == "empty-string,string":
        assert r.groups_a == 1 and r.groups_b == r.groups


@pytest.mark.parametrize("case", ["field-16", "field-17", "field-16-both", "field-17-both", "joint-16", "joint-17",
                                  "joint-16-fixed", "joint-17-strings"])
def test_inline_heap_boundaries(gpu, case):
    """String fields of 16 bytes (the longest inline single-column key) and 17 (the shortest heap
    one); joint keys of 16 and 17 bytes, whatever their fields."""
    s16, s17 = "sixteen-bytes-%02d", "seventeen-byte-%02d"
    assert len(s16 % 0) == 16 and len(s17 % 0) == 17
    dtypes, fa, fb = {
        "field-16": (("string", "int8"), lambda i: s16 % i, lambda j: j),
        "field-17": (("int16", "string"), lambda i: i, lambda j: s17 % j),
        "field-16-both": (("string", "string"), lambda i: s16 % i, lambda j: s16 % (j + 50)),
        "field-17-both": (("string", "string"), lambda i: s17 % i, lambda j: s17 % (j + 50)),
        "joint-16": (("int64", "string"), lambda i: i << 33, lambda j: "c%03d" % j),      # 8 + 4 + 4
        "joint-17": (("int64", "string"), lambda i: i << 33, lambda j: "c%04d" % j),      # 8 + 4 + 5
        "joint-16-fixed": (("float64", "int64"), lambda i: i * 0.5, lambda j: -j),        # 8 + 8
        "joint-17-strings": (("string", "string"), lambda i: "abcd%d" % i, lambda j: "wxy%d" % j),  # 4 + 5 + 4 + 4
    }[case]
    rng = np.random.default_rng(5)
    joint = {(fa(i), fb(j)): int(rng.integers(1, 40)) for i in range(9) for j in range(7) if (i * 7 + j) % 5}
    raw = _raw(dtypes, joint)
    if case.startswith("joint"):
        assert {len(k) for k in raw} == {16 if "16" in case else 17}
    _check(_state(dtypes, joint, sum(joint.values()) + 3), raw, label=case)


# ---------------------------------------------------------------- contention, wide counts
@pytest.mark.parametrize("wide", [False, True], ids=["small-counts", "counts-above-2^33"])
def test_contention_and_wide_counts(gpu, wide):
    """50 000 ids x 2 categories: 100 000 joint counts go to 2 marginal groups.  With every count at
    2^33 + i no marginal sum fits 32 bits (and no workgroup's partial sum of 256 counts does)."""
    ids = np.arange(50_000, dtype=np.int64) * 1_000_003
    keys = np.empty((100_000, 2), dtype=np.int64)
    keys[:, 0] = np.repeat(ids, 2)
    keys[:, 1] = np.tile(np.array([7, -7], dtype=np.int64), 50_000)
    counts = (np.arange(100_000, dtype=np.int64) + (1 << 33)) if wide else (np.arange(100_000, dtype=np.int64) % 7 + 1)
    t = FrequencyTable(["a", "b"], {"a": "int64", "b": "int64"})
    t.import_flat(counts, np.arange(100_001, dtype=np.int64) * 16, keys.reshape(-1).view(np.uint8), int(counts.sum()) + 5)
    r, want = _check(FrequenciesAndNumRows(t), label="contention wide=%s" % wide)
    assert (r.groups, r.groups_a, r.groups_b) == (100_000, 50_000, 2)
    if wide:
        assert r.num_rows > 100_000 << 33


# ---------------------------------------------------------------- sizes
def _int_pairs_table(n, counts, num_rows=0, seed_mul=1_000_003):
    """n (int64, int64) groups (i * seed_mul, i % 1000): numpy only."""
    keys = np.empty((n, 2), dtype=np.int64)
    keys[:, 0] = np.arange(n, dtype=np.int64) * seed_mul
    keys[:, 1] = np.arange(n, dtype=np.int64) % 1000
    t = FrequencyTable(["a", "b"], {"a": "int64", "b": "int64"})
    t.import_flat(np.asarray(counts, dtype=np.int64), np.arange(n + 1, dtype=np.int64) * 16, keys.reshape(-1).view(np.uint8),
                  num_rows)
    return t


def test_table_past_its_first_slots(gpu):
    """45 000 groups: the table has left its first 2^16 slots (and the marginals have 2^17 too)."""
    rng = np.random.default_rng(3)
    counts = rng.integers(1, 30, 45_000)
    t = _int_pairs_table(45_000, counts, int(counts.sum()) + 17)
    assert t.paths()["slots"] == 1 << 17
    r, _ = _check(FrequenciesAndNumRows(t), label="45000 groups")
    assert (r.groups_a, r.groups_b) == (45_000, 1000)


def test_second_grid_stride_trip(gpu):
    """2^20 slots, 400 000 groups: twice the GRID_CAP_BLOCKS * BLOCK = 524 288 slots one trip of
    the capped grid covers.  The two largest terms sit in the first and in the last occupied slot:
    a trip that is cut short or run twice moves the sum far outside the bound."""
    n = 400_000
    t = _int_pairs_table(n, np.ones(n, dtype=np.int64), n)
    assert t.paths()["slots"] == 1 << 20 >= 2 * GRID_CAP_BLOCKS * BLOCK
    _, order = t.export()  # slot order
    first, last = order[0], order[-1]
    t.import_groups([300_000, 500_000], [first, last], 800_000 + 9)  # (the keys keep their slots)
    s = FrequenciesAndNumRows(t)
    assert t.paths()["slots"] == 1 << 20
    counts, order = t.export()
    assert (order[0], int(counts[0])) == (first, 300_001) and (order[-1], int(counts[-1])) == (last, 500_001)
    r, want = _check(s, label="two trips")
    assert r.groups == n and r.num_rows == n + 800_009
    mags = sorted(abs(x) for x in want.terms)
    bound = 8 * 2.0 ** -52 * want.sum_abs + n * 2.0 ** -96
    # the planted groups' terms: four orders above any other, twelve above the bound
    assert mags[-2] > 0.1 and mags[-2] > 1e4 * mags[-3] and mags[-2] > 1e12 * bound


# ---------------------------------------------------------------- order independence (== on the bits)
def _order_groups(n=5000):
    rng = np.random.default_rng(23)
    joint = {}
    for i in range(n):
        a = int(rng.integers(0, 300)) * 17
        b = "category-%d" % int(rng.integers(0, 40)) if i % 3 else "a-category-name-longer-than-16-%d" % int(rng.integers(0, 40))
        joint[(a, b)] = joint.get((a, b), 0) + int(rng.integers(1, 1000))
    return joint


def test_insertion_order_does_not_change_the_bits(gpu):
    joint = _order_groups()
    dtypes = ("int64", "string")
    fwd = _state(dtypes, joint, sum(joint.values()) + 1)
    rev = _state(dtypes, dict(reversed(list(joint.items()))), sum(joint.values()) + 1)
    r, _ = _check(fwd, label="forward")
    assert _bits(rev.table.mutual_information().mi) == _bits(r.mi)
    # the same state as the sum of two halves (a group's count split between them)
    items = list(joint.items())
    half1 = {k: c // 2 for k, c in items[: len(items) * 2 // 3] if c // 2}
    half2 = {k: c - half1.get(k, 0) for k, c in items}
    s1 = _state(dtypes, half1, 1)
    s2 = _state(dtypes, half2, sum(joint.values()))
    merged = s1.sum(s2)
    assert merged.frequencies(raw=True) == fwd.frequencies(raw=True) and merged.numRows == fwd.numRows
    assert _bits(merged.table.mutual_information().mi) == _bits(r.mi)


def test_row_order_does_not_change_the_bits(gpu):
    """The state computed from rows (the group-by's own insertion schedule) in two shuffles."""
    rng = np.random.default_rng(29)
    n = 30_000
    a = [None if i % 41 == 0 else int(x) for i, x in enumerate(rng.integers(0, 200, n))]
    b = [None if i % 53 == 0 else "v%d" % x for i, x in enumerate(rng.integers(0, 60, n))]
    got = []
    for seed in (1, 2):
        perm = np.random.default_rng(seed).permutation(n)
        table = d.Table.from_pydict({"a": ("int64", [a[i] for i in perm]), "b": ("string", [b[i] for i in perm])})
        s = compute_frequencies(table.to_device(0), ["a", "b"])
        assert s.numRows == n
        r, _ = _check(s, label="rows shuffle %d" % seed)
        got.append(r)
    assert _bits(got[0].mi) == _bits(got[1].mi) and got[0].groups == got[1].groups > 4096


def test_capacity_does_not_change_the_bits(gpu):
    """The same groups in a table of 2^16 slots and in one of 2^20: the larger one comes from one
    import of every key 64 times over (320 000 entries size the table, equal keys add up)."""
    n, copies = 5000, 64
    rng = np.random.default_rng(31)
    extra = rng.integers(1, 500, n)
    small = _int_pairs_table(n, extra + (copies - 1), int(extra.sum()) + n * (copies - 1) + 4)
    keys = np.empty((n, 2), dtype=np.int64)
    keys[:, 0] = np.arange(n, dtype=np.int64) * 1_000_003
    keys[:, 1] = np.arange(n, dtype=np.int64) % 1000
    counts = np.concatenate([extra, np.ones(n * (copies - 1), dtype=np.int64)])
    large = FrequencyTable(["a", "b"], {"a": "int64", "b": "int64"})
    large.import_flat(counts, np.arange(n * copies + 1, dtype=np.int64) * 16, np.tile(keys, (copies, 1)).reshape(-1).view(np.uint8),
                      int(extra.sum()) + n * (copies - 1) + 4)
    assert (small.paths()["slots"], large.paths()["slots"]) == (1 << 16, 1 << 20)
    s, l = FrequenciesAndNumRows(small), FrequenciesAndNumRows(large)
    assert s.frequencies(raw=True) == l.frequencies(raw=True)
    r, _ = _check(s, label="2^16 slots")
    assert _bits(l.table.mutual_information().mi) == _bits(r.mi)
    assert l.table.mutual_information().groups_b == 1000


# ---------------------------------------------------------------- the table is only read
def test_table_is_not_changed_and_calls_repeat(gpu):
    dtypes, raw = _form_raw("int64,40-byte-string", 1)
    s = _state_raw(dtypes, raw, sum(raw.values()) + 2)
    before = s.frequencies(raw=True)
    sm = s.table.summary()
    fields = lambda x: (x.num_rows, x.num_groups, x.num_unique, x.grouped_rows, _bits(x.entropy))  # noqa: E731
    r1 = s.table.mutual_information()
    r2 = s.table.mutual_information()
    assert (_bits(r1.mi), r1.num_rows, r1.groups, r1.groups_a, r1.groups_b) == \
        (_bits(r2.mi), r2.num_rows, r2.groups, r2.groups_a, r2.groups_b)
    assert s.frequencies(raw=True) == before and fields(s.table.summary()) == fields(sm)
    assert s.table.paths()["slots"] == 1 << 16
    s.table.import_groups([1], [next(iter(before))], 1)  # and the table still takes groups afterwards
    assert s.table.lookup(next(iter(before))) == before[next(iter(before))] + 1


# ---------------------------------------------------------------- refusals and edge cases
def test_no_groups(gpu):
    t = FrequencyTable(["a", "b"], {"a": "int64", "b": "string"})
    r = t.mutual_information()
    assert math.isnan(r.mi) and (r.num_rows, r.groups, r.groups_a, r.groups_b) == (0, 0, 0, 0)
    table = d.Table.from_pydict({"a": ("int64", [None, None, 3]), "b": ("string", ["x", None, None])})
    s = compute_frequencies(table.to_device(0), ["a", "b"])  # every row has a NULL key
    r = s.table.mutual_information()
    assert math.isnan(r.mi) and (r.num_rows, r.groups, r.groups_a, r.groups_b) == (3, 0, 0, 0)


def test_a_group_of_count_zero_is_nan(gpu):
    """0 * log(0 / ...) = 0 * -inf, or log(NaN) when its marginal is 0 too: NaN, as on the JVM."""
    for joint in ({(1, "x"): 4, (2, "x"): 0, (2, "y"): 5}, {(1, "x"): 4, (3, "z"): 0, (2, "y"): 5}):
        s = _state(("int64", "string"), joint, 9)
        r, want = _check(s, label="zero count")
        assert math.isnan(r.mi) and math.isnan(want.fsum) and r.groups == 3


def test_refused_tables(gpu):
    lib, out = L.lib(), L.DqFreqMi()
    one = FrequenciesAndNumRows.from_frequencies(["a"], ["int64"], {(1,): 2, (2,): 3}, 5)
    three = FrequenciesAndNumRows.from_frequencies(["a", "b", "c"], ["int64", "int8", "string"], {(1, 2, "x"): 2}, 2)
    hist = FrequenciesAndNumRows.from_frequencies(["a"], ["string"], {("x",): 2, (None,): 1}, 3, histogram=True)
    for s in (one, three, hist):
        assert lib.dq_freq_mutual_information(s.table.handle, ctypes.byref(out)) == L.DQ_ERR_INVALID
        with pytest.raises(L.DeequAmdError):
            s.table.mutual_information()
    two = _state(("int64", "string"), {(1, "x"): 1})
    assert lib.dq_freq_mutual_information(None, ctypes.byref(out)) == L.DQ_ERR_INVALID
    assert lib.dq_freq_mutual_information(two.table.handle, None) == L.DQ_ERR_INVALID


def test_num_rows_above_2_53(gpu):
    joint = {(1, "x"): 4, (2, "y"): 5}
    at = _state(("int64", "string"), joint, 2 ** 53)
    assert at.table.mutual_information().num_rows == 2 ** 53
    _check(at, label="numRows 2^53")
    above = _state(("int64", "string"), joint, 2 ** 53 + 2)
    with pytest.raises(L.UnsupportedOnGpu, match="2\\^53") as e:
        above.table.mutual_information()
    assert e.value.status == L.DQ_ERR_UNSUPPORTED
    with pytest.raises(L.UnsupportedOnGpu, match="more than its numRows"):  # a probability above 1
        _state(("int64", "string"), joint, 8).table.mutual_information()


# ---------------------------------------------------------------- the analyzer's route
def _rows_table(n_rows, na, nb, seed):
    rng = np.random.default_rng(seed)
    a = [None if i % 97 == 0 else int(x) * 3 for i, x in enumerate(rng.integers(0, na, n_rows))]
    b = [None if i % 89 == 0 else "name-%d" % x for i, x in enumerate(rng.integers(0, nb, n_rows))]
    joint = {}
    for x, y in zip(a, b):
        if x is not None and y is not None:
            k = (struct.pack("<q", x), y.encode())
            joint[k] = joint.get(k, 0) + 1
    return d.Table.from_pydict({"a": ("int64", a), "b": ("string", b)}).to_device(0), joint


def _host_loop(state, columns):
    """MutualInformation.computeMetricFrom's host loop as it stands (analyzers.py), restated."""
    total = state.numRows
    counts, keys = state.table.export()
    i1, i2 = state.columns.index(columns[0]), state.columns.index(columns[1])
    order = sorted(range(len(keys)), key=lambda i: keys[i])
    joint = [(decode_key(keys[i], state.table.dtypes), int(counts[i])) for i in order]
    m1, m2 = {}, {}
    for k, c in joint:
        m1[k[i1]] = m1.get(k[i1], 0) + c
        m2[k[i2]] = m2.get(k[i2], 0) + c
    value = 0.0
    for k, c in joint:
        px, py, pxy = float(m1[k[i1]]), float(m2[k[i2]]), float(c)
        value += (pxy / total) * math.log((pxy / total) / ((px / total) * (py / total)))
    return value


def test_analyzer_takes_the_device_route_above_the_bound(gpu, monkeypatch):
    from deequ_amd import analyzers
    assert analyzers.MI_HOST_MAX_GROUPS == 4096
    table, joint = _rows_table(20_000, 150, 60, 41)
    assert 5000 < len(joint) < 9000
    want = restate(joint, 20_000)

    def no_export(self, *a, **k):
        raise AssertionError("the joint table left the device")
    monkeypatch.setattr(FrequencyTable, "export", no_export)
    monkeypatch.setattr(FrequencyTable, "export_flat", no_export)
    metric = d.MutualInformation("a", "b").calculate(table)
    got = metric.value.get()
    assert abs(got - want.fsum) <= 8 * 2.0 ** -52 * want.sum_abs + len(joint) * 2.0 ** -96, (got, want.fsum)
    assert d.MutualInformation("b", "a").calculate(table).value.get() == got  # symmetric in the columns


def test_analyzer_keeps_the_host_loop_below_the_bound(gpu, monkeypatch):
    table, joint = _rows_table(3000, 20, 10, 43)
    assert len(joint) == 200
    state = compute_frequencies(table, ["a", "b"])
    want = _host_loop(state, ("a", "b"))

    def no_device(self):
        raise AssertionError("a small state took the device route")
    monkeypatch.setattr(FrequencyTable, "mutual_information", no_device)
    got = d.MutualInformation("a", "b").calculate(table).value.get()
    assert _bits(got) == _bits(want)
    assert abs(got - restate(joint, 3000).fsum) <= 1e-12
