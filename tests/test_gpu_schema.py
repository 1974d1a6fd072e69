"""RowLevelSchemaValidator on the GPU against the Python restatement (schema_cases.mirror): the counts,
both selection vectors and every output column, cell by cell.

Sizes: one wave's word (63, 64, 65), several workgroups (1000, 100003), and the scan's tile.  The
selection scans per-word popcounts (64 rows a word) and the string gather scans per-row lengths, both
with the tree's scan of 4096-element tiles: 4097 valid rows put the length scan one above a tile,
262145 rows put the word scan one above a tile (4097 words), and the square of the tile (2^24 words)
lies far beyond the 300 000 rows a test may use, so 300 000 stands in for it."""
from collections import OrderedDict

import numpy as np
import pytest

import deequ_amd as d
from deequ_amd import _lib as L

import hostile as H
import schema_cases as S

pytestmark = pytest.mark.gpu

SCAN_TILE = 4096
PATTERN = r"^[a-z]+[0-9]*$"
DEFS = [
    {"kind": "string", "name": "s", "minLength": 2, "maxLength": 12, "matches": PATTERN},
    {"kind": "int", "name": "i", "minValue": -1000, "maxValue": 100000},
    {"kind": "decimal", "name": "d", "precision": 10, "scale": 2},
]
# DEFS with another `matches`: a search that may start and end anywhere in the cell, and an alternation of
# an anchored branch with multi-byte classes (2-, 3- and 4-byte members, a Latin-1 and a CJK range)
OTHER_PATTERNS = {"unanchored": r"[a-z]{3}[0-9]", "alternation": r"^[a-m][a-z]+[0-9]*$|[é日ñ😀€本][^a-z]|[à-ÿ一-鿿]$"}
OTHER_DEFS = {k: [dict(DEFS[0], matches=p)] + DEFS[1:] for k, p in OTHER_PATTERNS.items()}


def _pools():
    rng = np.random.default_rng(77)
    letters = "abcdefghijklmnopqrstuvwxyz"
    s_pool, i_pool, d_pool = [], [], []
    for _ in range(3000):
        u = rng.random()
        if u < 0.8:
            s_pool.append("".join(letters[int(x)] for x in rng.integers(26, size=int(rng.integers(2, 10)))) +
                          "".join(str(int(x)) for x in rng.integers(10, size=int(rng.integers(0, 4)))))
        elif u < 0.9:
            s_pool.append(S.MULTIBYTE_TEXT[int(rng.integers(len(S.MULTIBYTE_TEXT)))])
        else:
            s_pool.append("".join("abXY z9_é日"[int(x)] for x in rng.integers(10, size=int(rng.integers(0, 16)))))
        u = rng.random()
        i_pool.append(str(int(rng.integers(-1000, 100001))) if u < 0.85 else
                      str(int(rng.integers(-(1 << 33), 1 << 33))) if u < 0.92 else None)
        u = rng.random()
        d_pool.append("%d.%s" % (int(rng.integers(-10 ** 7, 10 ** 7)),
                                 "".join(str(int(x)) for x in rng.integers(10, size=int(rng.integers(0, 5)))))
                      if u < 0.85 else None)
    noise = [c for c in S.random_numbers(2000, rng) + S.HOSTILE_NUMBERS
             if S.decimal_cell(c, 10, 2) != S.DECLINE]
    fill = iter(noise * 2)
    i_pool = [c if c is not None else next(fill) for c in i_pool]
    d_pool = [c if c is not None else next(fill) for c in d_pool]
    return s_pool, i_pool, d_pool


POOLS = _pools()


def random_columns(n, seed, null_rate=0.05):
    rng = np.random.default_rng(seed)
    cols = OrderedDict()
    for name, pool in zip("sid", POOLS):
        pick = rng.integers(len(pool), size=n)
        null = rng.random(n) < null_rate
        cols[name] = ("string", [None if z else pool[int(k)] for k, z in zip(pick, null)])
    null = rng.random(n) < null_rate
    cols["k"] = ("int64", [None if z else int(v) for v, z in zip(rng.integers(-(1 << 62), 1 << 62, size=n), null)])
    return cols


def make_table(cols, device):
    t = d.Table.from_pydict(cols)
    return t.to_device(0) if device else t


def compare(res, m, batch=None):
    """One batch's outputs against the restatement."""
    pick = (lambda x: x) if batch is None else (lambda x: x[batch])
    valid = res.validRows if batch is None else res.validRows.parts[batch]
    invalid = res.invalidRows if batch is None else res.invalidRows.parts[batch]
    assert pick(res.validRowIndices).tolist() == m.valid_idx
    assert pick(res.invalidRowIndices).tolist() == m.invalid_idx
    for out, want, rows in ((valid, m.valid_cols, len(m.valid_idx)), (invalid, m.invalid_cols, len(m.invalid_idx))):
        assert out.num_rows == rows and list(out.columns) == list(want)
        for name, (dtype, values) in want.items():
            col = out.columns[name]
            assert col.device and col.offset == 0 and col.dtype == dtype, name
            if dtype == "string":
                assert col.offsets is not None and col.offsets.numel() == rows + 1
            assert col.to_pylist() == values, name
    assert res.decimalColumns == m.decimals


def check(cols, defs, device=True, table=None):
    m = S.mirror(cols, defs)
    assert not m.declined
    res = d.RowLevelSchemaValidator.validate(table if table is not None else make_table(cols, device),
                                             S.build_schema(defs), withRowIndices=True)
    assert (res.numValidRows, res.numInvalidRows) == (len(m.valid_idx), len(m.invalid_idx))
    compare(res, m)
    return res, m


# ---------------------------------------------------------------- the reference's cases
@pytest.mark.parametrize("case", [c for c in S.known_answers() if not c["timestamp"]], ids=lambda c: c["id"])
def test_reference_case(gpu, case):
    cols = OrderedDict((c, ("string", [r[i] for r in case["rows"]])) for i, c in enumerate(case["columns"]))
    res, m = check(cols, case["schema"], device=False)
    assert (res.numValidRows, res.numInvalidRows) == (case["numValidRows"], case["numInvalidRows"])
    if "valid_members" in case:
        got = res.validRows.columns[case["valid_members"]["column"]].to_pylist()
        assert len(got) == case["numValidRows"] and set(got) == set(case["valid_members"]["values"])


# ---------------------------------------------------------------- random tables
@pytest.mark.parametrize("n,defs", [pytest.param(n, DEFS, id=str(n)) for n in [1, 63, 64, 65, 1000, 100003, 64 * SCAN_TILE + 1, 300000]] +
                         [pytest.param(n, OTHER_DEFS[k], id="%d-%s" % (n, k)) for k in OTHER_DEFS for n in [64, 1000, 100003]])
def test_random_table(gpu, n, defs):
    cols = random_columns(n, 1000 + n)
    res, m = check(cols, defs, device=n % 2 == 1)
    if n >= 1000:  # every verdict occurs, and a good share of each output
        assert min(len(m.valid_idx), len(m.invalid_idx)) > n // 5 and len(m.null_idx) > n // 100


def test_host_and_device_buffers_agree(gpu):
    cols = random_columns(1000, 5)
    a, _ = check(cols, DEFS, device=False)
    b, _ = check(cols, DEFS, device=True)
    for x, y in ((a.validRows, b.validRows), (a.invalidRows, b.invalidRows)):
        for name in x.columns:
            assert x.columns[name].to_pylist() == y.columns[name].to_pylist()


def test_all_valid_one_above_the_length_scans_tile(gpu):
    n = SCAN_TILE + 1
    cols = OrderedDict([("s", ("string", ["ab%d" % (r % 977) for r in range(n)])),
                        ("i", ("string", [str(r % 1000) for r in range(n)])),
                        ("d", ("string", ["%d.5" % r for r in range(n)])), ("k", ("int64", list(range(n))))])
    res, m = check(cols, DEFS)
    assert res.numValidRows == n and res.numInvalidRows == 0
    assert res.invalidRows.columns["s"].offsets.cpu().tolist() == [0]  # an empty table, one offsets entry


def test_all_invalid(gpu):
    n = 130
    cols = OrderedDict([("s", ("string", ["X"] * n)), ("i", ("string", ["1"] * n)), ("d", ("string", [None] * n)),
                        ("k", ("int64", [None] * n))])
    res, m = check(cols, DEFS)
    assert res.numValidRows == 0 and res.numInvalidRows == n
    assert res.validRows.columns["s"].offsets.cpu().tolist() == [0]
    assert res.validRows.columns["i"].dtype == "int32" and res.validRows.columns["d"].dtype == "int64"


def test_only_null_verdicts(gpu):
    n = 70
    cols = OrderedDict([("s", ("string", ["ab"] * n)), ("i", ("string", [None] * n)), ("d", ("string", ["1"] * n)),
                        ("k", ("int64", [7] * n))])
    res, m = check(cols, DEFS)
    assert res.numValidRows == 0 and res.numInvalidRows == 0 and len(m.null_idx) == n
    assert res.validRows.num_rows == 0 and res.invalidRows.num_rows == 0


def test_line_246_null_cells_under_a_min_value_vanish(gpu):
    rng = np.random.default_rng(246)
    n = 500
    vals = [None if rng.random() < 0.2 else str(int(v)) for v in rng.integers(-50, 50, n)]
    cols = OrderedDict([("i", ("string", vals)), ("s", ("string", ["x" if r % 7 else "toolong" for r in range(n)]))])
    defs = [{"kind": "int", "name": "i", "minValue": 0}, {"kind": "string", "name": "s", "maxLength": 3}]
    res, m = check(cols, defs)
    # the inputs really produce NULL verdicts: NULL cells whose row has no FALSE conjunct
    vanished = [r for r in range(n) if vals[r] is None and r % 7]
    assert vanished and m.null_idx == vanished
    assert res.numValidRows + res.numInvalidRows == n - len(m.null_idx) < n
    # with maxValue alone (colIsNull.or(...)) nothing vanishes
    res, m = check(cols, [{"kind": "int", "name": "i", "maxValue": 0}])
    assert res.numValidRows + res.numInvalidRows == n and not m.null_idx


def test_two_definitions_on_one_column(gpu):
    cols = random_columns(2000, 9)
    # both contribute to the conjunction; the last decides the cast
    defs = [{"kind": "int", "name": "i", "minValue": -1000},
            {"kind": "decimal", "name": "i", "precision": 7, "scale": 1, "isNullable": False},
            {"kind": "decimal", "name": "d", "precision": 10, "scale": 2},
            {"kind": "string", "name": "d", "maxLength": 9}]
    res, m = check(cols, defs)
    assert res.validRows.columns["i"].dtype == "int64" and res.decimalColumns == {"i": (7, 1)}
    assert res.validRows.columns["d"].dtype == "string"
    assert min(res.numValidRows, res.numInvalidRows) > 100


def test_sliced_device_columns(gpu):
    n = 2049
    cols = random_columns(n, 31)
    for flavour, offs in (("digits", {"s": 1, "i": 7, "d": 61, "k": 8}), ("high", {"s": 2051, "i": 64, "d": 24, "k": 1})):
        table = H.hostile_table(OrderedDict((c, [t, v]) for c, (t, v) in cols.items()), offset=offs, device=True,
                                flavour=flavour)
        check(cols, DEFS, table=table)
    host = H.hostile_table(OrderedDict((c, [t, v]) for c, (t, v) in cols.items()),
                           offset={"s": 7, "i": 1, "d": 8, "k": 61}, device=False, flavour="text")
    check(cols, DEFS, table=host)


def test_string_ending_at_the_heaps_end(gpu):
    import torch
    for last in ("ab", "abcdefghijkl", "abcdefghijklmnop7", "é", ""):
        vals = ["zz9", None, "toolongtoolongtoolong", last]
        data = [(v or "").encode("utf-8") for v in vals]
        offs = np.zeros(len(vals) + 1, dtype=np.int32)
        np.cumsum([len(x) for x in data], out=offs[1:])
        heap = np.frombuffer(b"".join(data), dtype=np.uint8).copy()
        assert offs[-1] == heap.size  # nothing after the last string
        col = d.Column("string", len(vals), torch.from_numpy(heap).cuda(),
                       torch.from_numpy(np.packbits(np.array([1, 0, 1, 1], dtype=bool), bitorder="little")).cuda(),
                       torch.from_numpy(offs).cuda(), device=True)
        check(OrderedDict([("s", ("string", vals))]), DEFS[:1], table=d.Table(OrderedDict([("s", col)])))


def test_partitioned_table_with_an_empty_batch(gpu):
    parts = [random_columns(300, 41), random_columns(0, 42), random_columns(1000, 43)]
    data = d.PartitionedTable([make_table(c, device=k != 2) for k, c in enumerate(parts)])
    res = d.RowLevelSchemaValidator.validate(data, S.build_schema(DEFS), withRowIndices=True)
    mirrors = [S.mirror(c, DEFS) for c in parts]
    assert isinstance(res.validRows, d.PartitionedTable) and len(res.validRows.parts) == 3
    assert len(res.invalidRows.parts) == 3
    assert res.numValidRows == sum(len(m.valid_idx) for m in mirrors)
    assert res.numInvalidRows == sum(len(m.invalid_idx) for m in mirrors)
    for k, m in enumerate(mirrors):
        compare(res, m, batch=k)
    assert res.validRows.parts[1].num_rows == 0 and res.invalidRows.parts[1].num_rows == 0


def test_one_long_row_beside_short_ones(gpu):
    long_ok = "a" * 65535 + "7"
    long_bad = "a" * 40000 + "é" + "b" * 25000
    vals = ["ab", long_ok, None, "cd9", long_bad, "X", "ef"] * 3
    cols = OrderedDict([("s", ("string", vals)), ("t", ("string", [v and v[:3] for v in vals]))])
    defs = [{"kind": "string", "name": "s", "minLength": 2, "matches": PATTERN}]
    res, m = check(cols, defs)
    assert long_ok in res.validRows.columns["s"].to_pylist() and long_bad in res.invalidRows.columns["s"].to_pylist()
    check(cols, [{"kind": "string", "name": "s", "maxLength": 65536}], device=False)


@pytest.mark.parametrize("cell", ["12é", "1e5000"])
def test_decimal_cells_the_gpu_declines(gpu, cell):
    cols = OrderedDict([("a", ("string", ["1.5", "x", None])), ("d", ("string", ["1", cell, "2.25"]))])
    defs = [{"kind": "decimal", "name": "a", "precision": 5, "scale": 1},
            {"kind": "decimal", "name": "d", "precision": 10, "scale": 2}]
    assert S.mirror(cols, defs).declined == ["d"]
    with pytest.raises(L.UnsupportedOnGpu) as e:
        d.RowLevelSchemaValidator.validate(make_table(cols, True), S.build_schema(defs))
    assert "'d'" in str(e.value) and "'a'" not in str(e.value)
    # the same cell under a string definition is no obstacle
    check(cols, defs[:1] + [{"kind": "string", "name": "d", "maxLength": 6}])
