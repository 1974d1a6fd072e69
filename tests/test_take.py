"""take without a device: the numpy restatement of take_cases.py against pyarrow's take (the
independent reference: pa.chunked_array(...).take with -1 as a null index) on every case the GPU
tests use, the argument checks that need no GPU, and the exported tiling constants."""
import numpy as np
import pytest

import deequ_amd as d
import take_cases as T
from deequ_amd import _lib as L
from deequ_amd.comparison import MatchCounts, MatchResult
from deequ_amd.distributed import ShardedTable
from deequ_amd.rowlevel import RowLevelResults
from hostile import hostile_column


def _agree(chunks, rows):
    got = T.restate(chunks, rows)
    col = got.column()
    assert col.length == len(rows)
    assert T.same_values(T.logical(col), T.arrow_take(chunks, rows)), chunks[0].dtype
    return got


def test_constants_are_readable():
    c = L.diag_take_constants()
    assert c["rows_per_block"] >= 64 and c["rows_per_block"] % 64 == 0
    assert c["scan_tile"] >= c["rows_per_block"]
    assert 16 <= c["wave_bytes"] < c["split_bytes"] <= 1 << 20


@pytest.mark.parametrize("chunking", ["one", "three", "empty_middle"])
def test_restatement_equals_pyarrow_on_every_dtype_and_shape(chunking):
    n = 1000
    lengths = T.chunkings(n)[chunking]
    parts = T.random_parts(lengths, seed=3)
    shapes = T.index_shapes(n, 333, seed=4)
    shapes["edges"] = T.chunk_edges(lengths)
    for name, rows in shapes.items():
        for col in parts[0].columns:
            _agree([p.columns[col] for p in parts], rows)


def test_restatement_on_empty_inputs():
    parts = T.random_parts([0], seed=1)
    for col in parts[0].columns:
        chunks = [parts[0].columns[col]]
        assert _agree(chunks, np.zeros(0, np.int64)).m == 0
        got = _agree(chunks, np.full(5, -1, np.int64))
        assert got.validity is not None and int(got.validity[0]) == 0


def test_restatement_keeps_float_bits_and_decimal_signs():
    for dtype, vals in T.SPECIAL_FLOATS.items():
        col = d.Column.from_numpy(vals, None, dtype)
        rows = np.array([7, 0, 3, 4, 1, 2, 5, 6, 3], dtype=np.int64)
        got = _agree([col], rows)
        assert got.validity is None  # (no validity buffer, no -1)
        assert got.values.tobytes() == vals[rows].tobytes()
    words = np.array([[1, 1 << 63], [0xFFFFFFFFFFFFFFFF, 0xFFFFFFFFFFFFFFFF], [5, 0]], dtype=np.uint64)
    col = T.sliced_decimal(words, np.array([True, True, False]), offset=5)
    got = _agree([col], np.array([2, 1, -1, 0], dtype=np.int64))
    assert got.values.view(np.uint64).reshape(-1, 2).tolist() == [[5, 0], [0xFFFFFFFFFFFFFFFF] * 2, [0, 0], [1, 1 << 63]]


@pytest.mark.parametrize("offset", [1, 7, 61])
def test_restatement_on_hostile_slices(offset):
    rng = np.random.default_rng(offset)
    n = 130
    for dtype in T.FIXED + ("bool", "string"):
        if dtype == "string":
            vals = [None if rng.random() < 0.2 else "s%d" % i * int(rng.integers(0, 4)) for i in range(n)]
        elif dtype == "bool":
            vals = [None if rng.random() < 0.2 else bool(rng.random() < 0.5) for _ in range(n)]
        elif dtype.startswith("float"):
            vals = [None if rng.random() < 0.2 else float(np.float32(rng.normal())) for _ in range(n)]
        else:
            vals = [None if rng.random() < 0.2 else int(rng.integers(-100, 100)) for _ in range(n)]
        chunks = [hostile_column(dtype, vals[:65], offset=offset), hostile_column(dtype, vals[65:], offset=offset + 3)]
        rows = rng.integers(-1, n, 200)
        got = _agree(chunks, rows)
        want = [None if r < 0 else vals[r] for r in rows.tolist()]
        assert T.same_values(got.column().to_pylist(), want)


def test_restatement_on_the_utf8_grids():
    c = L.diag_take_constants()
    col, rows = T.alignment_grid(T.SMALL_LENGTHS + (c["wave_bytes"] - 1, c["wave_bytes"], c["wave_bytes"] + 1))
    got = _agree([col], rows)
    offs = col.offsets
    assert {int(offs[r]) % 16 for r in rows[1::2]} == set(range(16))       # every source residue
    assert {int(o) % 16 for o in got.offsets[1:-1:2]} == set(range(16))    # every destination residue
    mb = T.multibyte_column()
    rows = np.arange(mb.length - 1, -1, -1)
    got = _agree([mb], rows)
    for s in got.column().to_pylist():
        assert s is None or s.encode("utf-8").decode("utf-8") == s
    offs = mb.offsets[mb.offset:mb.offset + mb.length + 1]
    null_rows = np.nonzero(~mb.valid_mask())[0]
    assert len(null_rows) and all(offs[r + 1] > offs[r] for r in null_rows)  # NULL cells with source bytes


def test_restatement_refuses_out_of_range():
    parts = T.random_parts([10], seed=2, dtypes=("int64",))
    for bad in (10, 11, -2, np.iinfo(np.int64).min):
        with pytest.raises(ValueError, match=r"rows\[3\]"):
            T.restate([parts[0].columns["c_int64"]], [0, 9, -1, bad, 12])


# ---------------------------------------------------------------- argument checks (no device)
def _table(n=4):
    return d.Table.from_pydict({"a": ("int64", list(range(n))), "s": ("string", ["x"] * n)})


def test_unknown_column_is_a_value_error():
    with pytest.raises(ValueError, match="no column 'nope'"):
        d.take(_table(), [0], columns=["a", "nope"])


def test_sharded_table_is_declined():
    with pytest.raises(L.UnsupportedOnGpu, match="ShardedTable"):
        d.take(ShardedTable(_table()), [0])


def test_row_count_mismatch_is_a_value_error():
    a = d.Completeness("a")
    res = RowLevelResults(5, 0, False, {a: (None, None)})
    with pytest.raises(ValueError, match="5 rows, the table has 4"):
        res.take(_table(4), a)
    with pytest.raises(ValueError, match="5 rows, the table has 4"):
        res.split(_table(4))
    with pytest.raises(KeyError):
        res.take(_table(5), d.Completeness("s"))
    m = MatchResult(res, MatchCounts(0, 0, 0, 0, 0))
    with pytest.raises(KeyError, match="reference_rows=True"):
        m.mismatches(_table(5), _table(5))
