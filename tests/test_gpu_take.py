"""take on the GPU (deequ_amd/take.py; dq_take_map_kernel, dq_take_fixed_kernel, dq_take_bits_kernel,
dq_take_len_kernel, dq_take_bytes_kernel, dq_take_pieces_kernel) against the numpy restatement of
take_cases.py, buffer for buffer: values, validity words, offsets, and the heap up to the last
offset.  The shapes come from the kernels' exported tiling constants (dq_diag_take_constants)."""
import ctypes
from collections import OrderedDict

import numpy as np
import pytest

import deequ_amd as d
import take_cases as T
from deequ_amd import _lib as L
from hostile import hostile_column

pytestmark = pytest.mark.gpu

C = L.diag_take_constants()
R, TILE, WAVE, SPLIT = C["rows_per_block"], C["scan_tile"], C["wave_bytes"], C["split_bytes"]
SIZES = sorted({0, 1, 63, 64, 65, R - 1, R, R + 1, TILE - 1, TILE, TILE + 1, 2 * TILE + 1})
BIG = 100_003


# ---------------------------------------------------------------- helpers
def _dataset(parts, device):
    if device:
        parts = [p.to_device(0) for p in parts]
    return parts[0] if len(parts) == 1 else d.PartitionedTable(parts)


def _bytes(buf):
    a = buf.cpu().numpy() if hasattr(buf, "cpu") else np.asarray(buf)
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


def _assert_column(col, want, device, what):
    assert col.dtype == want.dtype and col.length == want.m and col.offset == 0 and col.device == device, what
    if want.validity is None:
        assert col.validity is None, what
    else:
        assert _bytes(col.validity).tobytes() == want.validity.tobytes(), what
    if want.offsets is None:
        assert col.offsets is None, what
        assert _bytes(col.values).tobytes() == want.values.tobytes(), what
    else:
        offs = _bytes(col.offsets).view(np.int32)
        assert offs.tolist() == want.offsets.tolist(), what
        assert _bytes(col.values)[:int(offs[-1])].tobytes() == want.values.tobytes(), what


def _check(parts, rows, devices=(True,), columns=None, what=""):
    """d.take over the host Tables `parts` (one per batch), uploaded or not, against the restatement."""
    want = T.restate_table(parts, rows, columns)
    for device in devices:
        got = d.take(_dataset(parts, device), rows, columns)
        assert list(got.columns) == list(want) and got.num_rows == len(rows)
        for name, w in want.items():
            _assert_column(got.columns[name], w, device, (what, name, device))


def _single(col, name="c"):
    return d.Table(OrderedDict([(name, col)]))


# ---------------------------------------------------------------- sizes, index shapes, chunking
@pytest.mark.parametrize("size", SIZES)
def test_every_dtype_at_the_kernels_sizes(gpu, size):
    """n = m = size (a permutation with -1 rows mixed in), and m = size indices into 1000 rows."""
    lengths = T.chunkings(size).get("three", [size])
    parts = T.random_parts(lengths, seed=size)
    rng = np.random.default_rng(size + 1)
    rows = rng.permutation(size).astype(np.int64)
    rows[rng.random(size) < 0.1] = -1
    _check(parts, rows, what="n = m")
    small = T.random_parts([1, 64, 935], seed=size + 2)
    _check(small, rng.integers(-1, 1000, size), what="m alone")
    if size == 0:
        _check(parts, np.full(5, -1, dtype=np.int64), what="all -1 over no rows")


def test_the_larger_size(gpu):
    parts = T.random_parts([1, 64, BIG - 65], seed=11)
    rng = np.random.default_rng(12)
    rows = rng.permutation(BIG).astype(np.int64)
    rows[::17] = -1
    _check(parts, rows)


@pytest.mark.parametrize("chunking", ["one", "three", "empty_middle"])
def test_index_shapes_and_chunk_edges(gpu, chunking):
    n = 2 * TILE + 1
    lengths = T.chunkings(n)[chunking]
    parts = T.random_parts(lengths, seed=21)
    shapes = T.index_shapes(n, R + 1, seed=22)
    shapes["edges"] = T.chunk_edges(lengths)
    shapes["permutation_of_all"] = np.random.default_rng(23).permutation(n).astype(np.int64)
    for name, rows in shapes.items():
        _check(parts, rows, what=name)


def test_rows_as_list_numpy_host_and_device_tensors(gpu):
    import torch
    parts = T.random_parts([70], seed=31, dtypes=("int64", "string"))
    rows = [3, -1, 69, 0, 3]
    want = T.restate_table(parts, rows)
    data = _dataset(parts, True)
    for r in (rows, np.array(rows), torch.tensor(rows), torch.tensor(rows, device="cuda:0")):
        got = d.take(data, r, columns=["c_string"])
        assert list(got.columns) == ["c_string"]
        _assert_column(got.columns["c_string"], want["c_string"], True, type(r))
    with pytest.raises(ValueError):
        d.take(data, torch.tensor(rows, dtype=torch.int32))


# ---------------------------------------------------------------- dtypes and slices
def test_float_bits_decimal_signs_and_columns_without_validity(gpu):
    rows = np.array([7, 0, 3, -1, 4, 1, 2, 5, 6, 3], dtype=np.int64)
    for dtype, vals in T.SPECIAL_FLOATS.items():
        _check([_single(d.Column.from_numpy(vals, None, dtype))], rows, what=dtype)
        _check([_single(d.Column.from_numpy(vals, None, dtype))], rows[rows >= 0], what=dtype + " no validity out")
    words = np.array([[1, 1 << 63], [0xFFFFFFFFFFFFFFFF] * 2, [5, 0], [0, 1 << 63]] * 40, dtype=np.uint64)
    valid = np.arange(160) % 5 != 0
    for offset in (0, 1, 5):
        col = T.sliced_decimal(words, valid, offset)
        _check([_single(col)], np.random.default_rng(offset).integers(-1, 160, 300), what="decimal slice %d" % offset)
    parts = T.random_parts([100, 30], seed=41, nulls=False)
    got = d.take(_dataset(parts, True), [5, 129, 100])
    assert all(c.validity is None for c in got.columns.values())
    _check(parts, np.array([5, 129, 100, 99, 0]), what="no validity")


@pytest.mark.parametrize("offset", [1, 7, 61])
def test_hostile_slices_at_bit_offsets(gpu, offset):
    rng = np.random.default_rng(offset)
    n = 2 * R + 7
    cut = R + 1
    for dtype in T.FIXED + ("bool", "string"):
        if dtype == "string":
            vals = [None if rng.random() < 0.2 else "s%d" % i * int(rng.integers(0, 4)) for i in range(n)]
        elif dtype == "bool":
            vals = [None if rng.random() < 0.2 else bool(rng.random() < 0.5) for _ in range(n)]
        elif dtype.startswith("float"):
            vals = [None if rng.random() < 0.2 else float(np.float32(rng.normal())) for _ in range(n)]
        else:
            vals = [None if rng.random() < 0.2 else int(rng.integers(-100, 100)) for _ in range(n)]
        parts = [_single(hostile_column(dtype, vals[:cut], offset=offset)),
                 _single(hostile_column(dtype, vals[cut:], offset=offset + 3, flavour="high"))]
        _check(parts, rng.integers(-1, n, 3 * R), what=dtype)
        _check(parts, np.arange(n), what=dtype + " identity")


# ---------------------------------------------------------------- utf8
def test_utf8_lengths_at_every_source_and_destination_alignment(gpu):
    col, rows = T.alignment_grid(T.SMALL_LENGTHS + tuple(T.threshold_lengths(C)))
    _check([_single(col)], rows)


def test_one_long_cell_among_many_short_ones(gpu):
    cells = [b"x"] * 10_000
    cells[4321] = T.cell_bytes(4 * SPLIT, 9)
    col = T.string_column(cells)
    _check([_single(col)], np.arange(10_000))
    _check([_single(col)], np.array([4321, 0, 4321, -1, 4321, 1, 2]), what="the long cell at other residues")


def test_multibyte_strings_and_null_cells_with_source_bytes(gpu):
    mb = T.multibyte_column()
    for rows in (np.arange(mb.length), np.arange(mb.length - 1, -1, -1), np.array([0, 0, -1, 2, 1])):
        want = T.restate([mb], rows)
        _check([_single(mb)], rows)
        for s in want.column().to_pylist():
            assert s is None or s.encode("utf-8").decode("utf-8") == s


# ---------------------------------------------------------------- refusals
def _status(fn, *args, **kw):
    with pytest.raises(L.DeequAmdError) as e:
        fn(*args, **kw)
    return e.value.status, str(e.value)


@pytest.mark.parametrize("bad", [10, 11, -2, np.iinfo(np.int64).min])
def test_an_index_out_of_range_is_refused(gpu, bad):
    data = _dataset(T.random_parts([10], seed=51), True)
    rows = np.array([0, 9, -1, bad, 12, -5], dtype=np.int64)
    status, msg = _status(d.take, data, rows)
    assert status == L.DQ_ERR_INVALID and "rows[3] = %d" % bad in msg, msg


def test_more_than_4096_chunks_are_declined(gpu):
    empty = {"a": ("int64", [])}
    parts = [d.Table.from_pydict({"a": ("int64", list(range(10)))})] + [d.Table.from_pydict(empty) for _ in range(4096)]
    status, msg = _status(d.take, d.PartitionedTable(parts), [0])
    assert status == L.DQ_ERR_UNSUPPORTED and "4097 chunks" in msg, msg
    got = d.take(d.PartitionedTable(parts[:4096]), [9, 0])
    assert got.columns["a"].to_pylist() == [9, 0]


def test_a_host_resident_chunk_is_refused(gpu):
    import torch
    table = d.Table.from_pydict({"a": ("int64", list(range(10)))})
    rows = torch.tensor([1, 2], device="cuda:0")
    lens = (ctypes.c_int64 * 1)(10)
    h = ctypes.c_void_p()
    lib = L.lib()
    L.check(lib.dq_take_create(L.Context.get(0).handle, rows.data_ptr(), 2, lens, 1, ctypes.byref(h)))
    try:
        cols = (L.DqColumn * 1)(table.columns["a"].to_dq())
        t, vb, nb, ob = ctypes.c_int32(), ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        st = lib.dq_take_layout(h, cols, ctypes.byref(t), ctypes.byref(vb), ctypes.byref(nb), ctypes.byref(ob))
        assert st == L.DQ_ERR_INVALID and b"chunk 0 is host-resident" in lib.dq_last_error()
        st = lib.dq_take_gather(h, cols, None, None, None)
        assert st == L.DQ_ERR_STATE
        n = ctypes.c_int64(-1)
        L.check(lib.dq_take_info(h, ctypes.byref(n)))
        assert n.value == 0
    finally:
        lib.dq_take_destroy(h)


def test_a_utf8_output_above_int32_is_refused_before_any_copy(gpu):
    import torch
    cell = 1 << 20
    col = T.string_column([b"ab", b"y" * cell])
    data = _single(col).to_device(0)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    status, msg = _status(d.take, data, np.full(2049, 1, dtype=np.int64))
    assert status == L.DQ_ERR_SPACE and str(2049 * cell) in msg, msg
    assert torch.cuda.max_memory_allocated() - before < (64 << 20)  # (no 2 GiB heap was allocated)
    _check([_single(col)], np.array([1, 0, 1]), what="the same cell, taken three times")


# ---------------------------------------------------------------- end to end
def _products(n):
    rng = np.random.default_rng(61)
    return OrderedDict([
        ("id", ("int64", list(range(n)))),
        ("name", ("string", [None if i % 7 == 3 else "item-%d" % i * (1 + i % 3) for i in range(n)])),
        ("q", ("int64", [None if i % 11 == 5 else int(rng.integers(-3, 9)) for i in range(n)])),
        ("price", ("float64", [None if i % 13 == 2 else float(rng.integers(1, 100)) for i in range(n)])),
        ("ok", ("bool", [None if i % 5 == 1 else bool(i % 2) for i in range(n)])),
    ])


def _parts_of(spec, cuts):
    return [d.Table.from_pydict({c: (t, v[a:b]) for c, (t, v) in spec.items()}) for a, b in zip(cuts, cuts[1:])]


def _pick(spec, rows, columns=None):
    names = list(spec) if columns is None else columns
    return {c: [None if r < 0 else spec[c][1][r] for r in rows] for c in names}


def _pylists(table):
    return {c: col.to_pylist() for c, col in table.columns.items()}


@pytest.mark.parametrize("device", [False, True])
def test_row_level_results_take_and_split(gpu, device):
    n = 3 * R + 5
    spec = _products(n)
    data = _dataset(_parts_of(spec, [0, R - 1, R + 70, n]), device)
    analyzers = [d.Completeness("name"), d.Compliance("positive", "q > 0"),
                 d.Compliance("cheap", "price < 50", where="q > 0")]
    res = d.row_level_results(data, analyzers)
    outcomes = {a: res.to_pylist(a) for a in analyzers}
    for a in analyzers:
        for which, flag in (("false", False), ("true", True), ("null", None)):
            rows = [i for i, o in enumerate(outcomes[a]) if o is flag]
            got = res.take(data, a, which)
            assert all(c.device == device for c in got.columns.values())
            assert _pylists(got) == _pick(spec, rows), (a, which)
    got = res.take(data, analyzers[0], columns=["id", "q"])
    assert _pylists(got) == _pick(spec, [i for i, o in enumerate(outcomes[analyzers[0]]) if o is False], ["id", "q"])
    for subset in (None, analyzers[:1], analyzers[1:]):
        used = analyzers if subset is None else subset
        bad = [i for i in range(n) if any(outcomes[a][i] is False for a in used)]
        good = [i for i in range(n) if i not in set(bad)]
        passing, failing = res.split(data, subset)
        assert passing.num_rows + failing.num_rows == res.num_rows == n
        assert _pylists(failing) == _pick(spec, bad) and _pylists(passing) == _pick(spec, good)
    assert any(o is None for o in outcomes[analyzers[2]]) and len(bad) and len(good)


@pytest.mark.parametrize("device", [False, True])
def test_dataset_match_mismatches(gpu, device):
    orders = OrderedDict([
        ("customer", ("string", ["c1", "c2", None, "c9", "c3", "c2", "c8", None, "c4"])),
        ("city", ("string", ["Oslo", "Rome", "Bern", "Kyiv", "Lima", "Rome", "Riga", "Graz", None])),
        ("tier", ("int64", [1, 2, 3, 4, None, 7, 1, 2, 3])),
    ])
    customers = OrderedDict([
        ("id", ("string", ["c4", "c3", "c2", "c1", "c5", None])),
        ("city", ("string", ["Baku", "Lima", "Rome", "Oslo", "Pisa", "Graz"])),
        ("tier", ("int64", [3, 5, 2, 1, 1, 2])),
    ])
    a = _dataset(_parts_of(orders, [0, 4, 9]), device)
    b = _dataset(_parts_of(customers, [0, 6]), device)
    res = d.dataset_match(a, b, [("customer", "id")], ["city", "tier"], reference_rows=True)
    failing, refs = res.failing_rows().tolist(), res.reference_rows().tolist()
    assert failing == [2, 3, 4, 5, 6, 7, 8] and refs == [3, 2, -1, -1, 1, 2, -1, -1, 0]
    a_rows, b_rows = res.mismatches(a, b)
    assert a_rows.num_rows == b_rows.num_rows == len(failing)
    assert all(c.device == device for t in (a_rows, b_rows) for c in t.columns.values())
    assert _pylists(a_rows) == _pick(orders, failing)
    assert _pylists(b_rows) == _pick(customers, [refs[i] for i in failing])
    for i, r in enumerate(failing):  # all-NULL exactly where there is no reference row
        assert all(v[i] is None for v in _pylists(b_rows).values()) == (refs[r] == -1)
    a_rows, b_rows = res.mismatches(a, b, columns=["tier"], reference_columns=["tier", "id"])
    assert _pylists(a_rows) == _pick(orders, failing, ["tier"])
    assert _pylists(b_rows) == _pick(customers, [refs[i] for i in failing], ["tier", "id"])
    assert _pylists(res.take(a, "true")) == _pick(orders, [0, 1])
    plain = d.dataset_match(a, b, [("customer", "id")], ["city", "tier"])
    with pytest.raises(KeyError, match="reference_rows=True"):
        plain.mismatches(a, b)
