"""tests/hostile.py proved on the CPU before any GPU test trusts it: for every dtype, flavour and
offset the GPU tests use, the column reads back as the values it was built from, and the
hostility is real -- the same buffers decoded at offset 0, or with the validity ignored, give
other content; the bytes around the window's strings are not zero; bitmap padding is set; the
string starts take every residue mod 8 for every length 0..40."""
import math

import numpy as np
import pytest

import deequ_amd as d
import hostile as H
from helpers import random_table

DTYPES = list(H.NUMERIC) + ["bool", "string"]


def _same(a, b):
    if len(a) != len(b):
        return False
    for x, y in zip(a, b):
        if isinstance(x, float) and isinstance(y, float) and math.isnan(x) and math.isnan(y):
            continue
        if x != y:
            return False
    return True


def _read(col, offset, validity=True):
    """The column's buffers decoded at `offset`, with or without its validity (strings as bytes:
    hostile spans need not be UTF-8)."""
    c = d.Column(col.dtype, col.length, col.values, col.validity if validity else None, col.offsets, offset=offset)
    if col.dtype != "string":
        return c.to_pylist()
    ok = c.valid_mask()
    raw, o = bytes(col.values), col.offsets[offset:offset + col.length + 1]
    return [raw[o[i]:o[i + 1]] if ok[i] else None for i in range(col.length)]


def _values(dtype, n, null_frac, seed=3):
    rng = np.random.default_rng(seed + n)
    return random_table(rng, n, null_frac, [dtype])["c_" + dtype][1]


@pytest.mark.parametrize("offset", H.OFFSETS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_reads_back_and_is_hostile(dtype, offset):
    for n, null_frac, flavour in ((65, 0.3, "digits"), (2049, 0.3, "high"), (64, 1.0, "text"), (1, 0.0, "text")):
        values = _values(dtype, n, null_frac)
        col = H.hostile_column(dtype, values, offset=offset, flavour=flavour)
        assert (col.length, col.offset, col.dtype) == (n, offset, dtype)
        assert col.to_pylist() == values
        for buf in (col.values, col.validity, col.offsets):
            assert buf is None or buf.ctypes.data % 64 == 0
        # rows outside the window are valid; padding bits and the bytes beyond are set
        bits = np.unpackbits(col.validity, bitorder="little")
        total = offset + n + H.TRAILING
        assert bits[:offset].all() and bits[offset + n:].all()
        assert len(bits) >= total + 64
        # the validity ignored: NULL slots hold something else than from_pylist's 0 / ""
        bare = _read(col, offset, validity=False)
        benign_bare = _read(d.Column.from_pylist(values, dtype), 0, validity=False)
        if any(v is None for v in values):
            assert not _same(bare, benign_bare)
            for v, b in zip(values, bare):
                if v is None:
                    assert b not in (0, b"", False) or isinstance(b, float)
        # decoded at offset 0: other content
        if offset and n > 1:  # (one row may equal the hostile value before it)
            assert not _same(_read(col, 0), _read(col, offset))
        if dtype == "string":
            o = col.offsets
            heap = col.values
            assert o[offset] >= H.GUARD and len(heap) - o[offset + n] >= H.GUARD
            assert heap[o[offset] - 1] != 0 and heap[o[offset + n]] != 0
            assert (np.diff(o) >= 0).all()
            assert all(o[r + 1] - o[r] >= 1 for r in range(offset)) and \
                all(o[r + 1] - o[r] >= 1 for r in range(offset + n, total))
            for i, v in enumerate(values):  # NULL slots span 1..9 bytes
                if v is None:
                    assert 1 <= o[offset + i + 1] - o[offset + i] <= 9


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_nan_and_inf_under_nulls(dtype):
    values = [None if i % 2 else float(i) for i in range(40)]
    col = H.hostile_column(dtype, values, offset=7)
    under = col.values[7:47][1::2]
    assert np.isnan(under).any() and np.isinf(under).any() and (np.abs(under[np.isfinite(under)]) > 1e38).any()
    outside = np.concatenate([col.values[:7], col.values[47:]])
    assert np.isnan(outside).any() and np.isinf(outside).any()


@pytest.mark.parametrize("dtype", ["int8", "int16", "int32", "int64"])
def test_int_extremes_under_nulls(dtype):
    values = [None if i % 2 else i for i in range(40)]
    col = H.hostile_column(dtype, values, offset=8)
    info = np.iinfo(dtype)
    under = col.values[8:48][1::2]
    assert (under == info.max).any() and (under == info.min).any()
    assert set(np.concatenate([col.values[:8], col.values[48:]]).tolist()) == {int(info.max), int(info.min), -1}


def test_device_and_host_flags():
    col = H.hostile_column("int32", [1, None, 3], offset=1)
    assert not col.device and isinstance(col.values, np.ndarray)
    with pytest.raises(ValueError):
        H.hostile_column("int32", [1], flavour="zeros")
    with pytest.raises(ValueError):
        H.hostile_column("int32", [1], trailing=3)


@pytest.mark.parametrize("offset", H.OFFSETS)
@pytest.mark.parametrize("flavour", H.FLAVOURS)
def test_string_grid_takes_every_residue(flavour, offset):
    values = H.distinct_register_strings()
    col = H.hostile_column("string", values, offset=offset, flavour=flavour)
    assert col.to_pylist() == values
    o = col.offsets[offset:offset + len(values) + 1]
    seen8, seen16 = {}, set()
    for i, v in enumerate(values):
        if v is not None:
            ln = int(o[i + 1] - o[i])
            assert ln == len(v.encode())
            seen8.setdefault(ln, set()).add(int(o[i]) % 8)
            seen16.add(int(o[i]) % 16)
    for ln in range(41):
        assert seen8[ln] == set(range(8)), ln
    assert set(range(41, 73)) <= set(seen8) and {63, 64, 65} <= set(seen8)
    assert seen16 == set(range(16))
    assert any(len(v) != len(v.encode()) for v in values if v)  # multi-byte UTF-8
    # the bytes right after a string that a NULL follows are the flavour's, never zero
    heap = col.values
    for i, v in enumerate(values[:-1]):
        if v is not None and values[i + 1] is None:
            assert heap[o[i + 1]] != 0


def test_text_flavour_extends_keys_and_booleans():
    values = ["k", None, "tru", None, "fals", None, "111-05-113", None]
    col = H.hostile_column("string", values, offset=1, flavour="text")
    raw = bytes(col.values)
    o = col.offsets[1:]
    assert raw[o[0]:o[0] + 2] == b"k1"
    assert raw[o[2]:o[2] + 4] == b"true" and raw[o[4]:o[4] + 5] == b"false"
    assert raw[o[6]:o[6] + 11] == b"111-05-1131"
    dig = H.hostile_column("string", ["12", None], offset=0, flavour="digits")
    assert bytes(dig.values)[dig.offsets[0]:dig.offsets[0] + 3] == b"129"


def test_hostile_table_mirrors_product_table():
    spec = {"a": ["int64", [1, None, 3]], "s": ["string", ["x", None, "yz"]], "b": ["bool", [True, None, False]]}
    t = H.hostile_table(spec, offset={"a": 1, "s": 7, "b": 8}, flavour="high")
    assert list(t.columns) == ["a", "s", "b"] and t.num_rows == 3
    assert [t.columns[c].offset for c in t.columns] == [1, 7, 8]
    for name, (dtype, values) in spec.items():
        assert t.columns[name].to_pylist() == values
    assert dict(t.schema) == {"a": "int64", "s": "string", "b": "bool"}
