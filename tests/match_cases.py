"""Boundary cells of every dtype the cross-table checks compare, shared by test_match.py (the host
build of the cell equality against the restatement) and test_gpu_match.py (the same cells as
compare columns on the device).  `cells(dtype)` returns Python values (None = NULL) whose pairwise
equalities cover: NaNs of different payloads, +-0.0 and +-Inf; integer and decimal128 extremes;
strings that are empty, multi-byte, equal up to the last byte, and of lengths 0, 1, 7, 8, 9, 15, 16,
17 and 64; NULL on either side and on both (every list holds a None, and every pair is formed)."""
import struct

import numpy as np

STRING_LENGTHS = (0, 1, 7, 8, 9, 15, 16, 17, 64)
DTYPES = ("bool", "int8", "int16", "int32", "int64", "float32", "float64", "string", "decimal(38,0)",
          "decimal(10,2)")


def _f64(bits: int) -> float:
    return struct.unpack("<d", struct.pack("<Q", bits))[0]


def _strings():
    out = [None]
    for n in STRING_LENGTHS:
        base = "".join(chr(ord("a") + (i % 26)) for i in range(n))
        out.append(base)
        if n:
            out.append(base[:-1] + "#")      # equal up to the last byte
            out.append("#" + base[1:])       # differs in the first byte
    out += ["é", "é", "日本語", "日本誟", "aé" * 4]  # multi-byte
    return out


def cells(dtype: str):
    if dtype == "bool":
        return [True, False, None]
    if dtype in ("int8", "int16", "int32", "int64"):
        info = np.iinfo(dtype)
        return [int(info.min), int(info.min) + 1, -1, 0, 1, int(info.max) - 1, int(info.max), None]
    if dtype == "float64":
        return [0.0, -0.0, 1.0, -1.0, float("inf"), float("-inf"), 5e-324, -5e-324, 1.7976931348623157e308,
                _f64(0x7FF8000000000000), _f64(0x7FF8000000000001), _f64(0xFFF8000000000000),
                _f64(0x7FF0000000000001), None]
    if dtype == "float32":  # (every value is exactly a float32; NaN payloads are set by bits below)
        return [0.0, -0.0, 1.0, -1.0, float("inf"), float("-inf"), float(np.float32(1e-45)), float(np.float32(3.4028235e38)),
                float("nan"), float("nan"), float("nan"), float("nan"), None]
    if dtype == "string":
        return _strings()
    if dtype == "decimal(38,0)":
        top = 10 ** 38 - 1
        return [0, 1, -1, top, -top, top - 1, 2 ** 64, 2 ** 64 + 1, -(2 ** 64), 2 ** 63, None]
    if dtype == "decimal(10,2)":
        import decimal
        return [decimal.Decimal("0.00"), decimal.Decimal("0.01"), decimal.Decimal("-0.01"),
                decimal.Decimal("99999999.99"), decimal.Decimal("-99999999.99"), None]
    raise KeyError(dtype)


# float32 NaNs of different payloads, as bit patterns written over the NaN slots of a built column
FLOAT32_NAN_BITS = (0x7FC00000, 0x7FC00001, 0xFFC00000, 0x7F800001)


def column(dtype: str, values):
    """A host deequ_amd Column of `values`; a float32 column's NaNs get FLOAT32_NAN_BITS in turn."""
    from deequ_amd import Column
    col = Column.from_pylist(list(values), dtype)
    if dtype == "float32":
        bits = col.values.view(np.uint32).copy()
        k = 0
        for i, v in enumerate(values):
            if v is not None and v != v:
                bits[i] = FLOAT32_NAN_BITS[k % len(FLOAT32_NAN_BITS)]
                k += 1
        col.values = bits.view(np.float32)
    return col
