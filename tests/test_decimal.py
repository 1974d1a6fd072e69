"""CPU tests of decimal columns: the type through every host layer, and the host build of the
decimal arithmetic the kernels run (deequ_amd/csrc/dq_decimal.h) against Python's exact rationals.

The references are independent of the code under test (tests/decimal_cases.py):
Cast(DecimalType -> DoubleType) = BigDecimal.doubleValue is `float(Fraction(u, 10 ** s))`, bit for
bit; BigInteger.toByteArray is restated from its documentation.  No GPU is touched."""
import ctypes
import decimal
import struct

import numpy as np
import pyarrow as pa
import pytest

import deequ_amd as d
from deequ_amd import _lib as L
from deequ_amd.arrow import ArrowTable, arrow_columns
from deequ_amd.engine import op_spec_for, op_supported
from deequ_amd.predicates import UnsupportedPredicate, compile_predicate

import decimal_cases as C


def _bits(x: float) -> int:
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def _to_double(u: int, s: int):
    w = u & C.MASK128
    out, tier = ctypes.c_double(), ctypes.c_int32()
    hi = (w >> 64) - (1 << 64) if (w >> 127) else (w >> 64)
    L.check(L.lib().dq_diag_decimal_to_double(w & 0xFFFFFFFFFFFFFFFF, hi, s, ctypes.byref(out), ctypes.byref(tier)))
    return out.value, tier.value


def test_decimal_to_double_is_correctly_rounded():
    """Random (p, s, u) over every precision and scale, +-(10^p - 1), 0 at every scale, the exact
    ties and their neighbours: each equal, bit for bit, to float(Fraction); every tier is taken."""
    tiers = set()
    for p, s, u in C.cast_cases():
        got, tier = _to_double(u, s)
        want = C.exact_double(u, s)
        assert _bits(got) == _bits(want), (p, s, u, got, want, tier)
        tiers.add(tier)
    assert tiers == {1, 2, 3}


def test_ties_round_to_even_as_big_decimal_double_value():
    """The values to pin against the text of BigDecimal.doubleValue: an exact tie goes to the even
    neighbour, u - 1 and u + 1 to either side of it."""
    for u, s in C.tie_values():
        lo, mid, hi = (_to_double(u + k, s)[0] for k in (-1, 0, 1))
        assert lo <= mid <= hi and lo < hi, (u, s)
        assert _bits(mid) % 2 == 0, (u, s)  # ties to even
        assert mid in (lo, hi), (u, s)
        for k in (-1, 0, 1):
            assert _bits(_to_double(-(u + k), s)[0]) == _bits(-C.exact_double(u + k, s))
    for p in (1, 9, 18, 19, 38):
        for s in (0, p):
            for u in (10 ** p - 1, -(10 ** p - 1)):
                assert _bits(_to_double(u, s)[0]) == _bits(C.exact_double(u, s))


def test_to_byte_array_helper_and_library_agree():
    assert C.to_byte_array(0) == b"\x00"
    assert C.to_byte_array(128) == b"\x00\x80"
    assert C.to_byte_array(-128) == b"\x80"
    assert C.to_byte_array(-129) == b"\xff\x7f"
    buf, n = ctypes.create_string_buffer(16), ctypes.c_int32()
    for _p, _s, u in C.cast_cases(n_random=1500) + [(38, 0, -(1 << 127)), (38, 0, (1 << 127) - 1)]:
        w = u & C.MASK128
        hi = (w >> 64) - (1 << 64) if (w >> 127) else (w >> 64)
        L.check(L.lib().dq_diag_decimal_bytes(w & 0xFFFFFFFFFFFFFFFF, hi, buf, ctypes.byref(n)))
        assert buf.raw[:n.value] == C.to_byte_array(u), u


def test_type_code_packing_and_lookup():
    assert L.TYPE_CODES["decimal(10,2)"] == 9 | 10 << 8 | 2 << 16
    assert L.TYPE_CODES["decimal(38,38)"] == 9 | 38 << 8 | 38 << 16
    assert "decimal(1,0)" in L.TYPE_CODES and "int64" in L.TYPE_CODES
    for bad in ("decimal(0,0)", "decimal(39,0)", "decimal(5,6)", "decimal(5,-1)", "decimal(5)", "decimal128(5,1)"):
        assert bad not in L.TYPE_CODES
        with pytest.raises(KeyError):
            L.TYPE_CODES[bad]
    from deequ_amd.analyzers import NUMERIC_TYPES
    from deequ_amd.table import NUMERIC
    for t in (NUMERIC_TYPES, NUMERIC):
        assert "decimal(10,2)" in t and "float64" in t and "string" not in t and "decimal(0,0)" not in t
    assert L.lib().dq_abi_version() == 4
    assert ctypes.sizeof(L.DqColumn) == 48


def _supported(kind, code, column2=-1, types=None):
    op = L.DqOp()
    op.kind, op.column, op.column2 = kind, 0, column2
    arr = (ctypes.c_int32 * 2)(*(types or [code, L.DQ_T_FLOAT64]))
    return L.lib().dq_op_supported(ctypes.byref(op), arr, 2)


def test_op_supported_answers_for_decimal_columns():
    good = L.decimal_type(10, 2)
    for kind in (L.DQ_OP_COMPLETENESS, L.DQ_OP_SUM, L.DQ_OP_MEAN, L.DQ_OP_STDDEV, L.DQ_OP_MINIMUM, L.DQ_OP_MAXIMUM,
                 L.DQ_OP_APPROX_COUNT_DISTINCT):
        assert _supported(kind, good) == L.DQ_OK
        assert _supported(kind, L.decimal_type(38, 38)) == L.DQ_OK
        assert _supported(kind, L.decimal_type(1, 0)) == L.DQ_OK
        # precision outside 1..38, scale above the precision, bits above the scale byte
        for bad in (L.decimal_type(0, 0), L.decimal_type(39, 0), L.decimal_type(5, 6), good | 1 << 24, 9):
            assert _supported(kind, bad) == L.DQ_ERR_INVALID, (kind, bad)
    # ops outside the decimal scan stay on Spark
    for kind in (L.DQ_OP_DATATYPE, L.DQ_OP_MIN_LENGTH, L.DQ_OP_MAX_LENGTH, L.DQ_OP_PATTERN_MATCH):
        assert _supported(kind, good) == L.DQ_ERR_UNSUPPORTED, kind
    assert _supported(L.DQ_OP_CORRELATION, good, 1) == L.DQ_ERR_UNSUPPORTED
    op = L.DqOp()
    op.kind, op.column, op.column2 = L.DQ_OP_CORRELATION, 0, 1
    arr = (ctypes.c_int32 * 2)(L.DQ_T_FLOAT64, good)
    assert L.lib().dq_op_supported(ctypes.byref(op), arr, 2) == L.DQ_ERR_UNSUPPORTED
    assert "decimal(10,2)" in L.lib().dq_last_error().decode()


def test_preconditions_and_op_specs():
    schema = {"m": "decimal(10,2)", "i": "int64", "s": "string"}
    for a in (d.Sum("m"), d.Mean("m"), d.Minimum("m"), d.Maximum("m"), d.StandardDeviation("m"),
              d.Correlation("m", "i"), d.ApproxQuantile("m", 0.5), d.KLLSketch("m")):
        for cond in a.preconditions():
            cond(schema)  # Preconditions.isNumeric passes for DecimalType (Analyzer.scala:336)
    with pytest.raises(d.metrics.WrongColumnTypeException):
        for cond in d.Sum("s").preconditions():
            cond(schema)
    for a in (d.Sum("m", "i > 3"), d.Completeness("m", "m IS NOT NULL"), d.ApproxCountDistinct("m"),
              d.Compliance("nn", "m IS NULL OR i = 1")):
        op_supported(op_spec_for(a, schema), schema)
    with pytest.raises(L.UnsupportedOnGpu):
        op_supported(op_spec_for(d.DataType("m"), schema), schema)


def test_predicates_take_only_null_tests_of_a_decimal_column():
    idx = {"m": (0, "decimal(10,2)"), "i": (1, "int64"), "s": (2, "string")}
    for text in ("m IS NULL", "m IS NOT NULL", "NOT (m IS NULL) AND i > 2", "m IS NULL OR s = 'x'"):
        assert len(list(compile_predicate(text, idx))) >= 2
    for text in ("m > 1", "m = 1.5", "1 < m", "m = i", "m IN (1, 2)", "COALESCE(m, 0) > 1", "m <=> NULL",
                 "CAST(m AS DOUBLE) > 1", "m = '1'", "m BETWEEN 1 AND 2", "m"):
        with pytest.raises(UnsupportedPredicate) as e:
            compile_predicate(text, idx)
        if text != "m":
            assert "decimal-typed expression" in str(e.value), text
    # the library refuses the same programs when they are hand-built (DQ_P_COLUMN of a decimal, then a comparison)
    code = (L.DqPredInsn * 3)()
    code[0].opcode, code[0].arg = L.DQ_P_COLUMN, 0
    code[1].opcode, code[1].i64 = L.DQ_P_LIT_INT, 1
    code[2].opcode, code[2].arg = L.DQ_P_GT, L.DQ_CMP_AS_INT64
    op = L.DqOp()
    op.kind, op.column = L.DQ_OP_COMPLIANCE, -1
    op.predicate.code, op.predicate.n_insns = code, 3
    types = (ctypes.c_int32 * 1)(L.decimal_type(10, 2))
    assert L.lib().dq_op_supported(ctypes.byref(op), types, 1) == L.DQ_ERR_UNSUPPORTED
    assert "decimal-typed expression" in L.lib().dq_last_error().decode()
    code[1].opcode, op.predicate.n_insns = L.DQ_P_IS_NULL, 2
    assert L.lib().dq_op_supported(ctypes.byref(op), types, 1) == L.DQ_OK


def test_column_constructors():
    D = decimal.Decimal
    c = d.Column.from_pylist([D("1.50"), -3, None, D("-0.01"), D("99999999.99")], "decimal(10,2)")
    assert c.dtype == "decimal(10,2)" and c.length == 5
    assert c.to_pylist() == [150, -300, None, -1, 9999999999]
    assert c.values.dtype == np.uint64 and c.values.shape == (5, 2)
    assert c.to_dq().type == L.decimal_type(10, 2)
    for bad in (D("1.505"), D("100000000.00"), 10 ** 8, D("NaN"), 1.5, "1.5", True):
        with pytest.raises(ValueError):
            d.Column.from_pylist([bad], "decimal(10,2)")
    big = -(10 ** 38 - 1)
    nines = "0." + "9" * 38
    assert d.Column.from_pylist([D("-" + nines), D(nines)], "decimal(38,38)").to_pylist() == [big, -big]
    assert d.Column.from_pylist([big, -big], "decimal(38,0)").to_pylist() == [big, -big]
    words = C.le_words([5, -5, None])
    n = d.Column.from_numpy(words, np.array([True, True, False]), "decimal(9,0)")
    assert n.to_pylist() == [5, -5, None]
    with pytest.raises(ValueError):
        d.Column.from_numpy(np.zeros(4, dtype=np.uint64), None, "decimal(9,0)")
    with pytest.raises(ValueError):
        d.Column("decimal(39,0)", 0, words)
    t = d.Table({"m": c})
    assert t.schema == {"m": "decimal(10,2)"}


def test_arrow_decimal128_columns():
    D = decimal.Decimal
    vals = [D("1.50"), None, D("-7.25"), D("9.00"), None, D("-99999999.99")]
    arr = pa.array(vals, pa.decimal128(10, 2))
    col = d.Column.from_arrow(arr)
    assert col.dtype == "decimal(10,2)" and col.to_pylist() == [150, None, -725, 900, None, -9999999999]
    assert col.values.ctypes.data == arr.buffers()[1].address  # zero-copy
    sl = d.Column.from_arrow(arr.slice(2))
    assert sl.offset == 2 and sl.to_pylist() == [-725, 900, None, -9999999999]
    # a sliced column travels to the library as a dq_column: its offset counts 16-byte slots
    dq = sl.to_dq()
    assert dq.type == L.decimal_type(10, 2) and dq.offset == 2 and dq.length == 4
    assert dq.values == arr.buffers()[1].address and dq.validity == arr.buffers()[0].address
    t = d.Table.from_arrow(pa.table({"m": arr, "i": pa.array(range(6), pa.int64())}))
    assert t.schema == {"m": "decimal(10,2)", "i": "int64"}
    nonull = d.Column.from_arrow(pa.array([D("1"), D("2")], pa.decimal128(38, 0)))
    assert nonull.dtype == "decimal(38,0)" and nonull.validity is None and nonull.to_pylist() == [1, 2]
    # the Arrow C Data Interface entry points keep declining every decimal format, naming it
    # (tests/test_arrow_abi.py pins the refusal of decimal128): decimal128, other
    # widths, a negative scale
    for t, fmt in ((pa.decimal128(10, 2), "d:10,2"), (pa.decimal256(40, 2), "d:40,2,256"),
                   (pa.decimal128(10, -2), "d:10,-2")):
        bad = pa.record_batch([pa.array([None], t)], names=["m"])
        with pytest.raises(L.UnsupportedOnGpu) as e:
            arrow_columns(bad)
        assert fmt in str(e.value)
        with pytest.raises(L.UnsupportedOnGpu):
            ArrowTable(bad).schema
    for name in ("decimal32", "decimal64"):
        if hasattr(pa, name):
            bad = pa.record_batch([pa.array([None], getattr(pa, name)(5, 2))], names=["m"])
            with pytest.raises(L.UnsupportedOnGpu) as e:
                arrow_columns(bad)
            assert "d:5,2," in str(e.value)
    for t in (pa.decimal256(40, 2), pa.decimal128(10, -2)):
        with pytest.raises(L.UnsupportedOnGpu) as e:
            d.Column.from_arrow(pa.array([None], t))
        assert str(t) in str(e.value)
        with pytest.raises(L.UnsupportedOnGpu) as e:
            d.Table.from_arrow(pa.table({"i": pa.array([1]), "amount": pa.array([None], t)}))
        assert "column amount" in str(e.value) and str(t) in str(e.value)
    with pytest.raises(TypeError):  # (other off-path types keep their TypeError)
        d.Column.from_arrow(pa.array([1], pa.uint64()))


def test_excluded_uses_raise_unsupported_naming_the_column():
    """decimal keys of the frequency family and Histogram, decimal columns in
    RowLevelSchemaValidator input, date / timestamp columns -- refused, never answered wrongly."""
    from deequ_amd.frequencies import FrequencyTable
    from deequ_amd.schema import RowLevelSchema, check_schema
    schema = {"m": "decimal(10,2)", "s": "string"}
    for histogram in (False, True):
        with pytest.raises(L.UnsupportedOnGpu) as e:
            FrequencyTable(["m"], schema, histogram=histogram)
        assert "column m" in str(e.value) and "decimal(10,2)" in str(e.value)
    with pytest.raises(L.UnsupportedOnGpu) as e:
        check_schema(RowLevelSchema().withStringColumn("s"), schema)
    assert "column m" in str(e.value)
    # ... and the library itself declines it at plan time, whoever calls it
    defs = (L.DqSchemaDef * 1)()
    defs[0].kind, defs[0].column = L.DQ_SCHEMA_STRING, 1
    types = (ctypes.c_int32 * 2)(L.decimal_type(10, 2), L.DQ_T_UTF8)
    assert L.lib().dq_schema_supported(defs, 1, types, 2) == L.DQ_ERR_UNSUPPORTED
    assert "decimal(10,2)" in L.lib().dq_last_error().decode()
    types[0] = L.DQ_T_INT64
    assert L.lib().dq_schema_supported(defs, 1, types, 2) == L.DQ_OK
    import datetime
    for arr in (pa.array([datetime.date(2020, 1, 1)]), pa.array([datetime.datetime(2020, 1, 1)])):
        with pytest.raises(L.UnsupportedOnGpu) as e:
            ArrowTable(pa.table({"when": arr})).schema
        assert "date" in str(e.value) or "timestamp" in str(e.value)
    from deequ_amd.kll import check_column
    with pytest.raises(ValueError) as e:
        check_column(schema, "m")
    assert str(e.value) == "Cannot handle DecimalType(10,2)"
