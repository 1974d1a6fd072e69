"""RowLevelSchemaValidator (schema/RowLevelSchemaValidator.scala) without a GPU: the builders, every
plan-time decline and ValueError, the Python restatement (schema_cases.mirror) against the
reference's known answers, and the host build of the int and decimal cell tests
(dq_diag_schema_cell: the source the evaluate kernel runs) against the restatement on hostile and
generated cells.  GPU runs: test_gpu_schema.py."""
import ctypes
from collections import OrderedDict

import numpy as np
import pytest

import deequ_amd as d
from deequ_amd import _lib as L
from deequ_amd.distributed import ShardedTable
from deequ_amd.schema import (DecimalColumnDefinition, IntColumnDefinition, StringColumnDefinition,
                              TimestampColumnDefinition, check_schema)

import pattern_cases as P
import schema_cases as S


def schema_cell(kind, text, precision=0, scale=0):
    """(result, value) of dq_diag_schema_cell."""
    b = text.encode("utf-8")
    res, val = ctypes.c_int32(-1), ctypes.c_int64(-1)
    st = L.lib().dq_diag_schema_cell(kind, b, len(b), precision, scale, ctypes.byref(res), ctypes.byref(val))
    assert st == L.DQ_OK, L.lib().dq_last_error()
    return res.value, val.value


def expect_int(text):
    v = S.int_cell(text)
    return (0, 0) if v is None else (1, v)


def expect_decimal(text, p, s):
    v = S.decimal_cell(text, p, s)
    return (2, 0) if v == S.DECLINE else (0, 0) if v is None else (1, v)


def table_of(case):
    return d.Table.from_rows(case["columns"], ["string"] * len(case["columns"]), case["rows"])


def columns_of(case):
    return OrderedDict((c, ("string", [r[i] for r in case["rows"]])) for i, c in enumerate(case["columns"]))


# ---------------------------------------------------------------- builders
def test_builder_defaults_and_immutability():
    s0 = d.RowLevelSchema()
    assert s0.columnDefinitions == ()
    s1 = s0.withStringColumn("a")
    s2 = s1.withIntColumn("b")
    s3 = s2.withDecimalColumn("c", 10, 2)
    s4 = s3.withTimestampColumn("t", "yyyy-MM-dd")
    assert s0.columnDefinitions == () and len(s1.columnDefinitions) == 1 and len(s2.columnDefinitions) == 2
    assert s4.columnDefinitions == (
        StringColumnDefinition("a", True, None, None, None), IntColumnDefinition("b", True, None, None),
        DecimalColumnDefinition("c", 10, 2, True), TimestampColumnDefinition("t", "yyyy-MM-dd", True))
    assert s1 == d.RowLevelSchema().withStringColumn("a") and s1 != s2 and hash(s1) == hash(d.RowLevelSchema(s1.columnDefinitions))
    with pytest.raises(AttributeError):
        s1.columnDefinitions = ()
    with pytest.raises(AttributeError):
        s1.other = 1
    full = d.RowLevelSchema().withStringColumn(name="n", isNullable=False, minLength=1, maxLength=2, matches="x") \
        .withIntColumn(name="i", isNullable=False, minValue=-1, maxValue=1) \
        .withDecimalColumn(name="d", precision=5, scale=1, isNullable=False) \
        .withTimestampColumn(name="t", mask="m", isNullable=False)
    assert full.columnDefinitions == (
        StringColumnDefinition("n", False, 1, 2, "x"), IntColumnDefinition("i", False, -1, 1),
        DecimalColumnDefinition("d", 5, 1, False), TimestampColumnDefinition("t", "m", False))


# ---------------------------------------------------------------- plan-time declines and errors
STRINGS = OrderedDict([("s", "string"), ("n", "int64")])


@pytest.mark.parametrize("schema,needle", [
    (d.RowLevelSchema().withTimestampColumn("s", "yyyy-MM-dd"), "timestamp"),
    (d.RowLevelSchema().withStringColumn("s").withTimestampColumn("s", "yyyy", isNullable=False), "timestamp"),
    (d.RowLevelSchema().withStringColumn("s", matches=r"(a)\1"), "matches"),
    (d.RowLevelSchema().withStringColumn("s", matches=r"a*"), "matches"),
    (d.RowLevelSchema().withStringColumn("s", matches=P.STATE_CAP_PATTERN), "matches"),
    (d.RowLevelSchema().withIntColumn("n"), "string columns"),
    (d.RowLevelSchema().withStringColumn("n", maxLength=3), "string columns"),
    (d.RowLevelSchema().withDecimalColumn("n", 5, 2), "string columns"),
    (d.RowLevelSchema().withDecimalColumn("s", 19, 2), "precision"),
    (d.RowLevelSchema().withDecimalColumn("s", 38, 38), "precision"),
])
def test_plan_time_declines(schema, needle):
    with pytest.raises(L.UnsupportedOnGpu) as e:
        check_schema(schema, STRINGS)
    assert needle in str(e.value), str(e.value)
    table = d.Table.from_pydict({"s": ("string", ["1"]), "n": ("int64", [1])})
    with pytest.raises(L.UnsupportedOnGpu):
        d.RowLevelSchemaValidator.validate(table, schema)


def test_declined_pattern_carries_the_compilers_message():
    pb = r"(a)\1".encode()
    m = ctypes.c_int32()
    assert L.lib().dq_diag_regex_match(pb, len(pb), b"", 0, ctypes.byref(m), None, None) == L.DQ_ERR_UNSUPPORTED
    compiler = L.lib().dq_last_error().decode()
    with pytest.raises(L.UnsupportedOnGpu) as e:
        check_schema(d.RowLevelSchema().withStringColumn("s", matches=r"(a)\1"), STRINGS)
    assert compiler and compiler in str(e.value)


def test_sharded_table_is_declined():
    table = d.Table.from_pydict({"s": ("string", ["1"])})
    with pytest.raises(L.UnsupportedOnGpu):
        d.RowLevelSchemaValidator.validate(ShardedTable(table), d.RowLevelSchema().withIntColumn("s"))


@pytest.mark.parametrize("schema", [
    d.RowLevelSchema().withIntColumn("missing"),
    d.RowLevelSchema().withStringColumn("s").withDecimalColumn("nope", 5, 2),
    d.RowLevelSchema().withDecimalColumn("s", 0, 0),
    d.RowLevelSchema().withDecimalColumn("s", 39, 2),
    d.RowLevelSchema().withDecimalColumn("s", 5, 6),
    d.RowLevelSchema().withDecimalColumn("s", 5, -1),
    # (Spark's errors come before anything is declined)
    d.RowLevelSchema().withTimestampColumn("s", "yyyy").withIntColumn("missing"),
])
def test_value_errors(schema):
    with pytest.raises(ValueError):
        check_schema(schema, STRINGS)
    table = d.Table.from_pydict({"s": ("string", ["1"]), "n": ("int64", [1])})
    with pytest.raises(ValueError):
        d.RowLevelSchemaValidator.validate(table, schema)


def test_supported_schemas_pass_the_plan_check():
    check_schema(d.RowLevelSchema(), STRINGS)
    check_schema(d.RowLevelSchema().withIntColumn("s", False, -5, 5).withDecimalColumn("s", 18, 18)
                 .withStringColumn("s", False, 0, 9, P.EMAIL), STRINGS)


# ---------------------------------------------------------------- the reference's cases
CASES = S.known_answers()


def test_known_answers_are_the_seven_reference_cases():
    assert len(CASES) == 7 and sum(c["timestamp"] for c in CASES) == 3
    for c in CASES:
        assert c["timestamp"] == any(dn["kind"] == "timestamp" for dn in c["schema"])
        assert c["source"].startswith("src/test/scala/com/amazon/deequ/schema/RowLevelSchemaValidatorTest.scala:")


@pytest.mark.parametrize("case", [c for c in CASES if not c["timestamp"]], ids=lambda c: c["id"])
def test_mirror_reproduces_reference_case(case):
    m = S.mirror(columns_of(case), case["schema"])
    assert len(m.valid_idx) == case["numValidRows"] and len(m.invalid_idx) == case["numInvalidRows"]
    assert not m.declined and not m.null_idx
    if "valid_members" in case:
        got = m.valid_cols[case["valid_members"]["column"]][1]
        assert len(got) == case["numValidRows"] and set(got) == set(case["valid_members"]["values"])
    check_schema(S.build_schema(case["schema"]), d.Table.from_rows(
        case["columns"], ["string"] * len(case["columns"]), case["rows"]).schema)


@pytest.mark.parametrize("case", [c for c in CASES if c["timestamp"]], ids=lambda c: c["id"])
def test_timestamp_cases_are_declined(case):
    with pytest.raises(L.UnsupportedOnGpu) as e:
        d.RowLevelSchemaValidator.validate(table_of(case), S.build_schema(case["schema"]))
    assert "timestamp" in str(e.value)


def test_mirror_line_246():
    """A NULL cell of a nullable int column with a minValue: the row is in neither output."""
    cols = OrderedDict([("i", ("string", ["5", None, "x", "-3"]))])
    m = S.mirror(cols, [{"kind": "int", "name": "i", "minValue": 0}])
    assert (m.valid_idx, m.invalid_idx, m.null_idx) == ([0], [2, 3], [1])
    m = S.mirror(cols, [{"kind": "int", "name": "i", "maxValue": 9}])  # maxValue uses colIsNull: never NULL
    assert (m.valid_idx, m.invalid_idx, m.null_idx) == ([0, 1, 3], [2], [])
    both = OrderedDict([("i", ("string", [None, None])), ("s", ("string", ["toolong", "ok"]))])
    m = S.mirror(both, [{"kind": "int", "name": "i", "minValue": 0}, {"kind": "string", "name": "s", "maxLength": 3}])
    assert (m.valid_idx, m.invalid_idx, m.null_idx) == ([], [0], [1])  # FALSE wins over NULL


# ---------------------------------------------------------------- the shared cell tests
def test_cells_by_hand():
    """Values worked out from the reference's definitions, independent of the restatement."""
    for text, want in [(".", (1, 0)), ("+", (0, 0)), ("-", (0, 0)), ("1.", (1, 1)), (".5", (1, 0)), ("1.9", (1, 1)),
                       ("-1.9", (1, -1)), ("2147483647", (1, 2147483647)), ("2147483648", (0, 0)),
                       ("-2147483648", (1, -2147483648)), ("-2147483649", (0, 0)), (" 1", (0, 0)), ("1 ", (0, 0)),
                       ("", (0, 0)), ("1.2x", (0, 0)), ("1e2", (0, 0)), ("+7", (1, 7))]:
        assert schema_cell(L.DQ_SCHEMA_INT, text) == want, text
    for text, p, s, want in [("99.995", 4, 2, (0, 0)), ("9.995", 4, 2, (1, 1000)), ("99.994", 4, 2, (1, 9999)),
                             ("0.005", 4, 2, (1, 1)), ("-0.005", 4, 2, (1, -1)), ("0.004", 4, 2, (1, 0)),
                             ("1e2", 4, 2, (0, 0)), ("1e2", 5, 2, (1, 10000)), ("1E-3", 4, 2, (1, 0)),
                             ("5E-3", 4, 2, (1, 1)), ("1e", 4, 2, (0, 0)), ("e1", 4, 2, (0, 0)), (".", 4, 2, (0, 0)),
                             ("1.", 4, 2, (1, 100)), (".5", 4, 2, (1, 50)), (" 1", 4, 2, (0, 0)), ("1 ", 4, 2, (0, 0)),
                             ("", 4, 2, (0, 0)), ("0" * 40 + "7", 4, 2, (1, 700)), ("0." + "3" * 30, 4, 2, (1, 33)),
                             ("NaN", 4, 2, (0, 0)), ("Infinity", 4, 2, (0, 0)), ("1_0", 4, 2, (0, 0)),
                             ("299.000", 10, 2, (1, 29900)), ("-99.99", 10, 2, (1, -9999)),
                             ("1e5000", 10, 2, (2, 0)), ("1é", 10, 2, (2, 0)), ("9" * 18, 18, 0, (1, 10 ** 18 - 1)),
                             ("9" * 18 + ".5", 18, 0, (0, 0)), ("9" * 19, 18, 0, (0, 0)), ("1e17", 18, 0, (1, 10 ** 17)),
                             ("1e18", 18, 0, (0, 0)), ("0.5", 1, 0, (1, 1)), ("9.5", 1, 0, (0, 0))]:
        assert schema_cell(L.DQ_SCHEMA_DECIMAL, text, p, s) == want, (text, p, s)


def test_hostile_cells_equal_the_mirror():
    cells = S.HOSTILE_NUMBERS + S.HOSTILE_DECLINED + S.MULTIBYTE_TEXT
    assert {".", "+", "-", "1.", ".5", "1.9", "2147483647", "2147483648", "-2147483648", "-2147483649", " 1", "1 ",
            "99.995", "9.995", "0.005", "-0.005", "1e2", "1E-3", "1e", "e1", ""} <= set(cells)
    assert "0" * 40 + "7" in cells and "0." + "3" * 30 in cells
    for text in cells:
        assert schema_cell(L.DQ_SCHEMA_INT, text) == expect_int(text), text
        for p, s in S.DECIMAL_TYPES:
            assert schema_cell(L.DQ_SCHEMA_DECIMAL, text, p, s) == expect_decimal(text, p, s), (text, p, s)
    for text in S.HOSTILE_DECLINED:
        assert schema_cell(L.DQ_SCHEMA_DECIMAL, text, 10, 2)[0] == 2, text


def test_generated_cells_equal_the_mirror():
    rng = np.random.default_rng(20240)
    cells = S.random_numbers(20000, rng)
    seen = {0: 0, 1: 0}
    seen_int = {0: 0, 1: 0}
    for k, text in enumerate(cells):
        got = schema_cell(L.DQ_SCHEMA_INT, text)
        assert got == expect_int(text), text
        seen_int[got[0]] += 1
        p, s = S.DECIMAL_TYPES[k % len(S.DECIMAL_TYPES)]
        got = schema_cell(L.DQ_SCHEMA_DECIMAL, text, p, s)
        assert got == expect_decimal(text, p, s), (text, p, s)
        seen[got[0]] = seen.get(got[0], 0) + 1  # (2: noise that happens to spell an exponent beyond 1000)
    # (an always-valid or always-invalid cell test cannot pass)
    assert min(seen[0], seen[1]) > 2000 and min(seen_int.values()) > 2000, (seen, seen_int)


def test_diag_schema_cell_rejects_bad_arguments():
    res, val = ctypes.c_int32(), ctypes.c_int64()
    f = L.lib().dq_diag_schema_cell
    assert f(L.DQ_SCHEMA_DECIMAL, b"1", 1, 19, 0, ctypes.byref(res), ctypes.byref(val)) == L.DQ_ERR_INVALID
    assert f(L.DQ_SCHEMA_DECIMAL, b"1", 1, 5, 6, ctypes.byref(res), ctypes.byref(val)) == L.DQ_ERR_INVALID
    assert f(L.DQ_SCHEMA_STRING, b"1", 1, 0, 0, ctypes.byref(res), ctypes.byref(val)) == L.DQ_ERR_INVALID
