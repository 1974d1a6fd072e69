"""CPU tests of the cross-table checks: the independent restatement (match_restated.py) on the
worked example, every argument error (raised before any device work), and the host build of the
cell equality (dq_diag_cell_equal: the source the match kernel runs) against the restatement over
the boundary cells of match_cases.py."""
import ctypes

import pytest

import deequ_amd as d
import match_cases as C
import match_restated as M
from deequ_amd import _lib as L
from helpers import oracle_table, product_table

T, F, N = True, False, None
KV = [("id", "id")]
CMP = [("v", "v"), ("s", "s")]


# ---------------------------------------------------------------- the restatement: worked example
def test_worked_example_referential_integrity():
    a, b = oracle_table(M.EXAMPLE_A), oracle_table(M.EXAMPLE_B)
    got = M.referential_integrity(a, ["id"], b, ["id"])
    assert got == [T, T, T, F, F, T]
    assert M.state_of(got) == (4, 6)


def test_worked_example_dataset_match():
    a, b = oracle_table(M.EXAMPLE_A), oracle_table(M.EXAMPLE_B)
    got = M.dataset_match(a, b, KV, CMP)
    assert got == [T, T, T, F, F, F]
    assert M.state_of(got) == (3, 6)
    assert M.counts(a, b, KV, CMP) == {"matched": 3, "key_null": 1, "key_absent": 1, "cells_differ": 1, "selected": 6}
    assert M.reference_rows(a, ["id"], b, ["id"]) == [3, 2, 1, -1, -1, 0]


def test_worked_example_with_where():
    a, b = oracle_table(M.EXAMPLE_A), oracle_table(M.EXAMPLE_B)
    got = M.dataset_match(a, b, KV, CMP, where="id < 9")
    assert got == [T, T, T, N, N, F]
    assert M.state_of(got) == (3, 4)
    c = M.counts(a, b, KV, CMP, where="id < 9")
    assert c["matched"] + c["key_null"] + c["key_absent"] + c["cells_differ"] == c["selected"] == 4
    assert M.state_of(M.dataset_match(a, b, KV, CMP, where="id > 100")) is None


def test_restated_duplicates_and_null_keys_in_the_reference():
    a = oracle_table({"k": ("int64", [1, 2, None])})
    dup = oracle_table({"k": ("int64", [1, 1, 2, None, None])})
    with pytest.raises(ValueError, match="1 groups"):
        M.dataset_match(a, dup, [("k", "k")])
    assert M.referential_integrity(a, ["k"], dup, ["k"]) == [T, T, F]
    nulls = oracle_table({"k": ("int64", [None, 2, None])})  # (NULL-key rows are unreachable, and allowed)
    assert M.dataset_match(a, nulls, [("k", "k")]) == [F, T, F]
    assert M.reference_rows(a, ["k"], nulls, ["k"]) == [-1, 1, -1]


# ---------------------------------------------------------------- argument errors (no device)
A_SPEC = {"id": ("int64", [1, 2]), "v": ("float64", [1.0, 2.0]), "s": ("string", ["a", "b"]),
          "dec": ("decimal(10,2)", [1, 2])}
B_SPEC = {"id": ("int64", [1, 2]), "v": ("float64", [1.0, 2.0]), "s": ("string", ["a", "b"]), "w": ("int32", [1, 2]),
          "dec": ("decimal(10,2)", [1, 2])}


def _tables():
    return product_table(A_SPEC), product_table(B_SPEC)


def test_unknown_columns_raise_value_error():
    a, b = _tables()
    with pytest.raises(ValueError, match="nope"):
        d.dataset_match(a, b, ["nope"])
    with pytest.raises(ValueError, match="nope"):
        d.dataset_match(a, b, [("id", "nope")])
    with pytest.raises(ValueError, match="nope"):
        d.dataset_match(a, b, ["id"], compare=["nope"])
    with pytest.raises(ValueError, match="nope"):
        d.referential_integrity(a, ["nope"], b)
    with pytest.raises(ValueError, match="nope"):
        d.referential_integrity(a, ["id"], b, ["nope"])


def test_empty_keys_raise_value_error():
    a, b = _tables()
    with pytest.raises(ValueError, match="at least one key"):
        d.dataset_match(a, b, [])
    with pytest.raises(ValueError, match="at least one key"):
        d.referential_integrity(a, [], b)
    with pytest.raises(ValueError):
        d.referential_integrity(a, ["id", "v"], b, ["id"])


def test_unequal_dtypes_raise_value_error():
    a, b = _tables()
    with pytest.raises(ValueError, match="int64.*int32"):
        d.dataset_match(a, b, [("id", "w")])
    with pytest.raises(ValueError, match="float64.*int32"):
        d.dataset_match(a, b, ["id"], compare=[("v", "w")])
    with pytest.raises(ValueError, match="int64.*int32"):
        d.referential_integrity(a, ["id"], b, ["w"])


def test_exactly_one_reference():
    a, b = _tables()
    with pytest.raises(ValueError, match="exactly one"):
        d.referential_integrity(a, ["id"])
    with pytest.raises(ValueError, match="exactly one"):
        d.referential_integrity(a, ["id"], b, reference_state=object())


def test_decimal_keys_are_declined_as_the_group_by_declines_them():
    a, b = _tables()
    with pytest.raises(L.UnsupportedOnGpu, match="dec"):
        d.dataset_match(a, b, ["dec"])
    with pytest.raises(L.UnsupportedOnGpu, match="dec"):
        d.referential_integrity(a, ["dec"], b)


def test_a_where_the_compiler_declines_is_declined_alike():
    from deequ_amd.predicates import UnsupportedPredicate, compile_predicate
    from deequ_amd.engine import schema_index
    a, b = _tables()
    where = "upper(s) = 'A'"
    with pytest.raises((UnsupportedPredicate, ValueError)) as want:
        compile_predicate(where, schema_index(a.schema))
    for call in (lambda: d.dataset_match(a, b, ["id"], where=where),
                 lambda: d.referential_integrity(a, ["id"], b, where=where)):
        with pytest.raises(type(want.value)) as got:
            call()
        assert str(got.value) == str(want.value)  # (unchanged message)


def test_sharded_and_multi_batch_inputs_are_unsupported():
    from deequ_amd.distributed import ShardedTable
    a, b = _tables()
    with pytest.raises(L.UnsupportedOnGpu, match="ShardedTable"):
        d.dataset_match(ShardedTable(a), b, ["id"])
    with pytest.raises(L.UnsupportedOnGpu, match="ShardedTable"):
        d.referential_integrity(ShardedTable(a), ["id"], b)
    with pytest.raises(L.UnsupportedOnGpu, match="2 batches"):
        d.dataset_match(a, d.PartitionedTable([b, b]), ["id"])

    class ShardedState:  # (anything that is not a FrequenciesAndNumRows held on this GPU)
        pass
    with pytest.raises(L.UnsupportedOnGpu, match="ShardedState"):
        d.referential_integrity(a, ["id"], reference_state=ShardedState())


def test_histogram_state_is_invalid_and_other_keys_are_rejected():
    from deequ_amd.frequencies import FrequenciesAndNumRows
    from fake_freq import FakeFrequencyTable
    a, _ = _tables()
    hist = FrequenciesAndNumRows(FakeFrequencyTable(["id"], {"id": "int64"}, histogram=True))
    with pytest.raises(L.DeequAmdError) as e:
        d.referential_integrity(a, ["id"], reference_state=hist)
    assert e.value.status == L.DQ_ERR_INVALID and not isinstance(e.value, L.UnsupportedOnGpu)
    other = FrequenciesAndNumRows(FakeFrequencyTable(["id"], {"id": "int32"}))
    with pytest.raises(ValueError, match="int64.*int32"):
        d.referential_integrity(a, ["id"], reference_state=other)
    with pytest.raises(ValueError, match="groups"):
        d.referential_integrity(a, ["id"], reference_columns=["s"],
                                reference_state=FrequenciesAndNumRows(FakeFrequencyTable(["id"], {"id": "int64"})))


def test_more_than_32_compare_pairs_are_unsupported():
    a, b = _tables()
    with pytest.raises(L.UnsupportedOnGpu, match="32"):
        d.dataset_match(a, b, ["id"], compare=["v"] * 33)


# ---------------------------------------------------------------- the cell equality (host build)
def _lib_equal(ca, i, cb, j) -> bool:
    out = ctypes.c_int32(-1)
    da, db = ca.to_dq(), cb.to_dq()
    L.check(L.lib().dq_diag_cell_equal(ctypes.byref(da), i, ctypes.byref(db), j, ctypes.byref(out)))
    assert out.value in (0, 1)
    return bool(out.value)


@pytest.mark.parametrize("dtype", C.DTYPES)
def test_cell_equal_matches_the_restatement_on_every_pair(dtype):
    values = C.cells(dtype)
    ca, cb = C.column(dtype, values), C.column(dtype, list(reversed(values)))
    back = list(reversed(values))
    n = len(values)
    equal_pairs = 0
    for i in range(n):
        for j in range(n):
            want = M.cell_equal(values[i], back[j], dtype)
            assert _lib_equal(ca, i, cb, j) == want, (dtype, values[i], back[j])
            assert _lib_equal(cb, j, ca, i) == want, (dtype, "swapped", values[i], back[j])  # each follows the other
            equal_pairs += want
    assert n <= equal_pairs < n * n  # (both verdicts occur)


def test_cell_equal_nan_payloads_zeros_and_infinities():
    for dtype in ("float32", "float64"):
        values = C.cells(dtype)
        col = C.column(dtype, values)
        nans = [i for i, v in enumerate(values) if v is not None and v != v]
        assert len(nans) >= 4
        raw = col.values.view("u4" if dtype == "float32" else "u8")
        assert len({int(raw[i]) for i in nans}) == len(nans)  # (really different payloads)
        for i in nans:
            for j in nans:
                assert _lib_equal(col, i, col, j)
            assert not _lib_equal(col, i, col, values.index(1.0))
        assert _lib_equal(col, 0, col, 1) and values[0] == 0.0 and str(values[1]) == "-0.0"
        assert not _lib_equal(col, values.index(float("inf")), col, values.index(float("-inf")))


def test_cell_equal_never_reads_a_null_slot_or_outside_the_window():
    """Sliced columns (offset 3): the NULL slots and the rows outside the window hold other values."""
    a = d.Column.from_pylist(["zzz", "yy", "x", "same", None, "tail"], "string")
    b = d.Column.from_pylist(["q", "same", "other", "tail"], "string")
    a3 = d.Column("string", 3, a.values, a.validity, offsets=a.offsets, offset=3)
    b1 = d.Column("string", 3, b.values, None, offsets=b.offsets, offset=1)
    assert [_lib_equal(a3, i, b1, j) for i in range(3) for j in range(3)] == [T, F, F, F, F, F, F, F, T]
    x = d.Column.from_pylist([True, False, True, None, False, True, True, False, None, True, False], "bool")
    x9 = d.Column("bool", 2, x.values, x.validity, offset=9)
    assert _lib_equal(x9, 0, x, 0) and _lib_equal(x9, 1, x, 1) and not _lib_equal(x9, 0, x, 1)
    assert _lib_equal(x, 3, x, 8) and not _lib_equal(x, 3, x, 4)  # NULL <=> NULL, NULL <=> FALSE


def test_cell_equal_rejects_bad_arguments():
    a = d.Column.from_pylist([1, 2], "int64").to_dq()
    b = d.Column.from_pylist([1, 2], "int32").to_dq()
    out = ctypes.c_int32()
    lib = L.lib()
    assert lib.dq_diag_cell_equal(ctypes.byref(a), 0, ctypes.byref(b), 0, ctypes.byref(out)) == L.DQ_ERR_INVALID
    assert lib.dq_diag_cell_equal(ctypes.byref(a), 2, ctypes.byref(a), 0, ctypes.byref(out)) == L.DQ_ERR_INVALID
    assert lib.dq_diag_cell_equal(ctypes.byref(a), 0, ctypes.byref(a), -1, ctypes.byref(out)) == L.DQ_ERR_INVALID
    p, q = d.Column.from_pylist([1], "decimal(10,2)").to_dq(), d.Column.from_pylist([1], "decimal(10,3)").to_dq()
    assert lib.dq_diag_cell_equal(ctypes.byref(p), 0, ctypes.byref(q), 0, ctypes.byref(out)) == L.DQ_ERR_INVALID
