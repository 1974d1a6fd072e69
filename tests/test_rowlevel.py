"""CPU tests of the row-level outcomes: the independent restatement (rowlevel_restated.py) against
hand-written tables, the refusals that need no device, and the bitmap layout helpers."""
import numpy as np
import pytest

import deequ_amd as d
import rowlevel_restated as R
from deequ_amd import _lib as L
from deequ_amd import rowlevel
from helpers import oracle_table, product_table

T, F, N = True, False, None

SPEC = {
    "id": ("int64", [1, 2, 2, None, 5, 6, 6, 6]),
    "s": ("string", ["a", None, "b", "b", "", "c", "c", None]),
    "q": ("int64", [3, -1, None, 4, 0, 7, None, 2]),
}


# ---------------------------------------------------------------- the restatement
def test_restated_completeness_by_hand():
    t = oracle_table(SPEC)
    assert R.completeness(t, "s") == [T, F, T, T, T, T, T, F]
    # q > 0 is TRUE on rows 0, 3, 5, 7; FALSE on 1, 4; NULL on 2, 6
    assert R.completeness(t, "s", "q > 0") == [T, N, N, T, N, T, N, F]


def test_restated_compliance_null_counts_as_false():
    t = oracle_table(SPEC)
    assert R.compliance(t, "q > 0") == [T, F, F, T, F, T, F, T]
    assert R.compliance(t, "q > 0", "id IS NOT NULL") == [T, F, F, N, F, T, F, T]
    assert R.counts(R.compliance(t, "q > 0", "id IS NOT NULL")) == (3, 4, 1)


def test_restated_pattern_match_null_value_is_false():
    t = oracle_table(SPEC)
    expected = [1, 1, 0, 1, 0, 0, 1, 1]  # (rows 1 and 7 are NULL: their expectation is ignored)
    assert R.pattern_match(t, "s", expected) == [T, F, F, T, F, F, T, F]
    assert R.pattern_match(t, "s", expected, "q >= 0") == [T, N, N, T, F, F, N, F]


def test_restated_uniqueness_null_keys_and_absent_keys():
    t = oracle_table(SPEC)
    # id: 1 and 5 are unique, 2 and 6 are not, the NULL is in no group
    assert R.uniqueness(t, ["id"]) == [T, F, F, F, T, F, F, F]
    # (id, s): a NULL in either column takes the row out of every group
    assert R.uniqueness(t, ["id", "s"]) == [T, F, T, F, T, F, F, F]
    # with a filter the groups are those of the selected rows: q > 2 keeps one of the three 6s
    assert R.uniqueness(t, ["id"], "q > 2") == [T, N, N, F, N, T, N, N]
    assert R.uniqueness(t, ["id"], "q > 0") == [T, N, N, F, N, F, N, F]
    # a state from elsewhere: 1 is duplicated there, 5 is absent, 2 is unique
    assert R.uniqueness(t, ["id"], state={(1,): 2, (2,): 1, (6,): 1}) == [F, T, T, F, F, T, T, T]
    assert R.frequencies(t, ["id"]) == {(1,): 1, (2,): 2, (5,): 1, (6,): 3}


def test_restated_float_keys_group_by_bits():
    t = oracle_table({"f": ("float64", [0.0, -0.0, float("nan"), float("nan"), 1.5])})
    assert R.uniqueness(t, ["f"]) == [T, T, F, F, T]


def test_restated_invariants_tie_outcomes_to_oracle_states():
    import pyoracle as O
    t = oracle_table(SPEC)
    for where in (None, "q > 0", "id < 0"):
        tr, fa, _ = R.counts(R.completeness(t, "s", where))
        st = O.completeness_state(t, "s", where)
        assert (tr, tr + fa) == (st.num_matches, st.count)
        tr, fa, _ = R.counts(R.compliance(t, "q >= 3", where))
        st = O.compliance_state(t, "q >= 3", where)  # (None: the sum over no selected row is NULL)
        assert (tr, tr + fa) == ((st.num_matches, st.count) if st is not None else (0, 0))
    tr, fa, _ = R.counts(R.uniqueness(t, ["id"]))
    st = O.frequencies_state(t, ["id"])
    assert tr == sum(1 for c in st.frequencies.values() if c == 1) and tr + fa == st.num_rows
    assert R.rows(R.uniqueness(t, ["id"]), False) == [1, 2, 3, 5, 6, 7]


# ---------------------------------------------------------------- refusals
@pytest.mark.parametrize("analyzer", [d.Size(), d.Distinctness(["id"]), d.Entropy("id"), d.Mean("q"),
                                      d.MinLength("s"), d.DataType("s"), d.Histogram("id"),
                                      d.UniqueValueRatio(["id"]), d.MutualInformation(["id", "s"])])
def test_analyzers_without_a_row_meaning_raise_value_error(analyzer):
    with pytest.raises(ValueError, match=type(analyzer).__name__):
        d.row_level_results(product_table(SPEC), [d.Completeness("s"), analyzer])


def test_sharded_table_is_declined():
    from deequ_amd.distributed import ShardedTable
    with pytest.raises(L.UnsupportedOnGpu, match="ShardedTable"):
        d.row_level_results(ShardedTable(product_table(SPEC)), [d.Uniqueness(["id"])])


def test_histogram_state_is_invalid():
    from deequ_amd.frequencies import FrequenciesAndNumRows
    from fake_freq import FakeFrequencyTable
    a = d.Uniqueness(["id"])
    state = FrequenciesAndNumRows(FakeFrequencyTable(["id"], {"id": "int64"}, histogram=True))
    with pytest.raises(L.DeequAmdError) as e:
        d.row_level_results(product_table(SPEC), [a], states={a: state})
    assert e.value.status == L.DQ_ERR_INVALID and not isinstance(e.value, L.UnsupportedOnGpu)


def test_state_over_other_columns_or_types_is_rejected():
    from deequ_amd.frequencies import FrequenciesAndNumRows
    from fake_freq import FakeFrequencyTable
    a = d.Uniqueness(["id"])
    for cols, schema in ((["s"], {"s": "string"}), (["id"], {"id": "int32"})):
        with pytest.raises(ValueError):
            d.row_level_results(product_table(SPEC), [a],
                                states={a: FrequenciesAndNumRows(FakeFrequencyTable(cols, schema))})


def test_what_the_analyzer_declines_is_declined_alike():
    from deequ_amd.predicates import UnsupportedPredicate
    table = product_table(SPEC)
    with pytest.raises((UnsupportedPredicate, ValueError)):
        d.row_level_results(table, [d.Compliance("c", "upper(s) = 'A'")])
    with pytest.raises(L.UnsupportedOnGpu):  # a back-reference: the scan's PatternMatch declines it too
        d.row_level_results(table, [d.PatternMatch("s", r"(a)\1")])
    with pytest.raises(Exception, match="nope"):
        d.row_level_results(table, [d.Completeness("nope")])


# ---------------------------------------------------------------- bitmap layout
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 200])
def test_bitmap_helpers_round_trip(n):
    rng = np.random.default_rng(n)
    bits = rng.random(n) < 0.5
    words = rowlevel.pack_bits(bits)
    assert words.dtype == np.dtype("<u8") and len(words) == rowlevel.bitmap_words(n) == (n + 63) // 64
    assert rowlevel.unpack_bits(words, n).tolist() == bits.tolist()
    for i in range(n):  # LSB first: row i is bit i % 64 of word i // 64
        assert bool((int(words[i // 64]) >> (i % 64)) & 1) == bool(bits[i])
    if n % 64:  # the trailing bits of the last word are 0
        assert int(words[-1]) >> (n % 64) == 0


def test_outcomes_from_bitmaps():
    value = rowlevel.pack_bits([1, 0, 1, 0])
    valid = rowlevel.pack_bits([1, 1, 0, 0])
    assert rowlevel.outcomes_from_bitmaps(value, valid, 4) == [T, F, N, N]
    # the same bytes are an Arrow boolean array: a bool Column reads them back alike
    col = d.Column("bool", 4, value.view(np.uint8), valid.view(np.uint8))
    assert col.to_pylist() == [T, F, N, N]
