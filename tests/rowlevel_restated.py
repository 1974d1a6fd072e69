"""An independent restatement of the row-level outcomes (deequ_amd/rowlevel.py), shared by
test_rowlevel.py and test_gpu_rowlevel.py.  Plain Python over the oracle's tables:

* `where` and Compliance row by row through `O.eval_predicate` (SQL three-valued logic);
* PatternMatch from the per-row expectations of tests/pattern_cases.py (its `oracle`, or the
  hand-written answers of JAVA_LINE_CASES);
* Uniqueness from a `collections.Counter` over the key tuples of the selected rows.

An outcome is True, False or None (NULL) per row.  A row that `where` does not select (FALSE or
NULL) is None; the rules for a selected row are those of DESIGN.md §3, "Row-level outcomes", restated
in each function."""
import struct
from collections import Counter
from typing import Dict, List, Optional, Sequence

import pyoracle as O


def num_rows(table) -> int:
    return len(next(iter(table.values())).values)


def selected(table, where: Optional[str]) -> List[bool]:
    """The rows `where` selects: TRUE only (FALSE and NULL are dropped, as Spark's filter drops them)."""
    if where is None:
        return [True] * num_rows(table)
    return [v is True for v in O.eval_predicate(where, table)]


def _outcomes(sel: Sequence[bool], cond: Sequence[bool]) -> List[Optional[bool]]:
    return [bool(c) if s else None for s, c in zip(sel, cond)]


def completeness(table, column: str, where: Optional[str] = None):
    """TRUE iff the column is not NULL."""
    return _outcomes(selected(table, where), [v is not None for v in table[column].values])


def compliance(table, predicate: str, where: Optional[str] = None):
    """TRUE iff the predicate is TRUE; NULL counts as FALSE (Compliance.scala sums when(p, 1).otherwise(0))."""
    return _outcomes(selected(table, where), [v is True for v in O.eval_predicate(predicate, table)])


def pattern_match(table, column: str, expected: Sequence[int], where: Optional[str] = None):
    """TRUE iff the row's expectation says the pattern matches; a NULL value is FALSE.  `expected`
    holds one 0 / 1 per row (ignored where the value is NULL)."""
    values = table[column].values
    return _outcomes(selected(table, where), [v is not None and bool(e) for v, e in zip(values, expected)])


def key_identity(value, dtype: str):
    """What groups a value: floats by their bits (Spark 2.2 groups UnsafeRow bytes: -0.0 and 0.0,
    and NaNs of different payloads, are different keys), everything else by itself."""
    if value is None:
        return None
    if dtype == "float64":
        return struct.pack("<d", value)
    if dtype == "float32":
        return struct.pack("<f", value)
    if dtype == "bool":
        return bool(value)
    return value


def keys_of(table, columns: Sequence[str]) -> List[Optional[tuple]]:
    """Per row the key tuple, or None when any key column is NULL (the row is in no group)."""
    cols = [[key_identity(v, table[c].dtype) for v in table[c].values] for c in columns]
    return [None if any(v is None for v in row) else tuple(row) for row in zip(*cols)]


def frequencies(table, columns: Sequence[str], where: Optional[str] = None) -> Counter:
    """The groups of the selected rows: what the FrequenciesAndNumRows state of the table holds."""
    return Counter(k for k, s in zip(keys_of(table, columns), selected(table, where)) if s and k is not None)


def uniqueness(table, columns: Sequence[str], where: Optional[str] = None, state: Optional[Dict] = None):
    """TRUE iff the row's key has count exactly 1 in `state` (default: the table's own groups under
    the same `where`).  A NULL key column and a key absent from the state are FALSE."""
    groups = frequencies(table, columns, where) if state is None else state
    return _outcomes(selected(table, where), [k is not None and groups.get(k, 0) == 1 for k in keys_of(table, columns)])


def counts(outcomes) -> tuple:
    """(TRUE, FALSE, NULL)."""
    t = sum(1 for v in outcomes if v is True)
    f = sum(1 for v in outcomes if v is False)
    return t, f, len(outcomes) - t - f


def rows(outcomes, which) -> List[int]:
    """Ascending indices of the rows whose outcome is `which` (True, False or None)."""
    return [i for i, v in enumerate(outcomes) if v is which]
