"""An independent restatement of the cross-table checks (deequ_amd/comparison.py), shared by
test_match.py and test_gpu_match.py: a plain Python dict join over the oracle's tables
(`helpers.oracle_table` columns), with no import of deequ_amd.

`A` is the primary table, `B` the reference.  An outcome is True, False or None (NULL) per row of
`A`: None where `where` does not select the row (FALSE or NULL); for a selected row

* referential_integrity: True iff every key column is non-NULL and some row of B holds the key;
* dataset_match: True iff the key is non-NULL, B holds it in row j, and every compare pair is
  NULL-safe equal between row i of A and row j of B.

Key identity is the group-by's (rowlevel_restated.key_identity: floats by their bits).  Cell equality
is Spark's `<=>`: NULL equals NULL only; floats compare as doubles with NaN == NaN and -0.0 == 0.0;
everything else by value (strings by their UTF-8 bytes)."""
import math
from typing import Dict, List, Optional, Sequence, Tuple

import rowlevel_restated as R


def cell_equal(a, b, dtype: str) -> bool:
    """a <=> b for two cells of one dtype (None = NULL)."""
    if a is None or b is None:
        return a is None and b is None
    if dtype in ("float32", "float64"):
        a, b = float(a), float(b)
        if math.isnan(a) or math.isnan(b):
            return math.isnan(a) and math.isnan(b)
        return a == b  # (-0.0 == 0.0 holds)
    if dtype == "string":
        return a.encode("utf-8") == b.encode("utf-8")
    if dtype == "bool":
        return bool(a) == bool(b)
    return a == b


def key_rows(b_table, b_keys: Sequence[str]) -> Dict[tuple, List[int]]:
    """key -> the rows of B holding it (rows with a NULL key column are in no entry)."""
    out: Dict[tuple, List[int]] = {}
    for j, k in enumerate(R.keys_of(b_table, b_keys)):
        if k is not None:
            out.setdefault(k, []).append(j)
    return out


def duplicate_groups(b_table, b_keys: Sequence[str]) -> int:
    return sum(1 for rows in key_rows(b_table, b_keys).values() if len(rows) > 1)


def reference_rows(a_table, a_keys, b_table, b_keys) -> List[int]:
    """Per row of A the row of B holding its key, or -1 (whatever any `where` says).  B's keys are
    unique, or the lowest row is named."""
    index = key_rows(b_table, b_keys)
    return [-1 if k is None or k not in index else index[k][0] for k in R.keys_of(a_table, a_keys)]


def referential_integrity(a_table, a_keys, b_table=None, b_keys=None, where: Optional[str] = None,
                          state: Optional[Dict[tuple, int]] = None):
    """`state`: the reference keys as {key tuple: count} instead of a table."""
    held = set(state) if state is not None else set(key_rows(b_table, b_keys or a_keys))
    sel = R.selected(a_table, where)
    return [None if not s else (k is not None and k in held) for s, k in zip(sel, R.keys_of(a_table, a_keys))]


def classify(a_table, b_table, key_pairs: Sequence[Tuple[str, str]], cmp_pairs: Sequence[Tuple[str, str]] = ()):
    """Per row of A one of "true", "key_null", "key_absent", "cells_differ" (before any `where`)."""
    a_keys, b_keys = [a for a, _ in key_pairs], [b for _, b in key_pairs]
    if duplicate_groups(b_table, b_keys):
        raise ValueError("%d groups hold more than one row" % duplicate_groups(b_table, b_keys))
    index = key_rows(b_table, b_keys)
    out = []
    for i, k in enumerate(R.keys_of(a_table, a_keys)):
        if k is None:
            out.append("key_null")
        elif k not in index:
            out.append("key_absent")
        else:
            j = index[k][0]
            same = all(cell_equal(a_table[a].values[i], b_table[b].values[j], a_table[a].dtype) for a, b in cmp_pairs)
            out.append("true" if same else "cells_differ")
    return out


def evaluate(a_table, b_table, key_pairs, cmp_pairs=(), where: Optional[str] = None):
    """(outcomes, {"matched", "key_null", "key_absent", "cells_differ", "selected"} over the selected
    rows) of dataset_match, from one pass."""
    sel = R.selected(a_table, where)
    classes = classify(a_table, b_table, key_pairs, cmp_pairs)
    kinds = [c for s, c in zip(sel, classes) if s]
    out = {name: kinds.count(kind) for name, kind in (("matched", "true"), ("key_null", "key_null"),
                                                      ("key_absent", "key_absent"), ("cells_differ", "cells_differ"))}
    out["selected"] = len(kinds)
    return [None if not s else c == "true" for s, c in zip(sel, classes)], out


def dataset_match(a_table, b_table, key_pairs, cmp_pairs=(), where: Optional[str] = None):
    return evaluate(a_table, b_table, key_pairs, cmp_pairs, where)[0]


def counts(a_table, b_table, key_pairs, cmp_pairs=(), where: Optional[str] = None) -> Dict[str, int]:
    return evaluate(a_table, b_table, key_pairs, cmp_pairs, where)[1]


def state_of(outcomes) -> Optional[Tuple[int, int]]:
    """(TRUE rows, selected rows), or None when no row is selected."""
    t, f, _ = R.counts(outcomes)
    return (t, t + f) if t + f else None


# ---------------------------------------------------------------- the worked example
NAN = float("nan")
EXAMPLE_A = {"id": ("int64", [1, 2, 3, None, 9, 4]),
             "v": ("float64", [1.0, NAN, 0.0, 1.0, 1.0, 2.0]),
             "s": ("string", ["a", "b", None, "a", "a", "x"])}
EXAMPLE_B = {"id": ("int64", [4, 3, 2, 1, 7]),
             "v": ("float64", [2.5, -0.0, NAN, 1.0, 0.0]),
             "s": ("string", ["x", None, "b", "a", "z"])}
