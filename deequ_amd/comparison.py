"""Cross-table checks on the GPU: referential integrity and dataset match.

`A` is the primary table, `B` the reference table.  Both checks give every row of `A` one nullable
boolean (the bitmap pair of deequ_amd/rowlevel.py) and the state NumMatchesAndCount(TRUE rows,
selected rows): count(TRUE) is the numerator and count(non-NULL) the denominator, as for the other
row-level outcomes.  A row that `where` (a predicate over `A`) does not select is NULL.

    referential_integrity   a selected row is TRUE iff all its key columns are non-NULL and B's key
                            state holds the key ("does every orders.customer_id exist in
                            customers.id?").
    dataset_match           a selected row is TRUE iff its key is non-NULL, B holds the key in row j,
                            and every compare pair is NULL-safe equal (a_c[i] <=> b_c[j] as Spark
                            evaluates it: NULL equals NULL only; integers, bool and decimals by
                            value; floats with NaN == NaN and -0.0 == 0.0; strings by bytes).  No key
                            of B may occur in more than one row of B (rows of B with a NULL key
                            column are unreachable and allowed).

Key equality is the group-by's own (deequ_amd/frequencies.py).  Duplicate keys in `A` are fine; rows
of `B` that no row of `A` names are not counted -- swap the arguments for the other direction.

`B`'s keys are grouped by the frequency table (dq_freq_consume); dataset_match then maps every
table slot to the row of `B` holding its key (dq_freq_index_rows) and one pass over `A` probes the
table, follows the map and compares the cells (dq_freq_match_rows).  Nothing falls back to the
host: what the group-by or the predicate compiler declines is declined here with the same error.
"""
from __future__ import annotations

import ctypes
from collections import OrderedDict, namedtuple
from typing import List, Optional, Sequence, Tuple

from . import _lib as L
from .rowlevel import RowLevelResults, _ScanRows, _on_device, bitmap_words
from .states import NumMatchesAndCount
from .table import Column, Table

MatchCounts = namedtuple("MatchCounts", "matched key_null key_absent cells_differ selected")
_OUTCOME = "match"  # the one outcome a MatchResult holds (RowLevelResults keys its bitmaps)


class MatchResult:
    """The outcome of one cross-table check over every row of the primary table."""

    def __init__(self, rows: RowLevelResults, counts: MatchCounts, reference_rows=None):
        self._rows = rows
        self.num_rows = rows.num_rows
        self.counts = counts
        self._reference_rows = reference_rows

    @property
    def state(self) -> Optional[NumMatchesAndCount]:
        """NumMatchesAndCount(TRUE rows, selected rows), or None when no row is selected."""
        if self.counts.selected == 0:
            return None
        return NumMatchesAndCount(self.counts.matched, self.counts.selected)

    @property
    def ratio(self) -> Optional[float]:
        """TRUE rows / selected rows; None when no row is selected (never NaN)."""
        s = self.state
        return None if s is None else s.numMatches / s.count

    def column(self) -> Column:
        """The outcome as a nullable bool Column, device-resident when the primary table is."""
        return self._rows.column(_OUTCOME)

    def to_pylist(self) -> List[Optional[bool]]:
        return self._rows.to_pylist(_OUTCOME)

    def rows(self, which: str = "false"):
        """Ascending int64 indices of the rows whose outcome is "false", "true" or "null"."""
        return self._rows.rows(_OUTCOME, which)

    def failing_rows(self):
        """The selected rows that are not TRUE."""
        return self._rows.rows(_OUTCOME, "false")

    def reference_rows(self):
        """Per row of the primary table, the row of the reference table holding its key, or -1
        (a NULL key, or a key the reference does not hold), whatever `where` says: an int64 tensor,
        kept only on request (`reference_rows=True`)."""
        if self._reference_rows is None:
            raise KeyError("no reference rows were kept: ask with reference_rows=True")
        return self._reference_rows if self._rows.on_device else self._reference_rows.cpu()

    def take(self, primary, which: str = "false", columns=None) -> Table:
        """The rows of `primary` whose outcome is `which`, as a Table in row order."""
        return self._rows.take(primary, _OUTCOME, which, columns)

    def mismatches(self, primary, reference, columns=None, reference_columns=None) -> Tuple[Table, Table]:
        """(a_rows, b_rows), two tables of equal length: the failing rows of `primary` and, row for
        row, the row of `reference` holding that key -- an all-NULL row where no row holds it.  Needs
        the reference rows (`reference_rows=True`)."""
        from .take import take
        if self._reference_rows is None:
            self.reference_rows()  # (raises the KeyError)
        rows = self._rows.rows(_OUTCOME, "false").to(self._reference_rows.device)
        a_rows = self._rows.take(primary, _OUTCOME, "false", columns)
        return a_rows, take(reference, self._reference_rows[rows], reference_columns)


# ---------------------------------------------------------------- argument checks (no device)
def _pairs(items, what: str) -> List[Tuple[str, str]]:
    out = []
    for it in items:
        if isinstance(it, str):
            out.append((it, it))
        elif isinstance(it, (tuple, list)) and len(it) == 2 and all(isinstance(x, str) for x in it):
            out.append((it[0], it[1]))
        else:
            raise ValueError("%s takes column names or (primary, reference) pairs, not %r" % (what, it))
    return out


def _check_pairs(pairs, a_schema, b_schema, what: str) -> None:
    for a, b in pairs:
        if a not in a_schema:
            raise ValueError("%s: the primary table has no column %r" % (what, a))
        if b not in b_schema:
            raise ValueError("%s: the reference table has no column %r" % (what, b))
        if a_schema[a] != b_schema[b]:
            raise ValueError("%s: %s is %s in the primary table and %s is %s in the reference (no coercion: cast "
                             "one side first)" % (what, a, a_schema[a], b, b_schema[b]))


def _check_primary(primary, what: str) -> None:
    from .distributed import is_sharded
    if is_sharded(primary):
        raise L.UnsupportedOnGpu(L.DQ_ERR_UNSUPPORTED, "%s over a ShardedTable: a key's owner is another rank, and "
                                 "the outcome bitmaps are not gathered across ranks" % what)


def _compile_where(where: Optional[str], schema):
    """The OpSpec of `where` as a Compliance over the primary schema (its TRUE plane selects)."""
    if where is None:
        return None
    from .engine import OpSpec, op_supported, schema_index
    from .predicates import compile_predicate
    spec = OpSpec(L.DQ_OP_COMPLIANCE, -1, compile_predicate(where, schema_index(schema)), None)
    op_supported(spec, schema)
    return spec


def _single_batch(reference, what: str):
    from .distributed import is_sharded
    if is_sharded(reference):
        raise L.UnsupportedOnGpu(L.DQ_ERR_UNSUPPORTED, "%s: the reference is a ShardedTable" % what)
    batches = reference.batches()
    if len(batches) != 1:
        raise L.UnsupportedOnGpu(L.DQ_ERR_UNSUPPORTED, "%s: the reference has %d batches; its rows are numbered "
                                 "within one batch (concatenate it first)" % (what, len(batches)))
    return _as_table(batches[0], list(reference.schema))


# ---------------------------------------------------------------- evaluation
def _as_table(batch, names: Sequence[str]) -> Table:
    """The columns `names` of a Table or an ArrowBatch as a Table (host Arrow buffers: zero-copy)."""
    from .arrow import ArrowBatch
    names = list(dict.fromkeys(names))
    if isinstance(batch, ArrowBatch):
        return Table.from_arrow(batch.batch.select(names))
    return Table(OrderedDict((n, batch.columns[n]) for n in names))


def _key_columns(table, a_for_b, batch: Table):
    """dq_columns in the frequency table's column order, `batch`'s key columns in the places of the
    reference's (the table reads its key columns only)."""
    arr = (L.DqColumn * max(1, len(table.names)))()
    for i, n in enumerate(table.names):
        if n in a_for_b:
            arr[i] = batch.columns[a_for_b[n]].to_dq()
    return arr


def _device_columns(batch: Table, names: Sequence[str], device: int):
    """(dq_column array, the device Columns kept alive) of `names`: host columns are uploaded."""
    cols = [batch.columns[n].to_device(device) for n in names]
    arr = (L.DqColumn * max(1, len(cols)))()
    for i, c in enumerate(cols):
        arr[i] = c.to_dq()
    return arr, cols


def _match(primary, table, a_keys, b_keys, compare, reference: Optional[Table], where_spec,
           want_rows: bool) -> MatchResult:
    """One dq_freq_match_rows per batch of `primary` against `table` (the group-by of the reference's
    `b_keys`, indexed when `compare` or `want_rows` follow it into `reference`, a device Table)."""
    import torch
    from .engine import current_device
    device = current_device()
    dev = torch.device("cuda", device)
    schema = primary.schema
    names = list(schema.keys())
    a_for_b = dict(zip(b_keys, a_keys))
    n = primary.count()
    words = max(1, bitmap_words(n))
    value = torch.zeros(words, dtype=torch.int64, device=dev)
    valid = torch.zeros(words, dtype=torch.int64, device=dev)
    ref_rows = torch.full((max(1, n),), -1, dtype=torch.int64, device=dev) if want_rows else None
    follow = bool(compare) or want_rows
    b_rows, b_cmp, b_keep = 0, None, None
    if follow:
        b_rows = reference.num_rows
        b_cmp, b_keep = _device_columns(reference, [b for _, b in compare], device)
    counts = L.DqMatchCounts()
    filter_rows = _ScanRows([where_spec], schema, device) if where_spec is not None else None
    lib = L.lib()
    try:
        offset = 0
        for raw in primary.batches():
            rows = raw.num_rows
            if rows == 0:
                continue
            torch.cuda.synchronize(dev)  # the library works on its own streams: the bitmaps are zeroed, the batch is there
            sel, sel_keep = None, None
            if filter_rows is not None:
                from .rowlevel import _batch_columns
                cols, _, keep = _batch_columns(raw, names)
                bw = bitmap_words(rows)
                sel_keep = (torch.empty(bw, dtype=torch.int64, device=dev), torch.empty(bw, dtype=torch.int64, device=dev))
                filter_rows.evaluate(cols, rows, 0, [sel_keep])
                sel = sel_keep[0].data_ptr()
                del keep
            batch = _as_table(raw, list(a_keys) + [a for a, _ in compare])
            kcols = _key_columns(table, a_for_b, batch)
            a_cmp, a_keep = _device_columns(batch, [a for a, _ in compare], device)
            torch.cuda.synchronize(dev)  # (the uploads)
            L.check(lib.dq_freq_match_rows(table.handle, kcols, len(table.names), rows, sel, offset, value.data_ptr(),
                                           valid.data_ptr(), a_cmp if compare else None, b_cmp if compare else None,
                                           len(compare), b_rows, ref_rows.data_ptr() + 8 * offset if want_rows else None,
                                           ctypes.byref(counts)))
            del a_keep, sel_keep
            offset += rows
    finally:
        if filter_rows is not None:
            filter_rows.close()
    del b_keep
    c = MatchCounts(counts.matched, counts.key_null, counts.key_absent, counts.cells_differ,
                    counts.matched + counts.key_null + counts.key_absent + counts.cells_differ)
    rows_out = RowLevelResults(n, device, _on_device(primary), {_OUTCOME: (value, valid)})
    return MatchResult(rows_out, c, ref_rows[:n] if want_rows else None)


def _reference_table(reference: Table, b_keys: Sequence[str], what: str):
    """(FrequencyTable over the reference's key columns, the reference in HBM)."""
    from .engine import current_device
    from .frequencies import FrequencyTable
    table = FrequencyTable(b_keys, OrderedDict((k, reference.schema[k]) for k in b_keys))
    on_dev = reference.to_device(current_device())
    table.reserve(on_dev.num_rows)
    table.consume(_as_table(on_dev, b_keys))
    return table, on_dev


def _index(table, reference: Table) -> None:
    """dq_freq_index_rows over `reference`, the table's key columns of the rows it was built from."""
    from .table import dq_columns
    cols = dq_columns(reference, table.names)
    L.check(L.lib().dq_freq_index_rows(table.handle, cols, len(table.names), reference.num_rows, 0))


def referential_integrity(primary, columns: Sequence[str], reference=None, reference_columns: Optional[Sequence[str]] = None,
                          where: Optional[str] = None, reference_state=None, reference_rows: bool = False) -> MatchResult:
    """Which rows of `primary` hold, in `columns`, a key that the reference holds in
    `reference_columns` (default: the same names).  The reference is a table (`reference`: one
    batch or several) or the FrequenciesAndNumRows state of its key columns (`reference_state`:
    computed, loaded, or the `State.sum` of several partitions' states); give exactly one.
    `reference_rows=True` also keeps, per row, the reference row holding its key (a single-batch
    `reference` only)."""
    from .decimals import reject_decimal
    from .frequencies import FrequenciesAndNumRows
    what = "referential_integrity"
    if (reference is None) == (reference_state is None):
        raise ValueError("%s takes exactly one of `reference` and `reference_state`" % what)
    if isinstance(columns, str):
        columns = [columns]
    a_keys = list(columns)
    if not a_keys:
        raise ValueError("%s needs at least one key column" % what)
    _check_primary(primary, what)
    a_schema = primary.schema
    if reference_state is not None:
        if not isinstance(reference_state, FrequenciesAndNumRows):
            raise L.UnsupportedOnGpu(L.DQ_ERR_UNSUPPORTED, "%s probes a FrequenciesAndNumRows state held on this GPU, not "
                                     "a %s (a sharded state's keys are owned by other ranks)"
                                     % (what, type(reference_state).__name__))
        if reference_rows:
            raise ValueError("%s: a state holds keys, not rows: reference_rows needs `reference`" % what)
        table = reference_state.table
        if table.histogram:
            raise L.DeequAmdError(L.DQ_ERR_INVALID, "%s cannot probe a Histogram state: it groups NULLs "
                                  "(DQ_FREQ_NULL_AS_KEY), so \"the state holds the key\" is not a join's condition"
                                  % what)
        b_keys = list(reference_columns) if reference_columns is not None else list(table.key_columns)
        if b_keys != list(table.key_columns):
            raise ValueError("%s: the state groups %s, not %s" % (what, table.key_columns, b_keys))
        b_schema = dict(zip(table.key_columns, table.dtypes))
    else:
        b_keys = list(reference_columns) if reference_columns is not None else list(a_keys)
        b_schema = reference.schema
    if len(b_keys) != len(a_keys):
        raise ValueError("%s: %d key columns against %d reference columns" % (what, len(a_keys), len(b_keys)))
    _check_pairs(list(zip(a_keys, b_keys)), a_schema, b_schema, what)
    reject_decimal(a_schema, a_keys, what)
    where_spec = _compile_where(where, a_schema)
    if reference_state is not None:
        return _match(primary, reference_state.table, a_keys, b_keys, [], None, where_spec, False)
    from .distributed import is_sharded
    if is_sharded(reference):
        raise L.UnsupportedOnGpu(L.DQ_ERR_UNSUPPORTED, "%s: the reference is a ShardedTable" % what)
    if reference_rows:
        ref = _single_batch(reference, what + " with reference_rows")
        table, on_dev = _reference_table(ref, b_keys, what)
        _index(table, _as_table(on_dev, b_keys))
        return _match(primary, table, a_keys, b_keys, [], on_dev, where_spec, True)
    from .frequencies import compute_frequencies
    state = compute_frequencies(_KeysOnly(reference, b_keys), b_keys)
    return _match(primary, state.table, a_keys, b_keys, [], None, where_spec, False)


class _KeysOnly:
    """A table's batches narrowed to some columns (the group-by's schema is then those alone)."""

    def __init__(self, data, names: Sequence[str]):
        self._data, self._names = data, list(names)
        self.schema = OrderedDict((n, data.schema[n]) for n in self._names)

    def batches(self):
        return [_as_table(b, self._names) for b in self._data.batches()]

    def count(self) -> int:
        return self._data.count()


def dataset_match(primary, reference, keys: Sequence, compare: Sequence = (), where: Optional[str] = None,
                  reference_rows: bool = False) -> MatchResult:
    """Which rows of `primary` agree with `reference`: the row's key (`keys`: names, or (primary,
    reference) pairs) is in exactly one reference row, and every `compare` pair of cells is
    NULL-safe equal.  `reference` is one batch (a Table, or a one-batch PartitionedTable /
    ArrowTable); a host one is uploaded.  ValueError when a key occurs in more than one reference
    row."""
    from .decimals import reject_decimal
    what = "dataset_match"
    if isinstance(keys, str):
        keys = [keys]
    if isinstance(compare, str):
        compare = [compare]
    key_pairs = _pairs(keys, what + " keys")
    cmp_pairs = _pairs(compare, what + " compare")
    if not key_pairs:
        raise ValueError("%s needs at least one key column" % what)
    if len(cmp_pairs) > 32:
        raise L.UnsupportedOnGpu(L.DQ_ERR_UNSUPPORTED, "%s: more than 32 compare pairs" % what)
    _check_primary(primary, what)
    from .distributed import is_sharded
    if is_sharded(reference):
        raise L.UnsupportedOnGpu(L.DQ_ERR_UNSUPPORTED, "%s: the reference is a ShardedTable" % what)
    a_schema, b_schema = primary.schema, reference.schema
    _check_pairs(key_pairs, a_schema, b_schema, what + " keys")
    _check_pairs(cmp_pairs, a_schema, b_schema, what + " compare")
    a_keys, b_keys = [a for a, _ in key_pairs], [b for _, b in key_pairs]
    reject_decimal(a_schema, a_keys, what)
    where_spec = _compile_where(where, a_schema)
    ref = _single_batch(reference, what)
    table, on_dev = _reference_table(ref, b_keys, what)
    s = table.summary()
    if s.num_groups != s.num_unique:
        raise ValueError("%s: %d keys of the reference occur in more than one of its rows (a match needs one row "
                         "per key: deduplicate the reference, or ask referential_integrity)"
                         % (what, s.num_groups - s.num_unique))
    _index(table, _as_table(on_dev, b_keys))
    return _match(primary, table, a_keys, b_keys, cmp_pairs, on_dev, where_spec, reference_rows)


__all__ = ["MatchCounts", "MatchResult", "referential_integrity", "dataset_match"]
