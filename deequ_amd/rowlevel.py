"""Row-level outcomes: which rows an analyzer counts, on the GPU.

Every supported analyzer over `data` yields one nullable boolean per row, tied to the analyzer's
state by two invariants: count(TRUE) is the state's numerator and count(non-NULL) its denominator.
A row that the analyzer's `where` does not select (FALSE or NULL) is NULL; a selected row is TRUE

    Completeness(c)       where c is not NULL,
    Compliance(_, p)      where p is TRUE (a NULL p is FALSE, as Compliance.scala sums it),
    PatternMatch(c, re)   where the scan's PatternMatch counts it (a NULL value is FALSE),
    Uniqueness(cols)      where the row's key has count exactly 1 in the FrequenciesAndNumRows state
                          probed (a NULL key column and a key the state does not hold are FALSE).

Uniqueness probes the state computed from `data` (the group-by pass, then the probe pass) unless
`states` hands it another one -- a loaded state, or the `State.sum` of several partitions' states:
"unique within the union".  Every other analyzer has no per-row meaning and raises ValueError.

An outcome is two bitmaps in the Arrow boolean layout (LSB first, padded to 64-bit words) over the
whole table: every batch is written at its row offset (dq_rows_evaluate, dq_freq_probe_rows,
include/deequ_amd.h).  They stay in HBM; `column()` hands them out as a bool Column, device-resident
when the data is, and `failing_rows()` compacts the rows of one outcome into ascending int64
indices on the device (dq_rows_select).
"""
from __future__ import annotations

import ctypes
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib as L
from .analyzers import Completeness, Compliance, PatternMatch, Uniqueness
from .table import Column, dq_columns

_SCAN = (Completeness, Compliance, PatternMatch)
_WHICH = {"false": L.DQ_ROWS_FALSE, "true": L.DQ_ROWS_TRUE, "null": L.DQ_ROWS_NULL}


# ---------------------------------------------------------------- bitmap layout
def bitmap_words(n_rows: int) -> int:
    """64-bit words of a bitmap over n_rows rows (Arrow boolean layout padded to 8 bytes)."""
    return (int(n_rows) + 63) // 64


def pack_bits(bits: Sequence[bool]) -> np.ndarray:
    """Booleans -> uint64 words, LSB first, the trailing bits of the last word 0."""
    b = np.asarray(bits, dtype=bool)
    padded = np.zeros(bitmap_words(len(b)) * 64, dtype=bool)
    padded[:len(b)] = b
    return np.packbits(padded, bitorder="little").view("<u8")


def unpack_bits(words, n_rows: int) -> np.ndarray:
    """The first n_rows bits of uint64 / int64 words (or their bytes) as booleans."""
    raw = np.ascontiguousarray(words).view(np.uint8)
    return np.unpackbits(raw, bitorder="little")[:n_rows].astype(bool)


def outcomes_from_bitmaps(value, valid, n_rows: int) -> List[Optional[bool]]:
    """[True | False | None] per row of a (value, valid) bitmap pair."""
    t, v = unpack_bits(value, n_rows), unpack_bits(valid, n_rows)
    return [None if not ok else bool(x) for x, ok in zip(t.tolist(), v.tolist())]


# ---------------------------------------------------------------- results
class RowLevelResults:
    """The outcome bitmaps of one `row_level_results` call, keyed by analyzer."""

    def __init__(self, num_rows: int, device: int, on_device: bool, bitmaps: Dict[object, tuple],
                 key_counts: Optional[Dict[object, object]] = None):
        self.num_rows = int(num_rows)
        self.device = device
        self.on_device = on_device
        self._bitmaps = bitmaps  # analyzer -> (value words, valid words): int64 tensors in HBM
        self._key_counts = key_counts or {}
        self._counts: Dict[tuple, int] = {}

    @property
    def analyzers(self) -> List:
        return list(self._bitmaps)

    def _pair(self, analyzer):
        try:
            return self._bitmaps[analyzer]
        except KeyError:
            raise KeyError("no row-level outcome was computed for %s" % (analyzer,)) from None

    def column(self, analyzer) -> Column:
        """The outcome as a nullable bool Column (values = TRUE bits, validity = non-NULL bits):
        torch tensors in HBM when the data is device-resident, numpy arrays otherwise."""
        import torch
        value, valid = self._pair(analyzer)
        vb, nb = value.view(torch.uint8), valid.view(torch.uint8)
        if self.on_device:
            return Column("bool", self.num_rows, vb, nb, device=True)
        return Column("bool", self.num_rows, vb.cpu().numpy(), nb.cpu().numpy())

    def to_pylist(self, analyzer) -> List[Optional[bool]]:
        """[True | False | None] per row (host objects: small results, tests)."""
        value, valid = self._pair(analyzer)
        return outcomes_from_bitmaps(value.cpu().numpy(), valid.cpu().numpy(), self.num_rows)

    def _select(self, analyzer, which: int, out, capacity: int) -> Tuple[int, int]:
        value, valid = self._pair(analyzer)
        n = ctypes.c_int64()
        st = L.lib().dq_rows_select(L.Context.get(self.device).handle, value.data_ptr(), valid.data_ptr(),
                                    self.num_rows, which, out, capacity, ctypes.byref(n))
        return st, n.value

    def _count(self, analyzer, which: int) -> int:
        key = (analyzer, which)
        if key not in self._counts:
            st, n = self._select(analyzer, which, None, 0)
            if st != L.DQ_ERR_SPACE:
                L.check(st)
            self._counts[key] = n
        return self._counts[key]

    def counts(self, analyzer) -> Tuple[int, int, int]:
        """(rows TRUE, rows FALSE, rows NULL)."""
        t, f = self._count(analyzer, L.DQ_ROWS_TRUE), self._count(analyzer, L.DQ_ROWS_FALSE)
        return t, f, self.num_rows - t - f

    def rows(self, analyzer, which: str = "false"):
        """The ascending int64 indices of the rows whose outcome is `which` ("false", "true" or
        "null"): a tensor in HBM when the data is device-resident, on the host otherwise."""
        import torch
        w = _WHICH[which]
        n = self._count(analyzer, w)
        out = torch.empty(max(1, n), dtype=torch.int64, device=torch.device("cuda", self.device))
        if n:
            st, _ = self._select(analyzer, w, out.data_ptr(), n)
            L.check(st)
        out = out[:n]
        return out if self.on_device else out.cpu()

    def key_counts(self, analyzer):
        """Per row, the count of its key in the state a Uniqueness probed (0: a NULL key column, or
        a key the state does not hold), whatever the `where` says: an int64 tensor, kept only by
        `row_level_results(..., key_counts=True)`."""
        try:
            out = self._key_counts[analyzer]
        except KeyError:
            raise KeyError("no key counts were kept for %s" % (analyzer,)) from None
        return out if self.on_device else out.cpu()

    def failing_rows(self, analyzer):
        """The ascending indices of the rows the analyzer selects and does not count (FALSE)."""
        return self.rows(analyzer, "false")

    def _check_data(self, data, what: str) -> None:
        if data.count() != self.num_rows:
            raise ValueError("%s: the outcomes cover %d rows, the table has %d (hand in the data they were computed "
                             "over)" % (what, self.num_rows, data.count()))

    def take(self, data, analyzer, which: str = "false", columns=None):
        """The rows of `data` (the table the outcomes were computed over) whose outcome of
        `analyzer` is `which`, as a Table in row order (deequ_amd/take.py): by default the failing
        records themselves."""
        from .take import take
        self._pair(analyzer)
        if which not in _WHICH:
            raise ValueError("which is \"false\", \"true\" or \"null\", not %r" % (which,))
        self._check_data(data, "RowLevelResults.take")
        return take(data, self.rows(analyzer, which), columns)

    def split(self, data, analyzers=None, columns=None):
        """(passing, failing): `failing` holds the rows that are FALSE for at least one of
        `analyzers` (default: all of them), `passing` every other row -- a NULL outcome passes: a row
        its `where` does not select is not a failure.  Both keep the input order, and their row
        counts sum to num_rows.  The FALSE planes are OR-ed as 64-bit words in HBM and the two row
        lists selected by dq_rows_select."""
        import torch
        from .take import take
        analyzers = self.analyzers if analyzers is None else list(analyzers)
        self._check_data(data, "RowLevelResults.split")
        dev = torch.device("cuda", self.device)
        words = max(1, bitmap_words(self.num_rows))
        failing = torch.zeros(words, dtype=torch.int64, device=dev)
        for a in analyzers:
            value, valid = self._pair(a)
            failing |= ~value & valid
        ones = torch.full((words,), -1, dtype=torch.int64, device=dev)
        torch.cuda.synchronize(dev)
        both = RowLevelResults(self.num_rows, self.device, True, {"failing": (failing, ones)})
        return (take(data, both.rows("failing", "false"), columns), take(data, both.rows("failing", "true"), columns))


# ---------------------------------------------------------------- evaluation
class _ScanRows:
    """Owns a dq_rows for a list of Completeness / Compliance / PatternMatch ops over one schema."""

    def __init__(self, specs, schema: Dict[str, str], device: int):
        self.names = list(schema.keys())
        self.specs = list(specs)  # (keeps the predicate arrays alive)
        ops = (L.DqOp * len(self.specs))()
        for i, s in enumerate(self.specs):
            s.fill(ops[i])
        types = (ctypes.c_int32 * len(self.names))(*[L.TYPE_CODES[schema[n]] for n in self.names])
        h = ctypes.c_void_p()
        L.check(L.lib().dq_rows_create(L.Context.get(device).handle, ops, len(self.specs), types, len(self.names),
                                       ctypes.byref(h)))
        self.handle = h

    def evaluate(self, cols, n_rows: int, bit_offset: int, pairs) -> None:
        value = (ctypes.c_void_p * len(pairs))(*[p[0].data_ptr() for p in pairs])
        valid = (ctypes.c_void_p * len(pairs))(*[p[1].data_ptr() for p in pairs])
        L.check(L.lib().dq_rows_evaluate(self.handle, cols, len(self.names), n_rows, bit_offset, value, valid))

    def close(self) -> None:
        if getattr(self, "handle", None):
            L.lib().dq_rows_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 - interpreter shutdown
            pass


def _batch_columns(batch, names: Sequence[str]):
    """(dq_column array, rows, what keeps the buffers alive) of a Table or an ArrowBatch."""
    from .arrow import ArrowBatch, arrow_columns
    if isinstance(batch, ArrowBatch):
        _, cols, rows, keep = arrow_columns(batch, names)
        return (L.DqColumn * max(1, len(cols)))(*cols), rows, keep
    return dq_columns(batch, names), batch.num_rows, batch


def _on_device(data) -> bool:
    from .table import Table
    batches = data.batches()
    return bool(batches) and all(isinstance(b, Table) and all(c.device for c in b.columns.values()) for b in batches)


def _check_supported(analyzer) -> None:
    if type(analyzer) not in _SCAN + (Uniqueness,):
        raise ValueError("%s has no row-level outcome: only Completeness, Compliance, PatternMatch and Uniqueness "
                         "say something about a single row" % type(analyzer).__name__)


def _probe_state(analyzer, data, states):
    """The FrequenciesAndNumRows state a Uniqueness probes: the caller's, or the one of `data`."""
    from .frequencies import FrequenciesAndNumRows
    state = None
    if states is not None:
        state = states.load(analyzer) if hasattr(states, "load") else states.get(analyzer)
    if state is None:
        return analyzer.computeStateFrom(data)
    if not isinstance(state, FrequenciesAndNumRows):
        raise L.UnsupportedOnGpu(L.DQ_ERR_UNSUPPORTED, "row-level Uniqueness probes a FrequenciesAndNumRows state held "
                                 "on this GPU, not a %s (a sharded state's keys are owned by other ranks)"
                                 % type(state).__name__)
    if state.table.histogram:
        raise L.DeequAmdError(L.DQ_ERR_INVALID, "row-level Uniqueness cannot probe a Histogram state: it groups NULLs "
                              "(DQ_FREQ_NULL_AS_KEY), so \"count == 1\" there is not Uniqueness's outcome")
    if list(state.table.key_columns) != list(analyzer.columns):
        raise ValueError("the state groups %s, the analyzer %s" % (state.table.key_columns, list(analyzer.columns)))
    return state


def row_level_results(data, analyzers: Sequence, states=None, key_counts: bool = False) -> RowLevelResults:
    """The row-level outcomes of `analyzers` over every batch of `data` (a Table, PartitionedTable or
    ArrowTable, on the host or in HBM).  `states`: {Uniqueness analyzer: FrequenciesAndNumRows} (or a
    StateLoader) to probe instead of the state of `data`; `key_counts` also keeps every row's key
    count of each Uniqueness (RowLevelResults.key_counts).  Whatever the analyzer itself declines
    (a predicate, a pattern, a decimal key) is declined here with the same error."""
    import torch
    from .distributed import is_sharded
    from .engine import OpSpec, current_device, op_spec_for, op_supported, schema_index
    from .predicates import compile_predicate
    analyzers = list(dict.fromkeys(analyzers))
    for a in analyzers:
        _check_supported(a)
    if is_sharded(data):
        raise L.UnsupportedOnGpu(L.DQ_ERR_UNSUPPORTED, "row-level outcomes over a ShardedTable: a key's owner is "
                                 "another rank, and the outcome bitmaps are not gathered across ranks")
    schema = data.schema
    for a in analyzers:
        for cond in a.preconditions():
            cond(schema)
    scans = [a for a in analyzers if type(a) in _SCAN]
    uniques = [a for a in analyzers if type(a) is Uniqueness]
    specs = [op_spec_for(a, schema) for a in scans]
    for s in specs:
        op_supported(s, schema)
    # a filtered Uniqueness selects its rows with the TRUE plane of its `where`: a Compliance outcome
    # of the filter, evaluated per batch at bit 0
    filters = list(dict.fromkeys(a.where for a in uniques if a.where is not None))
    fspecs = [OpSpec(L.DQ_OP_COMPLIANCE, -1, compile_predicate(w, schema_index(schema)), None) for w in filters]
    for s in fspecs:
        op_supported(s, schema)
    probed = [(a, _probe_state(a, data, states)) for a in uniques]  # (pass 1: the group-by)
    for a, st in probed:
        for c, t in zip(st.table.key_columns, st.table.dtypes):
            if schema[c] != t:
                raise ValueError("key column %s is %s in the data and %s in the state" % (c, schema[c], t))

    device = current_device()
    dev = torch.device("cuda", device)
    n = data.count()
    words = max(1, bitmap_words(n))
    bitmaps = {a: (torch.zeros(words, dtype=torch.int64, device=dev), torch.zeros(words, dtype=torch.int64, device=dev))
               for a in analyzers}
    kept = {a: torch.zeros(max(1, n), dtype=torch.int64, device=dev) for a in uniques} if key_counts else {}
    names = list(schema.keys())
    scan_rows = _ScanRows(specs, schema, device) if specs else None
    filter_rows = _ScanRows(fspecs, schema, device) if fspecs else None
    try:
        offset = 0
        for batch in data.batches():
            rows = batch.num_rows
            if rows == 0:
                continue
            torch.cuda.synchronize(dev)  # the library works on its own streams: the bitmaps are zeroed, the batch is there
            cols, _, keep = _batch_columns(batch, names)
            if scan_rows is not None:
                scan_rows.evaluate(cols, rows, offset, [bitmaps[a] for a in scans])
            selected = {}
            if filter_rows is not None:
                bw = bitmap_words(rows)
                pairs = [(torch.empty(bw, dtype=torch.int64, device=dev), torch.empty(bw, dtype=torch.int64, device=dev))
                         for _ in filters]
                filter_rows.evaluate(cols, rows, 0, pairs)
                selected = {w: p[0] for w, p in zip(filters, pairs)}
            for a, st in probed:
                tcols, _, tkeep = _batch_columns(batch, st.table.names)
                sel = selected[a.where].data_ptr() if a.where is not None else None
                value, valid = bitmaps[a]
                L.check(L.lib().dq_freq_probe_rows(st.table.handle, tcols, len(st.table.names), rows, sel, offset,
                                                   value.data_ptr(), valid.data_ptr(),
                                                   kept[a].data_ptr() + 8 * offset if key_counts else None))
                del tkeep
            del keep
            offset += rows
    finally:
        for r in (scan_rows, filter_rows):
            if r is not None:
                r.close()
    return RowLevelResults(n, device, _on_device(data), bitmaps, kept)


__all__ = ["RowLevelResults", "row_level_results", "bitmap_words", "pack_bits", "unpack_bits", "outcomes_from_bitmaps"]
