"""correlation_matrix: every pairwise Correlation state of a column list from one pass over the rows.

`Correlation(x, y, where)` runs one task per pair and each task reads both of its columns again, so
a plan of all pairs of k columns streams every column k times.  `correlation_matrix` reads each
column once per batch and forms the k (k + 1) / 2 pairwise-complete sums as rank-4 updates on the
fp64 matrix cores (dq_corrmat_*, include/deequ_amd.h; deequ_amd/csrc/dq_corrmat.hip).  The states
are ordinary CorrelationStates: a row counts for (x, y) when x and y are non-NULL and `where` is
TRUE, values are cast to double as Correlation casts them, and the states merge, persist and turn
into metrics exactly as the analyzer's own.

A pair that the matrix sums cannot answer for a batch (a selected non-finite value in one of its
columns, sums that are not finite, a shift that is an outlier) takes that batch's state from the
pair kernel Correlation itself runs; `fallback_pairs` counts those pair-batches.
"""
from __future__ import annotations

import ctypes
from typing import Dict, Optional, Sequence, Tuple

import numpy as np

from . import _lib as L
from .analyzers import Correlation
from .states import CorrelationState

MAX_COLUMNS = 64


def pair_index(i: int, j: int, k: int) -> int:
    """Where the pair (i, j), i <= j < k, lies in the row-major upper triangle."""
    return i * k - i * (i - 1) // 2 + (j - i)


def _swapped(s: CorrelationState) -> CorrelationState:
    return CorrelationState(s.n, s.yAvg, s.xAvg, s.ck, s.yMk, s.xMk)


class CorrelationMatrix:
    """The states of one `correlation_matrix` call."""

    def __init__(self, columns: Sequence[str], where: Optional[str], states: np.ndarray, fallback_pairs: int):
        self.columns: Tuple[str, ...] = tuple(columns)
        self.where = where
        self.fallback_pairs = int(fallback_pairs)
        self._index = {c: i for i, c in enumerate(self.columns)}
        self._states = states  # (pairs, 6) float64: n, xAvg, yAvg, ck, xMk, yMk

    def _at(self, x: str, y: str) -> Tuple[int, int]:
        try:
            return self._index[x], self._index[y]
        except KeyError as e:
            raise KeyError("column %s is not in this matrix %s" % (e.args[0], list(self.columns))) from None

    def state(self, x: str, y: str) -> Optional[CorrelationState]:
        """The CorrelationState of Correlation(x, y, where), None when no row has both."""
        i, j = self._at(x, y)
        row = self._states[pair_index(min(i, j), max(i, j), len(self.columns))]
        if row[0] == 0.0:
            return None
        s = CorrelationState(*[float(v) for v in row])
        return s if i <= j else _swapped(s)

    def states(self) -> Dict[Correlation, Optional[CorrelationState]]:
        """{Correlation(x, y, where): state} for i <= j in `columns` order."""
        return {Correlation(x, y, self.where): self.state(x, y)
                for i, x in enumerate(self.columns) for y in self.columns[i:]}

    def metric(self, x: str, y: str):
        """The DoubleMetric Correlation(x, y, where) computes from its state."""
        return Correlation(x, y, self.where).computeMetricFrom(self.state(x, y))

    def matrix(self) -> np.ndarray:
        """k x k metric values; NaN where the analyzer's metric is NaN or has no value."""
        k = len(self.columns)
        out = np.full((k, k), np.nan)
        for i, x in enumerate(self.columns):
            for j in range(i, k):
                s = self.state(x, self.columns[j])
                if s is not None:
                    out[i, j] = out[j, i] = s.metricValue()
        return out

    def counts(self) -> np.ndarray:
        """k x k: the rows that count for each pair."""
        k = len(self.columns)
        out = np.zeros((k, k))
        for i in range(k):
            for j in range(i, k):
                out[i, j] = out[j, i] = self._states[pair_index(i, j, k)][0]
        return out


class _Corrmat:
    """Owns a dq_corrmat over one schema."""

    def __init__(self, schema: Dict[str, str], columns: Sequence[str], where, device: int):
        from .engine import _fill_pred, _pred_array
        self.names = list(schema.keys())
        self.k = len(columns)
        types = (ctypes.c_int32 * len(self.names))(*[L.TYPE_CODES[schema[n]] for n in self.names])
        sel = (ctypes.c_int32 * self.k)(*[self.names.index(c) for c in columns])
        self._where = _pred_array(where)  # (keeps the arrays alive)
        pred = None
        if self._where is not None:
            pred = L.DqPredicate()
            _fill_pred(pred, self._where)
        h = ctypes.c_void_p()
        L.check(L.lib().dq_corrmat_create(L.Context.get(device).handle, types, len(self.names), sel, self.k,
                                          ctypes.byref(pred) if pred is not None else None, ctypes.byref(h)))
        self.handle = h

    def reset(self) -> None:
        L.check(L.lib().dq_corrmat_reset(self.handle))

    def consume(self, cols, n_rows: int) -> None:
        L.check(L.lib().dq_corrmat_consume(self.handle, cols, len(self.names), n_rows))

    def finish(self) -> Tuple[np.ndarray, int]:
        states = np.zeros((self.k * (self.k + 1) // 2, 6), dtype=np.float64)
        fb = ctypes.c_int64(0)
        L.check(L.lib().dq_corrmat_finish(self.handle, states.ctypes.data, ctypes.byref(fb)))
        return states, fb.value

    def close(self) -> None:
        if getattr(self, "handle", None):
            L.lib().dq_corrmat_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 - interpreter shutdown
            pass


def check_columns(schema: Dict[str, str], columns: Sequence[str]) -> None:
    """The preconditions of `correlation_matrix`: Correlation's own per column, a non-empty list
    without repeats, and at most MAX_COLUMNS columns."""
    columns = list(columns)
    if not columns:
        raise ValueError("correlation_matrix needs at least one column")
    if len(set(columns)) != len(columns):
        raise ValueError("correlation_matrix: column %s is listed twice"
                         % next(c for i, c in enumerate(columns) if c in columns[:i]))
    for c in columns:
        for cond in Correlation(c, c).additionalPreconditions():
            cond(schema)
    if len(columns) > MAX_COLUMNS:
        raise L.UnsupportedOnGpu(L.DQ_ERR_UNSUPPORTED, "correlation_matrix of %d columns: one matrix holds at most %d "
                                 "(cut the columns into blocks and take the cross pairs from Correlation)"
                                 % (len(columns), MAX_COLUMNS))


def correlation_matrix(data, columns: Sequence[str], where: Optional[str] = None) -> CorrelationMatrix:
    """Every CorrelationState of Correlation(x, y, where) for x, y in `columns` over `data` (a Table,
    PartitionedTable or ArrowTable, on the host or in HBM), each column read once per batch."""
    import torch
    from .decimals import float64_view
    from .distributed import is_sharded
    from .engine import current_device, schema_index
    from .predicates import compile_predicate
    from .rowlevel import _batch_columns
    columns = list(columns)
    if is_sharded(data):
        raise L.UnsupportedOnGpu(L.DQ_ERR_UNSUPPORTED, "correlation_matrix over a ShardedTable: the matrix runs on "
                                 "single-device tables, and its states are not merged across ranks (merge the ranks' "
                                 "matrices pair by pair with State.sum)")
    check_columns(data.schema, columns)
    if where:  # the filter is typed against the real schema (a decimal column is cast below)
        compile_predicate(where, schema_index(data.schema))
    view = float64_view(data, columns)
    schema = view.schema
    program = compile_predicate(where, schema_index(schema)) if where else None
    device = current_device()
    dev = torch.device("cuda", device)
    names = list(schema.keys())
    run = _Corrmat(schema, columns, program, device)
    try:
        for batch in view.batches():
            if batch.num_rows == 0:
                continue
            torch.cuda.synchronize(dev)  # the library reads the buffers on its own stream
            cols, rows, keep = _batch_columns(batch, names)
            run.consume(cols, rows)
            del keep
        states, fallback = run.finish()
    finally:
        run.close()
    return CorrelationMatrix(columns, where, states, fallback)


__all__ = ["CorrelationMatrix", "correlation_matrix", "pair_index", "MAX_COLUMNS"]
