"""ApproxQuantile / ApproxQuantiles' runner over the C-ABI's dq_aq_* family.

Every quantile analyzer of a run shares one sketcher: one kernel launch per pass and batch covers
all their (column, relativeError) pairs, and analyzers that differ only in their quantiles share a
digest.  The digest is this backend's own (ApproxQuantile): per batch the exact values at
ranks 1, 1 + gap, ..., n from a multi-rank radix select on the GPU, merged on the host in arrival
order.
"""
from __future__ import annotations

import ctypes
from typing import Dict, List, Optional, Sequence, Tuple

from . import _lib as L
from .states import ApproxQuantileState, PercentileDigest


def check_parameters(relativeError: float) -> None:
    """Raises UnsupportedOnGpu (the message names the bound) for a relativeError the GPU select does
    not serve: 0 (an exact quantile needs a full sort) and values below 0.001."""
    L.check(L.lib().dq_aq_supported(float(relativeError)))


class QuantileSketcher:
    """Owns a dq_aq for (column, relativeError) pairs over a fixed schema."""

    def __init__(self, schema: Dict[str, str], columns: Sequence[Tuple[str, float]], device: Optional[int] = None):
        from .engine import current_device
        self.device = current_device() if device is None else device
        self.ctx = L.Context.get(self.device)
        self.names = list(schema.keys())
        self.columns = [(c, float(e)) for c, e in columns]
        cols = (L.DqAqColumn * max(1, len(self.columns)))()
        for i, (c, e) in enumerate(self.columns):
            cols[i].column, cols[i].relative_error = self.names.index(c), e
        types = (ctypes.c_int32 * max(1, len(self.names)))(*[L.TYPE_CODES[schema[n]] for n in self.names])
        h = ctypes.c_void_p()
        L.check(L.lib().dq_aq_create(self.ctx.handle, cols, len(self.columns), types, len(self.names), ctypes.byref(h)))
        self.handle = h

    def consume(self, batch) -> None:
        from .arrow import ArrowBatch, arrow_columns
        from .table import dq_columns
        if isinstance(batch, ArrowBatch):
            _, cols, rows, _keep = arrow_columns(batch, self.names)
            arr = (L.DqColumn * max(1, len(cols)))(*cols)
            L.check(L.lib().dq_aq_consume(self.handle, arr, len(cols), rows))
            return
        cols = dq_columns(batch, self.names)
        if L.device_inputs(batch.columns[n] for n in self.names):
            L.after_current_stream(self.device)  # the library's launches wait for no torch stream: the batch is there
        L.check(L.lib().dq_aq_consume(self.handle, cols, len(self.names), batch.num_rows))

    def finish(self) -> List[ApproxQuantileState]:
        n = len(self.columns)
        sizes = (ctypes.c_int64 * max(1, n))()
        L.check(L.lib().dq_aq_finish(self.handle, sizes, n))
        out = []
        for i in range(n):
            buf = ctypes.create_string_buffer(max(8, sizes[i]))
            need = ctypes.c_int64()
            L.check(L.lib().dq_aq_export(self.handle, i, buf, sizes[i], ctypes.byref(need)))
            out.append(ApproxQuantileState(PercentileDigest.deserialize(buf.raw[:need.value])))
        return out

    def close(self) -> None:
        if getattr(self, "handle", None):
            L.lib().dq_aq_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 - interpreter shutdown
            pass


def compute_quantile_states(data, analyzers: Sequence) -> Dict[object, ApproxQuantileState]:
    """One pass over every batch of `data` for all quantile analyzers: distinct (column,
    relativeError) pairs are computed once each and shared (ApproxQuantileState.sum never mutates
    an operand)."""
    from .distributed import is_sharded
    if is_sharded(data):
        raise L.UnsupportedOnGpu(L.DQ_ERR_UNSUPPORTED, "ApproxQuantile over a ShardedTable: the ranks' target "
                                 "ranks are not gathered across ranks")
    # a decimal column is cast to double first, as Spark casts the digest's input (decimals.py)
    from .decimals import float64_view
    data = float64_view(data, [a.column for a in analyzers])
    keys, index = [], {}
    for a in analyzers:
        key = (a.column, float(a.relativeError))
        if key not in index:
            index[key] = len(keys)
            keys.append(key)
    sk = QuantileSketcher(data.schema, keys)
    try:
        for batch in data.batches():
            sk.consume(batch)
        states = sk.finish()
    finally:
        sk.close()
    return {a: states[index[(a.column, float(a.relativeError))]] for a in analyzers}


__all__ = ["QuantileSketcher", "check_parameters", "compute_quantile_states"]
