"""KLLSketch's runner: the reference's KLLRunner.computeKLLSketchesInExtraPass (KLLRunner.scala:
89-122) over the C-ABI's dq_kll_* family.

Every KLL analyzer of a run shares one sketcher: one kernel launch per batch covers all their
columns.  The reference's result depends on Spark's partitioning; this backend fixes one (DESIGN.md,
KLLSketch): slabs of `slab_rows` consecutive rows, a balanced tree merge per batch, batches in arrival
order.  `slab_rows` is the library's constant unless overridden -- per sketcher, or for a block of
code with `with kll.slab_rows(n):` (what the runner and the profiler then pick up).
"""
from __future__ import annotations

import contextlib
import contextvars
import ctypes
from typing import Dict, List, Optional, Sequence, Tuple

from . import _lib as L
from .states import KLLState

_SLAB_ROWS: "contextvars.ContextVar[Optional[int]]" = contextvars.ContextVar("deequ_amd_kll_slab_rows", default=None)


@contextlib.contextmanager
def slab_rows(n: Optional[int]):
    """Rows per slab of the sketchers created inside the block (None: the library's constant)."""
    token = _SLAB_ROWS.set(None if n is None else int(n))
    try:
        yield
    finally:
        _SLAB_ROWS.reset(token)


def check_parameters(sketchSize: int, shrinkingFactor: float) -> None:
    """Raises UnsupportedOnGpu (the message names the bound) for parameters whose levels do not
    fit the kernels' LDS budget, e.g. sketchSize 50000 or a shrinking factor >= 1."""
    L.check(L.lib().dq_kll_supported(int(sketchSize), float(shrinkingFactor)))


def check_column(schema: Dict[str, str], column: str) -> None:
    """KLLRunner.scala:135-144 matches the column's type after isNumeric passed: a DecimalType column
    reaches `case _ => throw new IllegalArgumentException(s"Cannot handle ${...dataType}")`."""
    if L.is_decimal(schema.get(column)):
        from .decimals import spark_type_name
        raise ValueError("Cannot handle %s" % spark_type_name(schema[column]))


class KLLSketcher:
    """Owns a dq_kll for (column, sketchSize, shrinkingFactor) triples over a fixed schema."""

    def __init__(self, schema: Dict[str, str], columns: Sequence[Tuple[str, int, float]],
                 slab_rows: Optional[int] = None, device: Optional[int] = None):
        from .engine import current_device
        self.device = current_device() if device is None else device
        self.ctx = L.Context.get(self.device)
        self.names = list(schema.keys())
        self.columns = [(c, int(k), float(f)) for c, k, f in columns]
        if slab_rows is None:
            slab_rows = _SLAB_ROWS.get()
        self.slab_rows = 0 if slab_rows is None else int(slab_rows)
        cols = (L.DqKllColumn * max(1, len(self.columns)))()
        for i, (c, k, f) in enumerate(self.columns):
            cols[i].column, cols[i].sketch_size, cols[i].shrinking_factor = self.names.index(c), k, f
        types = (ctypes.c_int32 * max(1, len(self.names)))(*[L.TYPE_CODES[schema[n]] for n in self.names])
        h = ctypes.c_void_p()
        L.check(L.lib().dq_kll_create(self.ctx.handle, cols, len(self.columns), types, len(self.names),
                                      self.slab_rows, ctypes.byref(h)))
        self.handle = h

    def consume(self, batch) -> None:
        from .arrow import ArrowBatch, arrow_columns
        from .table import dq_columns
        if isinstance(batch, ArrowBatch):
            _, cols, rows, _keep = arrow_columns(batch, self.names)
            arr = (L.DqColumn * max(1, len(cols)))(*cols)
            L.check(L.lib().dq_kll_consume(self.handle, arr, len(cols), rows))
            return
        cols = dq_columns(batch, self.names)
        if L.device_inputs(batch.columns[n] for n in self.names):
            L.after_current_stream(self.device)  # the library's launches wait for no torch stream: the batch is there
        L.check(L.lib().dq_kll_consume(self.handle, cols, len(self.names), batch.num_rows))

    def finish(self) -> List[KLLState]:
        n = len(self.columns)
        sizes = (ctypes.c_int64 * max(1, n))()
        L.check(L.lib().dq_kll_finish(self.handle, sizes, n))
        out = []
        for i, (_, k, f) in enumerate(self.columns):
            buf = ctypes.create_string_buffer(max(8, sizes[i]))
            need = ctypes.c_int64()
            L.check(L.lib().dq_kll_export(self.handle, i, buf, sizes[i], ctypes.byref(need)))
            out.append(KLLState.from_export(buf.raw[:need.value], k, f))
        return out

    def close(self) -> None:
        if getattr(self, "handle", None):
            L.lib().dq_kll_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 - interpreter shutdown
            pass


def compute_kll_states(data, analyzers: Sequence, slab_rows: Optional[int] = None) -> Dict[object, KLLState]:
    """One sketching pass over every batch of `data` for all KLL analyzers (the reference sketches
    a column once per run however many analyzers name it: columnsAndParameters is a Map,
    KLLRunner.scala:98-100 -- here distinct (column, parameters) are sketched once each)."""
    from .distributed import is_sharded
    if is_sharded(data):
        raise L.UnsupportedOnGpu(L.DQ_ERR_UNSUPPORTED, "KLLSketch over a ShardedTable: KLL states are not gathered "
                                 "across ranks")
    keys, index = [], {}
    for a in analyzers:
        check_column(data.schema, a.column)
        key = (a.column, a.sketchSize, a.shrinkingFactor)
        if key not in index:
            index[key] = len(keys)
            keys.append(key)
    sk = KLLSketcher(data.schema, keys, slab_rows)
    try:
        for batch in data.batches():
            sk.consume(batch)
        states = sk.finish()
    finally:
        sk.close()
    # (analyzers that differ only in numberOfBuckets share a state: KLLState.sum never mutates one)
    return {a: (states[index[(a.column, a.sketchSize, a.shrinkingFactor)]]) for a in analyzers}


__all__ = ["KLLSketcher", "check_parameters", "compute_kll_states", "slab_rows"]
