"""take: the rows of a table named by row indices, as a new Table, on the GPU.

Row-level outcomes and cross-table checks end in row numbers (`failing_rows`, `reference_rows`);
`take` turns them into records without leaving HBM.  `rows` numbers the rows of `data` from 0 over
all its batches, as `RowLevelResults` does; the indices may come in any order and repeat, and -1
means "no row": every column of that output row is NULL (what `reference_rows` holds for a key the
reference lacks).  The indices are validated and mapped to (batch, local row) once (dq_take_create);
every column is then sized (dq_take_layout), allocated here as torch tensors, and gathered
(dq_take_gather) -- values, validity and utf8 offsets in the Arrow layout at offset 0, honouring the
source columns' slices.  Nothing falls back to the host.
"""
from __future__ import annotations

import ctypes
from collections import OrderedDict
from typing import Optional, Sequence

import numpy as np

from . import _lib as L
from .table import Column, Table

_TORCH = {"int8": "int8", "int16": "int16", "int32": "int32", "int64": "int64", "float32": "float32",
          "float64": "float64"}


def _device_rows(rows, dev):
    """`rows` as a contiguous 1-D int64 tensor in HBM."""
    import torch
    if isinstance(rows, torch.Tensor):
        if rows.dtype != torch.int64 or rows.dim() != 1:
            raise ValueError("take: rows is a 1-D int64 tensor, not %s of %d dimensions" % (rows.dtype, rows.dim()))
        return rows.to(dev).contiguous()
    arr = np.asarray(rows)
    if arr.size and arr.dtype.kind not in "iu":
        raise ValueError("take: rows holds integers, not %s" % arr.dtype)
    arr = np.ascontiguousarray(arr.astype(np.int64, copy=False).reshape(-1))
    return torch.from_numpy(arr).to(dev)


class _Take:
    """Owns a dq_take: the validated indices of one `take`, mapped to (batch, local row)."""

    def __init__(self, rows, chunk_rows: Sequence[int], device: int):
        self.m = int(rows.numel())
        self.n_chunks = len(chunk_rows)
        lens = (ctypes.c_int64 * max(1, self.n_chunks))(*chunk_rows)
        h = ctypes.c_void_p()
        L.check(L.lib().dq_take_create(L.Context.get(device).handle, rows.data_ptr() if self.m else None, self.m, lens,
                                       self.n_chunks, ctypes.byref(h)))
        self.handle = h

    def null_rows(self) -> int:
        n = ctypes.c_int64()
        L.check(L.lib().dq_take_info(self.handle, ctypes.byref(n)))
        return n.value

    def layout(self, cols):
        t, vb, nb, ob = ctypes.c_int32(), ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        L.check(L.lib().dq_take_layout(self.handle, cols, ctypes.byref(t), ctypes.byref(vb), ctypes.byref(nb),
                                       ctypes.byref(ob)))
        return t.value, vb.value, nb.value, ob.value

    def gather(self, cols, values, validity, offsets) -> None:
        L.check(L.lib().dq_take_gather(self.handle, cols, values, validity, offsets))

    def column(self, dtype: str, chunks: Sequence[Column], dev) -> Column:
        """One output column (device-resident) from the device-resident `chunks` of its source."""
        import torch
        cols = (L.DqColumn * max(1, len(chunks)))(*[c.to_dq() for c in chunks])
        _, vb, nb, ob = self.layout(cols)
        m = self.m
        offsets = torch.empty(m + 1, dtype=torch.int32, device=dev) if ob else None
        validity = torch.empty(nb, dtype=torch.uint8, device=dev) if nb else None
        if dtype == "string":
            values = torch.empty(vb + 8, dtype=torch.uint8, device=dev)  # (8 spare bytes, as Column.from_pylist leaves)
            values[vb:] = 0
        elif dtype == "bool":
            values = torch.empty(vb, dtype=torch.uint8, device=dev)
        elif L.is_decimal(dtype):
            values = torch.empty((m, 2), dtype=torch.int64, device=dev)
        else:
            values = torch.empty(m, dtype=getattr(torch, _TORCH[dtype]), device=dev)
        torch.cuda.synchronize(dev)  # the library works on its own stream
        ptr = lambda t, n: t.data_ptr() if (t is not None and n) else None  # noqa: E731
        self.gather(cols, ptr(values, vb), ptr(validity, nb), ptr(offsets, ob))
        return Column(dtype, m, values, validity, offsets, device=True)

    def close(self) -> None:
        if getattr(self, "handle", None):
            L.lib().dq_take_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 - interpreter shutdown
            pass


def _to_host(c: Column) -> Column:
    def down(t):
        return None if t is None else t.cpu().numpy()
    values = down(c.values)
    if L.is_decimal(c.dtype):
        values = values.view(np.uint64)
    return Column(c.dtype, c.length, values, down(c.validity), down(c.offsets))


def take(data, rows, columns: Optional[Sequence[str]] = None) -> Table:
    """The rows `rows` of `data` (a Table, PartitionedTable or ArrowTable) as one Table, in the order
    of `rows`: an int64 torch tensor (in HBM or on the host), a numpy array or a list of global row
    numbers, -1 for an all-NULL row.  `columns` defaults to all, in schema order.  The result is
    device-resident when every batch of `data` is; otherwise host batches are uploaded column by
    column and the result comes back on the host."""
    import torch
    from .comparison import _as_table
    from .distributed import is_sharded
    from .engine import current_device
    from .rowlevel import _on_device
    if is_sharded(data):
        raise L.UnsupportedOnGpu(L.DQ_ERR_UNSUPPORTED, "take over a ShardedTable: a key's owner is another rank, and "
                                 "the outcome bitmaps are not gathered across ranks")
    schema = data.schema
    names = list(schema) if columns is None else ([columns] if isinstance(columns, str) else list(columns))
    for n in names:
        if n not in schema:
            raise ValueError("take: the table has no column %r" % (n,))
    names = list(dict.fromkeys(names))
    device = current_device()
    dev = torch.device("cuda", device)
    on_device = _on_device(data)
    batches = data.batches()
    d_rows = _device_rows(rows, dev)
    torch.cuda.synchronize(dev)  # the library works on its own stream: the indices are there
    t = _Take(d_rows, [b.num_rows for b in batches], device)
    try:
        out = OrderedDict()
        for n in names:
            chunks = [_as_table(b, [n]).columns[n].to_device(device) for b in batches]
            col = t.column(schema[n], chunks, dev)
            out[n] = col if on_device else _to_host(col)
            del chunks
    finally:
        t.close()
    return Table(out)


__all__ = ["take"]
