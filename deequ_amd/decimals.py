"""Decimal columns beyond the fused scan: the decimal -> float64 materialisation and the routes
that ride on it, and the refusals of what decimal columns do not do on the GPU.

The reference's StatefulStdDevPop, Corr and the percentile digest all take DoubleType, so Spark
casts a DecimalType(p, s) operand row by row first: Decimal.toDouble = BigDecimal.doubleValue, the
correctly rounded value of unscaled / 10^s.  StandardDeviation does that cast inside the decimal
scan; Correlation and ApproxQuantile(s) run their existing float64 kernels over a float64 column
that dq_cast_decimal wrote, one batch at a time (`Float64View`), so their results equal, bit for bit,
the same analyzer over a float64 column of the converted values.
"""
from __future__ import annotations

import ctypes
from collections import OrderedDict
from typing import Dict, Iterable, List, Sequence

from . import _lib as L


def spark_type_name(dtype: str) -> str:
    """"decimal(p,s)" -> Spark's DecimalType(p,s)."""
    p, s = L.decimal_params(dtype)
    return "DecimalType(%d,%d)" % (p, s)


def decimal_columns(schema: Dict[str, str], columns: Iterable[str]) -> List[str]:
    out = []
    for c in columns:
        if c in schema and L.is_decimal(schema[c]) and c not in out:
            out.append(c)
    return out


def reject_decimal(schema: Dict[str, str], columns: Iterable[str], what: str) -> None:
    """UnsupportedOnGpu naming the first decimal column among `columns` (the reference
    would run this on Spark; never a wrong answer)."""
    for c in decimal_columns(schema, columns):
        raise L.UnsupportedOnGpu(L.DQ_ERR_UNSUPPORTED, "%s: column %s is %s, which is not on the GPU path"
                                 % (what, c, schema[c]))


def cast_to_float64(column, device: int):
    """dq_cast_decimal of one decimal Column: a device-resident float64 Column with the source's NULLs."""
    import torch
    from .table import Column
    n = column.length
    dev = torch.device("cuda", device)
    values = torch.empty(max(1, n), dtype=torch.float64, device=dev)
    validity = torch.zeros(max(1, (n + 7) // 8) + 8, dtype=torch.uint8, device=dev)
    src = column.to_dq()
    # the library's stream waits for no torch stream: the column is there and the validity is zeroed
    L.after_current_stream(device)
    L.check(L.lib().dq_cast_decimal(L.Context.get(device).handle, ctypes.byref(src), n, values.data_ptr(),
                                    validity.data_ptr()))
    return Column("float64", n, values, validity, device=True)


class Float64View:
    """`data` with the decimal columns `names` replaced by their float64 casts.  Batches are cast as
    they are asked for and a batch's float64 columns are released once the next one is asked for
    (after the device has finished reading them), so one batch's casts are resident at a time."""

    def __init__(self, data, names: Sequence[str], device: int):
        self.data = data
        self.names = [n for n in names if L.is_decimal(data.schema[n])]
        self.device = device
        self._schema = OrderedDict((k, "float64" if k in self.names else t) for k, t in data.schema.items())

    @property
    def schema(self) -> Dict[str, str]:
        return self._schema

    def count(self) -> int:
        return self.data.count()

    @property
    def num_rows(self) -> int:
        return self.count()

    def batches(self):
        import torch
        from .table import Table
        for batch in self.data.batches():
            cols = OrderedDict(batch.columns)
            for n in self.names:
                cols[n] = cast_to_float64(cols[n], self.device)
            view = Table(cols)
            yield view
            torch.cuda.synchronize(self.device)  # the scan of this batch has read the casts
            del view, cols


def float64_view(data, columns: Iterable[str]):
    """`data` itself when none of `columns` is decimal, else a Float64View casting those that are."""
    from .distributed import is_sharded
    from .engine import current_device
    names = decimal_columns(data.schema, columns)
    if not names:
        return data
    if is_sharded(data):
        raise L.UnsupportedOnGpu(L.DQ_ERR_UNSUPPORTED, "decimal column %s of a ShardedTable: the cast runs on "
                                 "single-device tables" % names[0])
    return Float64View(data, names, current_device())


__all__ = ["Float64View", "cast_to_float64", "decimal_columns", "float64_view", "reject_decimal", "spark_type_name"]
