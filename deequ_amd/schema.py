"""Row-level schema enforcement on the GPU: the mirror of the reference's
`com.amazon.deequ.schema` (RowLevelSchemaValidator.scala).

`RowLevelSchemaValidator.validate(data, schema)` takes a batch of string-typed columns, evaluates
the schema's conjunction per row (Kleene three-valued logic, as Spark does) and returns the rows
that are TRUE (`validRows`, cast to the declared types) and the rows that are FALSE (`invalidRows`,
as they came) as new device-resident tables in input row order.  A row whose conjunction is NULL --
a NULL cell of a nullable int column with a `minValue`, RowLevelSchemaValidator.scala:246 -- is in
neither, exactly as `where(m)` and `where(not(m))` both drop it.

What the GPU cannot decide exactly it declines (`UnsupportedOnGpu`; the caller runs the schema on
Spark): timestamp columns, patterns outside the regex compiler's exact subset, decimal precision
above 18, and decimal cells with a non-ASCII byte or an exponent beyond +-1000.
"""
from __future__ import annotations

import ctypes
from collections import OrderedDict, namedtuple
from typing import Dict, List, Optional, Tuple

import numpy as np

from . import _lib as L
from .table import Column, PartitionedTable, Table, dq_columns

StringColumnDefinition = namedtuple("StringColumnDefinition", "name isNullable minLength maxLength matches")
IntColumnDefinition = namedtuple("IntColumnDefinition", "name isNullable minValue maxValue")
DecimalColumnDefinition = namedtuple("DecimalColumnDefinition", "name precision scale isNullable")
TimestampColumnDefinition = namedtuple("TimestampColumnDefinition", "name mask isNullable")


class RowLevelSchema:
    """A simple schema definition for relational data (RowLevelSchemaValidator.scala:73-151).
    Immutable: every builder returns a new schema."""

    __slots__ = ("_defs",)

    def __init__(self, columnDefinitions=()):
        object.__setattr__(self, "_defs", tuple(columnDefinitions))

    def __setattr__(self, name, value):
        raise AttributeError("RowLevelSchema is immutable")

    @property
    def columnDefinitions(self) -> tuple:
        return self._defs

    def __eq__(self, other):
        return isinstance(other, RowLevelSchema) and self._defs == other._defs

    def __hash__(self):
        return hash(self._defs)

    def __repr__(self):
        return "RowLevelSchema(%r)" % (list(self._defs),)

    def withStringColumn(self, name: str, isNullable: bool = True, minLength: Optional[int] = None,
                         maxLength: Optional[int] = None, matches: Optional[str] = None) -> "RowLevelSchema":
        return RowLevelSchema(self._defs + (StringColumnDefinition(name, bool(isNullable), minLength, maxLength,
                                                                   matches),))

    def withIntColumn(self, name: str, isNullable: bool = True, minValue: Optional[int] = None,
                      maxValue: Optional[int] = None) -> "RowLevelSchema":
        return RowLevelSchema(self._defs + (IntColumnDefinition(name, bool(isNullable), minValue, maxValue),))

    def withDecimalColumn(self, name: str, precision: int, scale: int, isNullable: bool = True) -> "RowLevelSchema":
        return RowLevelSchema(self._defs + (DecimalColumnDefinition(name, int(precision), int(scale),
                                                                    bool(isNullable)),))

    def withTimestampColumn(self, name: str, mask: str, isNullable: bool = True) -> "RowLevelSchema":
        return RowLevelSchema(self._defs + (TimestampColumnDefinition(name, mask, bool(isNullable)),))


class RowLevelSchemaValidationResult:
    """validRows / invalidRows are `Table`s of device-resident columns (a `PartitionedTable` with one
    part per input batch when the data was one).  `decimalColumns` records (precision, scale) of every
    validRows column that holds unscaled int64 decimals.  With `withRowIndices=True`,
    `validRowIndices` / `invalidRowIndices` hold the source row of every output row (a list of arrays,
    one per batch, for a PartitionedTable)."""

    def __init__(self, validRows, numValidRows: int, invalidRows, numInvalidRows: int,
                 decimalColumns: Dict[str, Tuple[int, int]], validRowIndices=None, invalidRowIndices=None):
        self.validRows = validRows
        self.numValidRows = numValidRows
        self.invalidRows = invalidRows
        self.numInvalidRows = numInvalidRows
        self.decimalColumns = decimalColumns
        self.validRowIndices = validRowIndices
        self.invalidRowIndices = invalidRowIndices

    def __iter__(self):  # the reference's four fields, in order
        return iter((self.validRows, self.numValidRows, self.invalidRows, self.numInvalidRows))


_INT32 = (-(1 << 31), (1 << 31) - 1)
_NP_OF = {L.DQ_T_INT8: "int8", L.DQ_T_INT16: "int16", L.DQ_T_INT32: "int32", L.DQ_T_INT64: "int64",
          L.DQ_T_FLOAT32: "float32", L.DQ_T_FLOAT64: "float64", L.DQ_T_BOOL: "bool", L.DQ_T_UTF8: "string"}


def _check_arguments(schema: RowLevelSchema, names: List[str]) -> None:
    """Spark's AnalysisException cases, before anything is declined."""
    for d in schema.columnDefinitions:
        if d.name not in names:
            raise ValueError("cannot resolve column %r among (%s)" % (d.name, ", ".join(names)))
        if isinstance(d, DecimalColumnDefinition):
            if not 1 <= d.precision <= 38:
                raise ValueError("DecimalType precision %d of column %r is outside 1..38" % (d.precision, d.name))
            if not 0 <= d.scale <= d.precision:
                raise ValueError("DecimalType scale %d of column %r is outside 0..precision (%d)"
                                 % (d.scale, d.name, d.precision))
        for bound in ((d.minValue, d.maxValue) if isinstance(d, IntColumnDefinition) else
                      (d.minLength, d.maxLength) if isinstance(d, StringColumnDefinition) else ()):
            if bound is not None and not _INT32[0] <= int(bound) <= _INT32[1]:
                raise ValueError("bound %r of column %r is not a 32-bit Int" % (bound, d.name))


def _abi_definitions(schema: RowLevelSchema, table_schema: Dict[str, str]):
    """(dq_schema_def array, its length, column types array, objects to keep alive)."""
    names = list(table_schema.keys())
    defs = list(schema.columnDefinitions)
    arr = (L.DqSchemaDef * max(1, len(defs)))()
    keep = []
    for i, d in enumerate(defs):
        a = arr[i]
        a.column = names.index(d.name)
        a.flags = 0 if d.isNullable else L.DQ_SCHEMA_NOT_NULL
        lo = hi = None
        if isinstance(d, StringColumnDefinition):
            a.kind = L.DQ_SCHEMA_STRING
            lo, hi = d.minLength, d.maxLength
            if d.matches is not None:
                pat = d.matches.encode("utf-8")
                keep.append(pat)
                a.pattern, a.pattern_len = pat, len(pat)
                a.flags |= L.DQ_SCHEMA_HAS_PATTERN
        elif isinstance(d, IntColumnDefinition):
            a.kind = L.DQ_SCHEMA_INT
            lo, hi = d.minValue, d.maxValue
        elif isinstance(d, DecimalColumnDefinition):
            a.kind = L.DQ_SCHEMA_DECIMAL
            a.precision, a.scale = d.precision, d.scale
        else:
            a.kind = L.DQ_SCHEMA_TIMESTAMP
        if lo is not None:
            a.flags |= L.DQ_SCHEMA_HAS_MIN
            a.min_value = int(lo)
        if hi is not None:
            a.flags |= L.DQ_SCHEMA_HAS_MAX
            a.max_value = int(hi)
    types = (ctypes.c_int32 * max(1, len(names)))(*[L.TYPE_CODES[table_schema[c]] for c in names])
    return arr, len(defs), types, keep


def check_schema(schema: RowLevelSchema, table_schema: Dict[str, str]) -> None:
    """The plan-time checks, without a device: ValueError for what Spark rejects, UnsupportedOnGpu
    (the message names the definition) for what the GPU declines."""
    _check_arguments(schema, list(table_schema.keys()))
    from .decimals import reject_decimal
    reject_decimal(table_schema, table_schema.keys(), "RowLevelSchemaValidator input")
    arr, n, types, _keep = _abi_definitions(schema, table_schema)
    L.check(L.lib().dq_schema_supported(arr, n, types, len(table_schema)))


class _Validator:
    """Owns a dq_schema for one RowLevelSchema over a fixed table schema."""

    def __init__(self, schema: RowLevelSchema, table_schema: Dict[str, str], device: int):
        self.device = device
        self.ctx = L.Context.get(device)
        self.names = list(table_schema.keys())
        self.defs = list(schema.columnDefinitions)
        from .decimals import reject_decimal
        reject_decimal(table_schema, table_schema.keys(), "RowLevelSchemaValidator input")
        arr, n, types, self._keep = _abi_definitions(schema, table_schema)
        h = ctypes.c_void_p()
        L.check(L.lib().dq_schema_create(self.ctx.handle, arr, n, types, len(self.names), ctypes.byref(h)))
        self.handle = h
        # castExpressions.toMap: the last definition of a column decides its cast
        self.decimals = OrderedDict()
        last = {d.name: d for d in self.defs}
        for c in self.names:
            if isinstance(last.get(c), DecimalColumnDefinition):
                self.decimals[c] = (last[c].precision, last[c].scale)

    def close(self) -> None:
        if getattr(self, "handle", None):
            L.lib().dq_schema_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 - interpreter shutdown
            pass

    def _output(self, which: int, rows: int) -> Table:
        import torch
        dev = torch.device("cuda", self.device)
        lib = L.lib()
        cols = OrderedDict()
        for ci, name in enumerate(self.names):
            t, vb, nb, ob = ctypes.c_int32(), ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
            L.check(lib.dq_schema_output_layout(self.handle, which, ci, ctypes.byref(t), ctypes.byref(vb),
                                                ctypes.byref(nb), ctypes.byref(ob)))
            dtype = _NP_OF[t.value]
            if dtype in ("string", "bool"):
                # (never an empty allocation: other entry points want a non-NULL values pointer)
                values = torch.empty(vb.value, dtype=torch.uint8, device=dev) if vb.value else \
                    torch.zeros(8, dtype=torch.uint8, device=dev)
            else:
                values = torch.empty(rows, dtype=getattr(torch, dtype), device=dev)
            validity = torch.empty(nb.value, dtype=torch.uint8, device=dev) if nb.value else None
            offsets = torch.empty(ob.value // 4, dtype=torch.int32, device=dev) if ob.value else None
            L.after_current_stream(self.device)  # (nothing queued there still uses the memory the outputs took)
            L.check(lib.dq_schema_gather(self.handle, which, ci, values.data_ptr() if vb.value else None,
                                         validity.data_ptr() if validity is not None else None,
                                         offsets.data_ptr() if offsets is not None else None))
            cols[name] = Column(dtype, rows, values, validity, offsets, offset=0, device=True)
        return Table(cols)

    def _indices(self, which: int, rows: int) -> np.ndarray:
        out = np.empty(rows, dtype=np.int32)
        L.check(L.lib().dq_schema_selection(self.handle, which, out.ctypes.data if rows else None, rows))
        return out

    def validate(self, batch: Table, with_indices: bool):
        cols = dq_columns(batch, self.names)
        nv, ni = ctypes.c_int64(), ctypes.c_int64()
        flags = (ctypes.c_int32 * max(1, len(self.defs)))()
        if L.device_inputs(batch.columns[n] for n in self.names):
            L.after_current_stream(self.device)  # the library's launches wait for no torch stream: the batch is there
        st = L.lib().dq_schema_validate(self.handle, cols, len(self.names), batch.num_rows, ctypes.byref(nv),
                                        ctypes.byref(ni), flags)
        flagged = [self.defs[i].name for i in range(len(self.defs)) if flags[i]]
        if st == L.DQ_ERR_UNSUPPORTED and flagged:
            raise L.UnsupportedOnGpu(st, "decimal column %s holds a cell the GPU cannot judge as java.math.BigDecimal "
                                         "does (a non-ASCII byte, or an exponent beyond +-1000)"
                                     % ", ".join(repr(c) for c in dict.fromkeys(flagged)))
        L.check(st)
        valid, invalid = self._output(0, nv.value), self._output(1, ni.value)
        idx = (self._indices(0, nv.value), self._indices(1, ni.value)) if with_indices else (None, None)
        return valid, nv.value, invalid, ni.value, idx


class RowLevelSchemaValidator:
    """Enforce a schema on textual data (RowLevelSchemaValidator.scala:169-282)."""

    @staticmethod
    def validate(data, schema: RowLevelSchema, withRowIndices: bool = False) -> RowLevelSchemaValidationResult:
        from .distributed import is_sharded
        from .engine import current_device
        if is_sharded(data):
            raise L.UnsupportedOnGpu(L.DQ_ERR_UNSUPPORTED, "RowLevelSchemaValidator over a ShardedTable: the row "
                                     "tables are not gathered across ranks")
        if not isinstance(data, (Table, PartitionedTable)):
            raise TypeError("RowLevelSchemaValidator.validate takes a Table or a PartitionedTable")
        if not isinstance(schema, RowLevelSchema):
            raise TypeError("schema must be a RowLevelSchema")
        check_schema(schema, data.schema)
        v = _Validator(schema, data.schema, current_device())
        try:
            parts = [v.validate(batch, withRowIndices) for batch in data.batches()]
        finally:
            v.close()
        decimals = dict(v.decimals)
        if isinstance(data, PartitionedTable):
            return RowLevelSchemaValidationResult(
                PartitionedTable([p[0] for p in parts]), sum(p[1] for p in parts),
                PartitionedTable([p[2] for p in parts]), sum(p[3] for p in parts), decimals,
                [p[4][0] for p in parts] if withRowIndices else None,
                [p[4][1] for p in parts] if withRowIndices else None)
        valid, nv, invalid, ni, idx = parts[0]
        return RowLevelSchemaValidationResult(valid, nv, invalid, ni, decimals, idx[0], idx[1])


__all__ = ["RowLevelSchema", "RowLevelSchemaValidator", "RowLevelSchemaValidationResult", "check_schema",
           "StringColumnDefinition", "IntColumnDefinition", "DecimalColumnDefinition",
           "TimestampColumnDefinition"]
