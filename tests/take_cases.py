"""Cases for take (deequ_amd/take.py, dq_take_*) and a numpy restatement of it over host Columns.

`restate(chunks, rows)` is written from the contract in include/deequ_amd.h, not from the kernels:
it walks the chunks' Arrow buffers at their `offset` and builds the output buffers byte for byte --
values (a fixed-width NULL cell keeps its source bytes, a -1 cell is zeros), validity and bool
words (whole 64-bit words, the bits past m 0), int32 offsets and the utf8 heap (a NULL or -1 cell
has length 0).  test_take.py checks it against pyarrow's take; test_gpu_take.py checks the GPU
against it buffer for buffer.
"""
from collections import OrderedDict

import numpy as np

import deequ_amd as d
from deequ_amd import _lib as L
from hostile import MULTIBYTE, hostile_column

FIXED = ("int8", "int16", "int32", "int64", "float32", "float64")
DEC_WIDE, DEC_MONEY = "decimal(38,10)", "decimal(12,2)"
DTYPES = FIXED + ("bool", DEC_WIDE, DEC_MONEY, "string")
_NP = {"int8": np.int8, "int16": np.int16, "int32": np.int32, "int64": np.int64,
       "float32": np.float32, "float64": np.float64}


def width(dtype):
    return 16 if L.is_decimal(dtype) else np.dtype(_NP[dtype]).itemsize


# ---------------------------------------------------------------- restatement
class Taken:
    """The output buffers of one column: `values` raw bytes (uint8), `validity` uint64 words or
    None, `offsets` int32 or None."""

    def __init__(self, dtype, m, values, validity, offsets):
        self.dtype, self.m, self.values, self.validity, self.offsets = dtype, m, values, validity, offsets

    def column(self):
        """The same as a host Column (logical views: to_pylist)."""
        vals = self.values
        if self.dtype == "string":
            vals = np.concatenate([vals, np.zeros(8, np.uint8)])
        elif L.is_decimal(self.dtype):
            vals = vals.view(np.uint64).reshape(-1, 2)
        elif self.dtype != "bool":
            vals = vals.view(_NP[self.dtype])
        validity = None if self.validity is None else self.validity.view(np.uint8)
        return d.Column(self.dtype, self.m, vals, validity, self.offsets)


def _host(a):
    return None if a is None else (a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a))


def _bits(buf, first, n):
    """Bits [first, first + n) of an LSB-first bitmap as booleans."""
    raw = np.ascontiguousarray(_host(buf)).view(np.uint8)
    lo, hi = first // 8, (first + n + 7) // 8
    return np.unpackbits(raw[lo:hi], bitorder="little")[first - 8 * lo:first - 8 * lo + n].astype(bool)


def _words(bits):
    padded = np.zeros(((len(bits) + 63) // 64) * 64, dtype=bool)
    padded[:len(bits)] = bits
    return np.packbits(padded, bitorder="little").view("<u8")


def locate(lengths, rows):
    """(chunk, local row) per index; chunk -1 for -1.  ValueError for anything else out of range."""
    rows = np.asarray(rows, dtype=np.int64).reshape(-1)
    prefix = np.concatenate([[0], np.cumsum(np.asarray(lengths, dtype=np.int64))])
    bad = (rows < -1) | (rows >= prefix[-1])
    if bad.any():
        o = int(np.argmax(bad))
        raise ValueError("rows[%d] = %d" % (o, rows[o]))
    chunk = np.searchsorted(prefix, rows, side="right") - 1
    chunk[rows < 0] = -1
    local = rows - prefix[np.maximum(chunk, 0)]
    local[rows < 0] = 0
    return chunk.astype(np.int64), local


def restate(chunks, rows):
    """take over the host Columns `chunks` (one column's batches) -> Taken."""
    dtype = chunks[0].dtype
    assert all(c.dtype == dtype for c in chunks)
    chunk, local = locate([c.length for c in chunks], rows)
    m = len(chunk)
    valid = np.zeros(m, dtype=bool)
    for k, c in enumerate(chunks):
        sel = np.nonzero(chunk == k)[0]
        if len(sel):
            valid[sel] = True if c.validity is None else _bits(c.validity, c.offset, c.length)[local[sel]]
    has_validity = m > 0 and (any(c.validity is not None for c in chunks) or bool((chunk < 0).any()))
    validity = _words(valid) if has_validity else None
    offsets = None
    if dtype == "bool":
        bits = np.zeros(m, dtype=bool)
        for k, c in enumerate(chunks):
            sel = np.nonzero(chunk == k)[0]
            if len(sel):
                bits[sel] = _bits(c.values, c.offset, c.length)[local[sel]]
        values = _words(bits).view(np.uint8)
    elif dtype == "string":
        lens = np.zeros(m, dtype=np.int64)
        starts = np.zeros(m, dtype=np.int64)
        for k, c in enumerate(chunks):
            sel = np.nonzero((chunk == k) & valid)[0]
            if len(sel):
                offs = _host(c.offsets).astype(np.int64)[c.offset:c.offset + c.length + 1]
                starts[sel] = offs[local[sel]]
                lens[sel] = offs[local[sel] + 1] - offs[local[sel]]
        total = int(lens.sum())
        if total > 0x7fffffff:
            raise OverflowError(total)
        offsets = np.zeros(m + 1, dtype=np.int32)
        np.cumsum(lens, out=offsets[1:])
        heaps = [np.ascontiguousarray(_host(c.values)).view(np.uint8) for c in chunks]
        parts = [heaps[chunk[o]][starts[o]:starts[o] + lens[o]] for o in np.nonzero(lens)[0]]
        values = np.concatenate(parts) if parts else np.zeros(0, np.uint8)
    else:
        w = width(dtype)
        values = np.zeros((m, w), dtype=np.uint8)
        for k, c in enumerate(chunks):
            sel = np.nonzero(chunk == k)[0]
            if len(sel):
                raw = np.ascontiguousarray(_host(c.values)).view(np.uint8).reshape(-1, w)
                values[sel] = raw[c.offset:c.offset + c.length][local[sel]]
        values = values.reshape(-1)
    return Taken(dtype, m, values, validity, offsets)


def restate_table(parts, rows, columns=None):
    """{name: Taken} of host Tables `parts` (the batches)."""
    names = list(parts[0].columns) if columns is None else list(columns)
    return OrderedDict((n, restate([p.columns[n] for p in parts], rows)) for n in names)


# ---------------------------------------------------------------- case builders
def random_column(dtype, n, rng, nulls=True):
    """A host Column of n rows built with numpy (fast at 10^5 rows): about one NULL in seven."""
    valid = rng.random(n) >= 0.15 if nulls else None
    if dtype == "bool":
        return d.Column.from_numpy(rng.random(n) < 0.5, valid, "bool")
    if dtype == "string":
        lens = rng.integers(0, 24, n)
        offs = np.zeros(n + 1, dtype=np.int32)
        np.cumsum(lens, out=offs[1:])
        heap = rng.integers(48, 123, int(offs[-1]) + 8).astype(np.uint8)
        return d.Column("string", n, heap, d.table.pack_validity(valid), offsets=offs)
    if L.is_decimal(dtype):
        p, _ = L.decimal_params(dtype)
        words = np.zeros((n, 2), dtype=np.uint64)
        words[:, 0] = rng.integers(0, 1 << 63, n, dtype=np.uint64)
        if p > 18:  # the high word too, the sign bit set on half the rows
            words[:, 1] = rng.integers(0, 1 << 62, n, dtype=np.uint64)
            neg = rng.random(n) < 0.5
            words[neg, 1] = ~words[neg, 1]
        else:
            neg = rng.random(n) < 0.5
            words[:, 0] %= np.uint64(10 ** p)
            words[neg, 0] = (~words[neg, 0]) + np.uint64(1)
            words[neg & (words[:, 0] != 0), 1] = np.uint64(0xFFFFFFFFFFFFFFFF)
        return d.Column.from_numpy(words, valid, dtype)
    if dtype.startswith("float"):
        vals = rng.normal(0, 1e3, n).astype(_NP[dtype])
        return d.Column.from_numpy(vals, valid, dtype)
    info = np.iinfo(_NP[dtype])
    return d.Column.from_numpy(rng.integers(info.min, info.max, n, dtype=_NP[dtype], endpoint=True), valid, dtype)


def random_parts(lengths, seed, dtypes=DTYPES, nulls=True):
    """Host Tables of the given row counts (the batches of one dataset), one column per dtype."""
    rng = np.random.default_rng(seed)
    return [d.Table(OrderedDict(("c_" + t, random_column(t, n, rng, nulls)) for t in dtypes)) for n in lengths]


def chunkings(n):
    """{name: chunk lengths}: one chunk; 1, 64 and the rest; the same with an empty chunk in the middle."""
    out = {"one": [n]}
    if n >= 66:
        out["three"] = [1, 64, n - 65]
        out["empty_middle"] = [1, 64, 0, n - 65]
    return out


def index_shapes(n, m, seed):
    """{name: int64 indices over n rows, m of them (or what the shape gives)}."""
    rng = np.random.default_rng(seed)
    out = {"all_null": np.full(m, -1, dtype=np.int64)}
    if n > 0:
        out["ascending_gaps"] = np.sort(rng.choice(n, size=min(n, m), replace=False)).astype(np.int64)
        out["permutation"] = rng.permutation(n).astype(np.int64)[:m] if m <= n else rng.integers(0, n, m)
        out["same"] = np.full(m, n // 2, dtype=np.int64)
        alt = rng.integers(0, n, m).astype(np.int64)
        alt[1::2] = -1
        out["alternate_null"] = alt
    return out


def chunk_edges(lengths):
    """The first and last row of every non-empty chunk, last rows first."""
    prefix = np.concatenate([[0], np.cumsum(lengths)])
    firsts = [int(prefix[k]) for k, ln in enumerate(lengths) if ln]
    lasts = [int(prefix[k + 1]) - 1 for k, ln in enumerate(lengths) if ln]
    return np.array(lasts + firsts, dtype=np.int64)


SPECIAL_FLOATS = {
    "float64": np.array([0x7ff8000000000001, 0xfff8000000000000, 0x7ff0000000000001, 0x8000000000000000, 0,
                         0x7ff0000000000000, 0xfff0000000000000, 1], dtype=np.uint64).view(np.float64),
    "float32": np.array([0x7fc00001, 0xffc00000, 0x7f800001, 0x80000000, 0, 0x7f800000, 0xff800000, 1],
                        dtype=np.uint32).view(np.float32),
}


def sliced_decimal(values_words, valid, offset, dtype=DEC_WIDE):
    """A decimal Column whose window starts `offset` rows into its buffers (rows before and after
    are valid and hold other words)."""
    n = len(values_words)
    full = np.full((offset + n + 3, 2), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    full[offset:offset + n] = values_words
    bits = np.ones(offset + n + 3 + 64, dtype=bool)
    bits[offset:offset + n] = valid
    return d.Column(dtype, n, full, np.packbits(bits, bitorder="little"), offset=offset)


def string_column(cells, valid=None):
    """A host string Column of the byte strings `cells` laid end to end from heap byte 0."""
    lens = np.array([len(c) for c in cells], dtype=np.int64)
    offs = np.zeros(len(cells) + 1, dtype=np.int32)
    np.cumsum(lens, out=offs[1:])
    heap = np.frombuffer(b"".join(cells) + b"\0" * 8, dtype=np.uint8)
    return d.Column("string", len(cells), heap, d.table.pack_validity(valid), offsets=offs)


def cell_bytes(length, tag):
    """`length` bytes that depend on `tag` and the position (a shifted or repeated copy shows)."""
    return ((np.arange(length, dtype=np.int64) * 7 + tag * 13) % 94 + 33).astype(np.uint8).tobytes()  # (ASCII)


def alignment_grid(lengths):
    """(column, rows): every length of `lengths` as a source cell at each of the 16 start residues
    mod 16 of the heap, taken so that it lands at each of the 16 destination residues.  The column
    starts with 16 spacer cells of lengths 0..15; a spacer before a cell fixes the residue."""
    cells = [cell_bytes(k, 1000 + k) for k in range(16)]
    pos = sum(range(16))
    data = []  # indices of the data cells
    tag = 0
    for ln in lengths:
        for a in range(16):
            pad = (a - pos) % 16
            cells.append(cell_bytes(pad, 2000 + tag))
            pos += pad
            data.append(len(cells))
            cells.append(cell_bytes(ln, tag))
            pos += ln
            tag += 1
    rows, out = [], 0
    for j in data:
        ln = len(cells[j])
        for b in range(16):
            pad = (b - out) % 16
            rows += [pad, j]  # (spacer k has length k)
            out += pad + ln
    return string_column(cells), np.array(rows, dtype=np.int64)


SMALL_LENGTHS = (0, 1, 3, 4, 5, 15, 16, 17)


def threshold_lengths(consts):
    return [consts[k] + dlt for k in ("wave_bytes", "split_bytes") for dlt in (-1, 0, 1)]


def multibyte_column():
    """Multi-byte UTF-8 strings (hostile.MULTIBYTE) between NULL cells whose source ranges are not
    empty, in hostile buffers at a window offset."""
    values = []
    for s in MULTIBYTE:
        values += [s, None]
    return hostile_column("string", values * 3, offset=7, flavour="high")


# ---------------------------------------------------------------- pyarrow views (the independent reference)
def to_arrow(col):
    """A host Column as a pyarrow array over the same buffers (its slice kept)."""
    import pyarrow as pa
    validity = None if col.validity is None else pa.py_buffer(np.ascontiguousarray(_host(col.validity)))
    vals = pa.py_buffer(np.ascontiguousarray(_host(col.values)))
    if col.dtype == "string":
        bufs = [validity, pa.py_buffer(np.ascontiguousarray(_host(col.offsets))), vals]
        typ = pa.string()
    elif L.is_decimal(col.dtype):
        bufs, typ = [validity, vals], pa.decimal128(*L.decimal_params(col.dtype))
    else:
        bufs = [validity, vals]
        typ = pa.bool_() if col.dtype == "bool" else pa.from_numpy_dtype(_NP[col.dtype])
    return pa.Array.from_buffers(typ, col.length, bufs, offset=col.offset)


def arrow_take(chunks, rows):
    """pyarrow's take over the chunked column, -1 as a null index -> Python values."""
    import pyarrow as pa
    idx = pa.array([None if r < 0 else int(r) for r in np.asarray(rows).tolist()], type=pa.int64())
    return pa.chunked_array([to_arrow(c) for c in chunks]).take(idx).to_pylist()


def logical(col):
    """to_pylist in the form pyarrow gives: decimals as Decimal, strings as str."""
    import decimal
    out = col.to_pylist()
    ps = L.decimal_params(col.dtype)
    if ps is not None:
        with decimal.localcontext() as ctx:
            ctx.prec = 60
            out = [None if v is None else decimal.Decimal(v).scaleb(-ps[1]) for v in out]
    return out


def same_values(a, b):
    """Lists equal value for value, floats by their bits (NaN payloads, -0.0)."""
    import struct
    if len(a) != len(b):
        return False
    for x, y in zip(a, b):
        if isinstance(x, float) and isinstance(y, float):
            if struct.pack("<d", x) != struct.pack("<d", y):
                return False
        elif x != y or (x is None) != (y is None):
            return False
    return True
