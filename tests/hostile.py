"""Columns whose buffers are as hostile as the Arrow layout allows.

`Column.from_pylist` (and pyarrow) write 0 / "" under every NULL, zero the bitmap's padding bits
and put nothing around the rows.  Arrow leaves all of that unspecified, and exporters leave stale
values there.  `hostile_column` builds a column with the same logical content whose

* rows outside [offset, offset + length) are valid (bit 1) and hold INT_MAX / INT_MIN, +-1e300 /
  NaN / +-Inf, set bits, or non-empty strings;
* bitmap padding bits -- and eight bytes beyond the last bitmap byte -- are all 1;
* NULL slots inside the window hold the same values; a NULL string slot spans 1..9 heap bytes,
  sized so that the starts of the strings after NULL slots walk through every residue mod 8;
* string heap has >= 32 guard bytes before the window's first string and after its last, and every
  byte that is not part of a valid window string comes from the `flavour`:
    "digits"  9 . e -      (would lengthen a number or a packed digit key)
    "high"    0xFF 0x80    (sign-extension, UTF-8 continuation bytes)
    "text"    1 t r u e 0 k (would complete a literal, a key, a pattern match; 'e' after a string
                            ending in "tru" / "fals")

Every buffer's base is 64-byte aligned (as Arrow recommends); misalignment comes from `offset` and
the string offsets alone.  device=False gives numpy buffers, device=True the same bytes as torch
tensors in HBM."""
from collections import OrderedDict

import numpy as np

import deequ_amd as d

TRAILING = 70  # rows after the window (at least)
GUARD = 32     # heap bytes before the first / after the last window string (at least)

FLAVOURS = ("digits", "high", "text")
# Window lengths (one wave, the 2048-row iteration +-1, several blocks) and offsets: 8 and 24 keep a
# bitmap in place at a byte address that is no multiple of 4; 1, 7, 61 and 2051 need it realigned;
# sliced values are 16-byte aligned for some widths only (int8 at 24 and int64 at 1 are copied,
# int64 at 8 is used in place).
WINDOWS = (1, 63, 64, 65, 2047, 2049, 6151)
OFFSETS = (0, 1, 7, 8, 24, 61, 64, 2051)
# (n, index of the first column's offset): column j of a table takes OFFSETS[(index + j) % 8], so
# the columns of one table are sliced differently and every dtype meets every offset
PAIRS = [(1, 0), (1, 3), (63, 1), (63, 4), (64, 2), (64, 5), (65, 6), (65, 7), (2047, 2), (2047, 4),
         (2049, 3), (2049, 1), (6151, 5), (6151, 0), (2049, 7), (2047, 6)]
NUMERIC = ("int8", "int16", "int32", "int64", "float32", "float64")
_FILL = {"digits": b"9.e-", "high": b"\xff\x80", "text": b"1true0k"}
_NP = {"int8": np.int8, "int16": np.int16, "int32": np.int32, "int64": np.int64,
       "float32": np.float32, "float64": np.float64}


def hostile_values(dtype):
    """The values put under NULLs and outside the window (a NaN and an Inf among the floats)."""
    if dtype.startswith("int"):
        info = np.iinfo(_NP[dtype])
        return [int(info.max), int(info.min), -1]
    if dtype == "float32":
        big = float(np.finfo(np.float32).max)
        return [float("nan"), float("inf"), big, -big, float("-inf")]
    return [float("nan"), float("inf"), 1e300, -1e300, float("-inf")]


def _aligned(nbytes, fill):
    """uint8 array of nbytes at a 64-byte aligned address."""
    raw = np.full(nbytes + 64, fill, dtype=np.uint8)
    shift = (-raw.ctypes.data) % 64
    out = raw[shift:shift + nbytes]
    assert out.ctypes.data % 64 == 0
    return out


def _bitmap(total_rows, window_bits, offset):
    """All-ones bitmap (padding and 8 spare bytes included) with the window's bits written in."""
    nbytes = (total_rows + 7) // 8 + 8
    bits = np.ones(nbytes * 8, dtype=np.uint8)
    bits[offset:offset + len(window_bits)] = window_bits
    out = _aligned(nbytes, 0xFF)
    out[:] = np.packbits(bits, bitorder="little")
    return out


def _filler(flavour, n, prev=b"", alt=0):
    """n bytes of the flavour, restarting at each span.  "digits" spans start with '9' (a longer
    number, another value) or, alt = 1, with '.' (an Integral read one byte too far is Fractional)."""
    pat = _FILL[flavour]
    if flavour == "digits" and alt:
        pat = pat[1:] + pat[:1]
    head = b"e" if flavour == "text" and (prev.endswith(b"tru") or prev.endswith(b"fals")) else b""
    return (head + pat * (n // len(pat) + 1))[:n]


def _string_buffers(values, offset, trailing, flavour):
    n = len(values)
    total = offset + n + trailing
    chunks = [_filler(flavour, GUARD + 5)]  # (+5: the first row does not start 8-aligned)
    pos = len(chunks[0])
    offs = np.zeros(total + 1, dtype=np.int32)
    k_null = 0
    prev = b""
    for r in range(total):
        offs[r] = pos
        v = values[r - offset] if offset <= r < offset + n else None
        if v is not None:
            span = v.encode("utf-8")
            prev = span
        elif offset <= r < offset + n:
            # a NULL slot: 1..9 bytes, so that the next row starts at residue k_null mod 8
            ln = (k_null - pos) % 8 or 8
            if ln == 1 and (k_null // 8) % 2:
                ln = 9
            span = _filler(flavour, ln, prev, alt=(k_null // 8 + k_null) % 2)
            k_null += 1
            prev = b""
        else:
            span = _filler(flavour, 1 + r % 9, prev)
            prev = b""
        chunks.append(span)
        pos += len(span)
    offs[total] = pos
    chunks.append(_filler(flavour, GUARD + 7, prev))
    blob = b"".join(chunks)
    heap = _aligned(len(blob), 0)
    heap[:] = np.frombuffer(blob, dtype=np.uint8)
    aoffs = _aligned(offs.nbytes, 0).view(np.int32)
    aoffs[:] = offs
    return heap, aoffs


def hostile_column(dtype, values, *, offset=0, device=False, flavour="digits", trailing=TRAILING):
    """A d.Column of logical content `values` (None = NULL) inside hostile buffers (see above)."""
    if flavour not in FLAVOURS:
        raise ValueError("unknown flavour %r" % (flavour,))
    if trailing < TRAILING:
        raise ValueError("at least %d trailing rows" % TRAILING)
    values = list(values)
    n = len(values)
    total = offset + n + trailing
    valid = np.array([v is not None for v in values], dtype=np.uint8)
    validity = _bitmap(total, valid, offset)
    offsets = None
    if dtype == "string":
        vals, offsets = _string_buffers(values, offset, trailing, flavour)
    elif dtype == "bool":
        window = np.array([1 if (v is None or v) else 0 for v in values], dtype=np.uint8)
        vals = _bitmap(total, window, offset)
    else:
        bad = hostile_values(dtype)
        full = [bad[r % len(bad)] for r in range(total)]
        k = 0
        for i, v in enumerate(values):
            if v is None:
                full[offset + i] = bad[k % len(bad)]
                k += 1
            else:
                full[offset + i] = v
        arr = np.array(full, dtype=_NP[dtype])
        vals = _aligned(arr.nbytes, 0).view(_NP[dtype])
        vals[:] = arr
    col = d.Column(dtype, n, vals, validity, offsets, offset=offset, device=False)
    return col.to_device(0) if device else col


def _per_column(v, name):
    return v[name] if isinstance(v, dict) else v


def hostile_table(spec, *, offset=0, device=False, flavour="digits", trailing=TRAILING):
    """helpers.product_table's counterpart: {name: [dtype, values]} -> d.Table of hostile columns.
    `offset` and `flavour` may be dicts keyed by column name."""
    cols = OrderedDict()
    for name, (dtype, values) in spec.items():
        cols[name] = hostile_column(dtype, values, offset=_per_column(offset, name), device=device,
                                    flavour=_per_column(flavour, name), trailing=trailing)
    return d.Table(cols)


# ---------------------------------------------------------------- the string windows of the tests
def _letters(rng, n):
    return "".join("abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ_ ,;"[int(i)] for i in rng.integers(0, 56, n))


def residue_grid(make, lengths=range(0, 41), extra=()):
    """[None, s] * 8 for each length: the builder's NULL spans give the eight strings of one length
    the eight start residues mod 8.  `make(length, k)` returns the k-th string of that byte length
    (or None to leave the combination out); `extra` strings follow, each after one NULL."""
    out = []
    for ln in lengths:
        for k in range(8):
            s = make(ln, k)
            if s is not None:
                out += [None, s]
    for s in extra:
        out += [None, s]
    return out + [None]


MULTIBYTE = ["é", "日本語", "😀", "a😀b", "ñandú€", "x" * 61 + "é", "é" * 32, "€" * 21 + "z", "日" * 24, "😀" * 16 + "q"]


def distinct_register_strings(seed=7):
    """String window for HLL: every (start mod 8, byte length 0..40) combination, byte lengths
    41..72 and multi-byte UTF-8, in which no two different strings share an HLL register index
    (pyoracle.spark_hash), so the expected words pin every row's (index, rank)."""
    import pyoracle as O
    rng = np.random.default_rng(seed)
    used = {}

    def idx(s):
        return O.hll_index_and_rank(O.spark_hash(s, "string"))[0]

    def fresh(ln):
        if ln == 0:
            used.setdefault(idx(""), "")
            return ""
        for _ in range(2000):
            s = _letters(rng, ln)
            i = idx(s)
            if used.get(i, s) == s:
                used[i] = s
                return s
        raise AssertionError("no free HLL register for a string of length %d" % ln)

    for s in MULTIBYTE:
        assert used.setdefault(idx(s), s) == s, "multi-byte strings share a register: change one"
    # (short strings last: they start inside the final 16 / 24 bytes of the window's heap, where
    # the kernels' window loads are shifted down)
    vals = residue_grid(lambda ln, k: fresh(ln), extra=[fresh(ln) for ln in range(41, 73)] + MULTIBYTE +
                        [fresh(ln) for ln in (15, 9, 4, 2, 1)])
    strings = {v for v in vals if v is not None}
    assert len({idx(s) for s in strings}) == len(strings)
    return vals
