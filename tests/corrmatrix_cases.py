"""Shared by test_corrmatrix.py (host mirror, CPU) and test_gpu_corrmatrix.py (device): the exact
rational reference and its bar (the helpers of test_gpu_correlation.py), column generators for
every numeric dtype, the NULL patterns, and the ctypes call of dq_diag_corrmat_host.

Bar (test_gpu_correlation.py): n bit-exact; xAvg, yAvg, xMk, yMk within 1e-12 relative of the exact
rational state, ck within 1e-12 of sqrt(xMk * yMk); no absolute slack, so an exact 0 must be 0.0.
Every column is c + k / 2^s with |k| < 2^20, so the exact sums are int64 sums (2^18 rows at most)."""
import ctypes
import math
from fractions import Fraction

import numpy as np

REL_TOL = 1e-12
SLAB = 1024      # kCorrmatSlabRows (deequ_amd/csrc/dq_corrmat.h)
PERIOD = 4096    # "unselected prefix": rows r with r mod PERIOD < PERIOD / 2 are NULL

ROW_COUNTS = [1, 3, 4, 5, 63, 64, 65, SLAB - 1, SLAB, SLAB + 1, 1 << 18]
COLUMN_COUNTS = [1, 2, 15, 16, 17, 33, 64]
NULL_PATTERNS = ["none", "five_percent", "all_null_column", "last_row_only", "prefix"]

_NP = {"int8": np.int8, "int16": np.int16, "int32": np.int32, "int64": np.int64, "float32": np.float32,
       "float64": np.float64}


# ---------------------------------------------------------------- the exact state (test_gpu_correlation.py)
def _state_from_sums(n, cx, sx, cy, sy, Sx, Sy, Sxx, Syy, Sxy):
    """Exact state of the pairs x = cx + kx / sx, y = cy + ky / sy from Σkx, Σky, Σkx², Σky², Σkxky
    (Python ints)."""
    return (n, cx + Fraction(Sx, n * sx), cy + Fraction(Sy, n * sy),
            Fraction(Sxy * n - Sx * Sy, n * sx * sy),
            Fraction(Sxx * n - Sx * Sx, n * sx * sx),
            Fraction(Syy * n - Sy * Sy, n * sy * sy))


def _centred(v):
    """Doubles v = (c + k) / 2**s exactly: (k, c, 2**s), k integers about the first value -- an
    int64 array when their squares can be summed in int64, Python ints otherwise."""
    s = 0
    while not np.array_equal(v * 2.0 ** s, np.rint(v * 2.0 ** s)):
        s += 1
        assert s <= 64, "value with too many fraction bits for this test"
    scaled = v * 2.0 ** s  # exact: a power of two
    assert np.abs(scaled).max() < 2.0 ** 62
    k = scaled.astype(np.int64)
    c = int(k[0])
    k = k - c
    if int(np.abs(k).max()) >= 2 ** 20:
        k = k.astype(object)
    return k, c, 2 ** s


def _exact_state(xs, ys):
    """Exact (n, xAvg, yAvg, ck, xMk, yMk), as Fractions, of the selected pairs (float64 arrays)."""
    (kx, cx, sx), (ky, cy, sy) = _centred(xs), _centred(ys)
    n = len(xs)
    assert n <= 2 ** 23
    return _state_from_sums(n, Fraction(cx, sx), sx, Fraction(cy, sy), sy, int(kx.sum()), int(ky.sum()),
                            int((kx * kx).sum()), int((ky * ky).sum()), int((kx * ky).sum()))


def _errors(got, exact):
    """Relative errors of a state against the exact one (ck on the scale sqrt(xMk * yMk)); a
    field whose exact value (or scale) is 0 reports 0 when it is 0.0 and inf otherwise."""
    n, xa, ya, ck, xmk, ymk = exact

    def rel(g, e, scale):
        diff = abs(Fraction(g) - e) if math.isfinite(g) else None
        if diff == 0:
            return 0.0
        return math.inf if diff is None or scale == 0 else float(diff) / scale
    out = {"xAvg": rel(got.xAvg, xa, abs(float(xa))), "yAvg": rel(got.yAvg, ya, abs(float(ya))),
           "xMk": rel(got.xMk, xmk, float(xmk)), "yMk": rel(got.yMk, ymk, float(ymk)),
           "ck": rel(got.ck, ck, math.sqrt(float(xmk) * float(ymk)))}
    return out


def check_state(label, got, exact, who="kernel"):
    """`got` (a CorrelationState, or None) against the exact state (None: no row has both) at the bar."""
    if exact is None:
        assert got is None, (who, label, got)
        return
    assert got is not None, (who, label)
    err = _errors(got, exact)
    print("%-6s %-44s %s" % (who, label, " ".join("%s=%.2e" % kv for kv in err.items())))
    assert got.n == float(exact[0]), (who, label, got.n, exact[0])
    for k, v in err.items():
        assert v <= REL_TOL, (who, label, k, v, got)
    exact_nan = exact[4] == 0 or exact[5] == 0  # ck / sqrt(xMk * yMk): 0 / 0
    assert math.isnan(got.metricValue()) == exact_nan, (who, label, got)


# ---------------------------------------------------------------- columns
# (dtype, value family): every value exact in its dtype, k = a * base + own with |k| <= 8704.
KINDS = [("float64", "big"), ("int64", "wide"), ("int32", "big"), ("float32", "f32"), ("int16", "i16"),
         ("float64", "frac"), ("int8", "i8"), ("float64", "frac_fine")]


def _values(family, k, fine):
    if family == "big":          # offset 2^24 against a spread of a few thousand
        return 2.0 ** 24 + k
    if family == "wide":
        return 2.0 ** 22 - 2.0 * k
    if family == "f32":          # integers below 2^24: exact in float32
        return 2.0 ** 20 + k
    if family == "i16":
        return 30000.0 + k // 8
    if family == "i8":
        return 40.0 + k // 128
    if family == "frac":         # 20 significant bits: the squares are still exact
        return 1000 + k / 1024
    if family == "frac_fine":    # 30 significant bits: no square is exactly representable
        return 1000 + fine / 2.0 ** 20
    raise ValueError(family)


class Case:
    """k columns of n rows: names c0.., dtypes, the exact doubles, validity (bool arrays)."""

    def __init__(self, k, n, seed, nulls="none"):
        rng = np.random.default_rng(seed)
        base = rng.integers(-4096, 4097, n)
        self.k, self.n = k, n
        self.names = ["c%d" % i for i in range(k)]
        self.dtypes, self.values, self.valid = [], [], []
        for i in range(k):
            dtype, family = KINDS[i % len(KINDS)]
            own = rng.integers(-512, 513, n)
            kk = (i % 3 - 1) * base + own
            fine = rng.integers(-2 ** 18, 2 ** 18 + 1, n)
            v = np.asarray(_values(family, kk, fine), dtype=np.float64)
            assert np.array_equal(v.astype(_NP[dtype]).astype(np.float64), v), (dtype, family)
            self.dtypes.append(dtype)
            self.values.append(v)
            self.valid.append(self._valid(nulls, i, rng))
        self._centred = [None] * k

    def _valid(self, nulls, i, rng):
        n, r = self.n, np.arange(self.n)
        target = 1 if self.k > 1 else 0
        if nulls == "five_percent":
            return rng.random(n) >= 0.05
        if nulls == "all_null_column" and i == target:
            return np.zeros(n, dtype=bool)
        if nulls == "last_row_only" and i == target:
            return r == n - 1
        if nulls == "prefix" and i % 2 == 1:
            return (r % PERIOD) >= PERIOD // 2
        return np.ones(n, dtype=bool)

    def has_nulls(self, i):
        return not self.valid[i].all()

    def numpy_column(self, i):
        return self.values[i].astype(_NP[self.dtypes[i]])

    def table(self, d, rows=slice(None)):
        """A host deequ_amd Table (rows: a slice of the case)."""
        cols = {}
        for i, name in enumerate(self.names):
            cols[name] = d.Column.from_numpy(self.numpy_column(i)[rows], self.valid[i][rows] if self.has_nulls(i) else None,
                                             self.dtypes[i])
        return d.Table(cols)

    def exact(self, i, j, keep=None):
        """The exact state of the pair (i, j) over the rows valid in both (and in `keep`), or None."""
        for c in (i, j):
            if self._centred[c] is None:
                self._centred[c] = _centred(self.values[c])
        s = self.valid[i] & self.valid[j]
        if keep is not None:
            s = s & keep
        n = int(s.sum())
        if n == 0:
            return None
        (kx, cx, sx), (ky, cy, sy) = self._centred[i], self._centred[j]
        kx, ky = kx[s], ky[s]
        return _state_from_sums(n, Fraction(cx, sx), sx, Fraction(cy, sy), sy, int(kx.sum()), int(ky.sum()),
                                int((kx * kx).sum()), int((ky * ky).sum()), int((kx * ky).sum()))

    def pairs(self):
        return [(i, j) for i in range(self.k) for j in range(i, self.k)]


def pair_index(i, j, k):
    return i * k - i * (i - 1) // 2 + (j - i)


# ---------------------------------------------------------------- the host mirror
def host_corrmat(values, valid=None, where=None, max_ranges=0):
    """dq_diag_corrmat_host: ((pairs, 6) states, (pairs,) flags).  values: float64 arrays; valid: bool
    arrays or None per column; where: a bool array or None."""
    from deequ_amd import _lib as L
    k, n = len(values), len(values[0])
    vals = [np.ascontiguousarray(v, dtype=np.float64) for v in values]
    vb = [None if v is None else np.ascontiguousarray(v, dtype=np.uint8) for v in (valid or [None] * k)]
    wb = None if where is None else np.ascontiguousarray(where, dtype=np.uint8)
    cols = (ctypes.c_void_p * k)(*[v.ctypes.data for v in vals])
    vptr = (ctypes.c_void_p * k)(*[None if v is None else v.ctypes.data for v in vb])
    states = np.zeros((k * (k + 1) // 2, 6), dtype=np.float64)
    flags = np.zeros(k * (k + 1) // 2, dtype=np.uint8)
    L.check(L.lib().dq_diag_corrmat_host(cols, vptr, None if wb is None else wb.ctypes.data, k, n, max_ranges,
                                         states.ctypes.data, flags.ctypes.data))
    return states, flags


def host_state(d, states, i, j, k):
    row = states[pair_index(i, j, k)]
    return None if row[0] == 0.0 else d.CorrelationState(*[float(v) for v in row])


def case_host_mirror(case, keep=None, max_ranges=0):
    valid = [case.valid[i] if case.has_nulls(i) else None for i in range(case.k)]
    return host_corrmat(case.values, valid, keep, max_ranges)
