"""The lane-mask loop of the fast scan (dq_scan_fast.hip: a wave reads its 512 validity bits as
eight 64-bit lane masks with one scalar load, and a NULL row is not executed).

Every case builds its device columns by hand, so that the bitmap tensor has an exact size and a
chosen byte alignment and the value buffer holds garbage under NULL rows; runs statistics + HLL +
one predicate, HLL only and predicate only, on an int64 and an fp64 column, with DQ_SCAN_MAX_BLOCKS
1 or 3 so that small tables loop; asserts from dq_diag_plan_lanemask which loop ran; checks every
state against the oracle as the other scan tests do (scan_plans.check_all: counts, int64 sums, min,
max, predicate counts and HLL words exact, the fp64 sum / mean / m2 within test_gpu_parity's bar);
and requires the exact kinds to equal the stand-in loop's (DQ_SCAN_LANEMASK=0) bit for bit.

DQ_SCAN_LANEMASK=2 selects the loop for every variant, so the predicate-only kernels run it here
whatever the default selection keeps for them; test_default_selection pins the default."""
import math
from collections import OrderedDict

import numpy as np
import pytest

import deequ_amd as d
import pyoracle as O
import scan_plans as S
from deequ_amd import _lib as L
from deequ_amd.table import Column, Table

pytestmark = pytest.mark.gpu

CHUNK = 2048
BIG = 14 * CHUNK + 77            # 28 749 rows: 15 / 5 chunks per block with 1 / 3 blocks
ROW = 15000                      # block 1, iteration 2 of three 10240-row blocks; iteration 7 of one block
INT64_MIN = -(2 ** 63)
_TABLES = {}


# ------------------------------------------------------------------------------ tables
def _word_shapes(n, rng):
    """valid[r] with every 64-row word one of: all NULL, all valid, only lane 0, only lane 63,
    alternating, 5 % random NULLs -- in turn, so every wave of every iteration meets each."""
    valid = np.zeros(n, dtype=bool)
    for w in range((n + 63) // 64):
        word = np.zeros(64, dtype=bool)
        shape = w % 6
        if shape == 1:
            word[:] = True
        elif shape == 2:
            word[0] = True
        elif shape == 3:
            word[63] = True
        elif shape == 4:
            word[::2] = True
        elif shape == 5:
            word[:] = rng.random(64) >= 0.05
        valid[w * 64:(w + 1) * 64] = word[:n - w * 64]
    return valid


def _random_nulls(n, rng):
    return rng.random(n) >= 0.05


class Case:
    """A table in three forms: the oracle's (None for NULL), the raw value buffers (garbage under
    NULL), and device columns built on demand with the bitmap at a chosen byte of its allocation."""

    def __init__(self, key, n, valid, ints, floats, bitmap=True):
        self.n = n
        self.valid = valid if bitmap else np.ones(n, dtype=bool)
        self.bitmap = bitmap
        self.raw = {"x": np.asarray(ints, dtype=np.int64), "f": np.asarray(floats, dtype=np.float64)}
        spec = {"x": ["int64", [int(v) if ok else None for v, ok in zip(self.raw["x"], self.valid)]],
                "f": ["float64", [float(v) if ok else None for v, ok in zip(self.raw["f"], self.valid)]]}
        self.tbl = S.Tbl(key, spec)  # (.ot for the oracle; its own device copy is not used)
        self._dev = {}

    def device(self, byte=0):
        """Device table whose bitmap tensors are exactly (n + 7) // 8 bytes, starting at byte
        `byte` of their allocation."""
        import torch
        if byte not in self._dev:
            dev = torch.device("cuda", 0)
            bits = np.packbits(self.valid, bitorder="little")
            assert len(bits) == (self.n + 7) // 8
            cols = OrderedDict()
            for name, dtype in (("x", "int64"), ("f", "float64")):
                validity = None
                if self.bitmap:
                    if byte == 0:
                        validity = torch.from_numpy(bits.copy()).to(dev)
                    else:
                        buf = torch.zeros(len(bits) + byte, dtype=torch.uint8, device=dev)
                        validity = buf[byte:]
                        validity.copy_(torch.from_numpy(bits.copy()))
                    assert validity.numel() == (self.n + 7) // 8 and validity.data_ptr() % 4 == byte % 4
                cols[name] = Column(dtype, self.n, torch.from_numpy(self.raw[name].copy()).to(dev), validity,
                                    device=True)
            self._dev[byte] = Table(cols)
        return self._dev[byte]


def _hash_min_garbage(values, valid):
    """An int64 whose HLL rank beats every valid value's in its register (the oracle's hash): left
    under a NULL row, it would change the sketch if the row were hashed into it."""
    regs = O.hll_registers([int(v) for v, ok in zip(values, valid) if ok], "int64")
    for g in range(1, 1 << 20):
        idx, pw = O.hll_index_and_rank(O.spark_hash(g, "int64"))
        if pw > regs[idx] + 1:
            return g
    raise AssertionError("no candidate")


def _f64_hash_min_garbage(values, valid):
    regs = O.hll_registers([float(v) for v, ok in zip(values, valid) if ok], "float64")
    for g in range(1, 1 << 20):
        idx, pw = O.hll_index_and_rank(O.spark_hash(g + 0.5, "float64"))
        if pw > regs[idx] + 1:
            return g + 0.5
    raise AssertionError("no candidate")


def _values(n, rng):
    return rng.integers(-2 ** 40, 2 ** 40, n), rng.normal(1e3, 1e2, n)


def cases():
    if _TABLES:
        return _TABLES
    rng = np.random.default_rng(20261021)
    for n in (2047, 2048, 2049, 3 * CHUNK + 77):
        ints, floats = _values(n, rng)
        _TABLES["shapes-%d" % n] = Case("lm-shapes-%d" % n, n, _word_shapes(n, rng), ints, floats)
    n = 3 * CHUNK + 77
    ints, floats = _values(n, rng)
    _TABLES["nobitmap"] = Case("lm-nobitmap", n, None, ints, floats, bitmap=False)
    valid = _random_nulls(n, rng)
    valid[:CHUNK] = False  # the probe finds no c for any wave of the block
    _TABLES["nullhead"] = Case("lm-nullhead", n, valid, ints, floats)
    # 5 % random NULLs with garbage under them
    ints, floats = _values(BIG, rng)
    valid = _random_nulls(BIG, rng)
    valid[[ROW, ROW + 1]] = True
    nulls = np.flatnonzero(~valid)
    for k, g in enumerate((math.nan, math.inf, -math.inf, 1e308)):
        floats[nulls[k::7][:40]] = g          # (spread over the blocks and iterations)
    for k, g in enumerate((2 ** 62, INT64_MIN)):
        ints[nulls[k::5][:40]] = g
    ints[nulls[-1]] = _hash_min_garbage(ints, valid)
    floats[nulls[-1]] = _f64_hash_min_garbage(floats, valid)
    _TABLES["garbage"] = Case("lm-garbage", BIG, valid, ints, floats)
    # a selected NaN and a selected |x| >= 2^51 in iteration 2 of a block
    ints, floats = ints.copy(), floats.copy()
    floats[ROW] = math.nan
    ints[ROW] = 2 ** 51 + 12345
    ints[ROW + 1] = -(2 ** 53) - 1
    _TABLES["special"] = Case("lm-special", BIG, valid, ints, floats)
    return _TABLES


# ------------------------------------------------------------------------------ plans
PRED = {"x": d.Compliance("px", "x > 5"), "f": d.Compliance("pf", "f < 1000.5")}


def plans(c):
    return {"both": S.stats(c) + S.hll(c) + [PRED[c]], "hll": S.hll(c), "pred": [PRED[c]]}


def run(monkeypatch, analyzers, table, cap, lanemask):
    """scan_plans.run_plan, with dq_diag_plan_lanemask read from the same plan before it closes."""
    seen = {}
    real = L.diag_plan_groups

    def spy(handle):
        seen["lm"] = L.diag_plan_lanemask(handle)
        return real(handle)

    env = {"DQ_SCAN_MAX_BLOCKS": cap, "DQ_SCAN_ROUNDS": None, "DQ_SCAN_FAST": None, "DQ_SCAN_LANEMASK": lanemask}
    with monkeypatch.context() as m:
        m.setattr(L, "diag_plan_groups", spy)
        states, groups, _ = S.run_plan(analyzers, table, monkeypatch, env)
    assert groups and all(g[0] == 2 and g[4] == cap for g in groups), groups  # the fast kernel, capped
    return states, seen["lm"]


def check_case(monkeypatch, case, cap, byte=0, expect_lanemask=True, skip=()):
    for c in ("x", "f"):
        for name, an in plans(c).items():
            got, lm = run(monkeypatch, an, case.device(byte), cap, "2")
            assert lm and all(v == expect_lanemask for v in lm), (name, c, lm)
            old, lm0 = run(monkeypatch, an, case.device(byte), cap, "0")
            assert lm0 and not any(lm0), (name, c, lm0)
            for a in an:
                if (type(a), c) in skip:
                    continue
                S.check(a, got[a], case.tbl)
                S.check(a, old[a], case.tbl)
                if S.is_exact(a, case.tbl):
                    assert got[a] == old[a], (a, got[a], old[a])


@pytest.mark.parametrize("n", (2047, 2048, 2049, 3 * CHUNK + 77))
def test_word_shapes(gpu, monkeypatch, n):
    """Tail only, exactly one iteration (a bitmap of exactly n / 8 bytes), one iteration and a
    one-row tail, three iterations and a tail: every shape of mask word in every wave."""
    check_case(monkeypatch, cases()["shapes-%d" % n], 1)


@pytest.mark.parametrize("key", ("nobitmap", "nullhead"))
def test_no_bitmap_and_no_shift(gpu, monkeypatch, key):
    check_case(monkeypatch, cases()[key], 1)


@pytest.mark.parametrize("cap", (1, 3))
def test_garbage_under_null(gpu, monkeypatch, cap):
    """NaN, +-Inf, 1e308, 2^62, INT64_MIN and a hash that would win its register, all in NULL
    slots: none of them may reach a statistic, the exact redo or the sketch."""
    check_case(monkeypatch, cases()["garbage"], cap)


@pytest.mark.parametrize("byte", (0, 1, 2, 3, 4))
def test_bitmap_alignment(gpu, monkeypatch, byte):
    """The scalar load wants a 4-byte aligned bitmap: any other task keeps the stand-in loop."""
    check_case(monkeypatch, cases()["shapes-%d" % (3 * CHUNK + 77)], 1, byte, expect_lanemask=byte % 4 == 0)


@pytest.mark.parametrize("cap", (1, 3))
def test_selected_special_values(gpu, monkeypatch, cap):
    """A selected NaN (fp64) and selected |x| >= 2^51 (int64: the exact redo) past the first
    iteration of a block, as test_gpu_scan_blocks places them."""
    case = cases()["special"]
    # (a NaN sum / max: asserted below, test_gpu_parity's relative bars do not apply to them)
    check_case(monkeypatch, case, cap, skip={(d.Sum, "f"), (d.Mean, "f"), (d.StandardDeviation, "f"), (d.Maximum, "f")})
    got, lm = run(monkeypatch, plans("f")["both"], case.device(), cap, "2")
    assert all(lm)
    vals = [v for v in case.tbl.spec["f"][1] if v is not None and v == v]
    assert math.isnan(got[d.Maximum("f")].maxValue)
    assert math.isnan(got[d.Sum("f")].sum_value)
    assert got[d.Minimum("f")].minValue == min(vals)


def test_default_selection(gpu, monkeypatch):
    """DQ_SCAN_LANEMASK unset: the variants with HLL take the lane-mask loop."""
    case = cases()["shapes-%d" % (3 * CHUNK + 77)]
    for c in ("x", "f"):
        for name in ("both", "hll"):
            _, lm = run(monkeypatch, plans(c)[name], case.device(), 1, None)
            assert lm and all(lm), (c, name, lm)
