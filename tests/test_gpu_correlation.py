"""Correlation where the kernel's shift probe finds nothing, or something it must not use.

dq_corr_kernel (dq_pair.hip) sums dx, dy, dx², dy², dx*dy about a wave-uniform shift -- the first
selected pair with finite values among the wave's rows -- and forms xMk = Σdx² - (Σdx)²/n and
ck = Σdxdy - ΣdxΣdy/n.  That difference cancels (relative rounding ~ eps * Σdx² / xMk) when the
shift lies far from the data, which Spark's per-row Corr update (StatefulCorrelation.scala:24-49)
never does.  Two ways to get there:

* no shift at all: a workgroup whose first 1024 rows (four probes of each wave) are all
  unselected -- NULL in x, NULL in y, or a `where` that is not TRUE -- followed by thousands of
  selected rows whose mean is large against their spread.  A workgroup only covers that many
  rows when the grid is small against the table (dq_plan_consume: blocks per task =
  min(max(256, 8 * CUs) / tasks, ceil(n / 256))), so every such case recomputes that grid from its
  own n and task count and FAILS if its premise does not hold on the card it runs on;
* a shift that is an outlier (a +-1e8 sentinel on the probe rows), or probe rows that are
  selected but not finite.

Reference: the exact rational state (n, xAvg, yAvg, ck, xMk, yMk) -- Fractions of the doubles on
host-sized tables, integer sums about the offset (on the GPU, in int64) on device-sized ones.
Bar: n bit-exact; xAvg, yAvg, xMk, yMk within 1e-12 of the exact value, ck within 1e-12 of
sqrt(xMk * yMk); no absolute slack, so an exact 0 must be 0.0 and the metric is NaN exactly when
the oracle's is.  Every host-sized case also holds pyoracle.correlation_state (Spark's per-row
update) to the same bar: inputs it cannot meet would prove nothing about the kernel."""
import math
import zlib
from fractions import Fraction

import numpy as np
import pytest

import deequ_amd as d
import pyoracle as O

pytestmark = pytest.mark.gpu

REL_TOL = 1e-12
PERIOD = 4096  # rows r with r mod PERIOD < PERIOD / 2 are unselected

_NP = {"int16": np.int16, "int32": np.int32, "int64": np.int64, "float32": np.float32, "float64": np.float64}

WHERES4 = [None, "g2 > 0", "g3 > 0", "g2 > 0 AND g3 = 1"]
WHERES8 = WHERES4 + ["g2 >= 1", "g3 = 1", "g2 > 0 OR g3 > 0", "g3 IS NOT NULL"]


# ---------------------------------------------------------------- the launch grid (premise)
def _grid(n, n_corr):
    """(blocks per task, rows per block) of dq_corr_kernel for an n-row batch."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    bpt = min(max(256, 8 * cus) // n_corr, -(-n // 256))
    return bpt, -(-n // bpt)


def _assert_no_shift(sel, n_corr):
    """At least a quarter of the blocks: no selected row among the first 1024 (so no probe finds a
    shift) and at least 2048 selected rows after them."""
    sel = np.asarray(sel, dtype=bool)
    n = len(sel)
    bpt, per_block = _grid(n, n_corr)
    hit = 0
    for r0 in range(0, n, per_block):
        r1 = min(r0 + per_block, n)
        p1 = min(r0 + 1024, r1)
        if not sel[r0:p1].any() and int(sel[p1:r1].sum()) >= 2048:
            hit += 1
    assert 4 * hit >= bpt, "premise: %d of %d blocks (%d rows each) start unselected" % (hit, bpt, per_block)


# ---------------------------------------------------------------- the exact state
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


def _check(label, got, exact, who="kernel"):
    assert got is not None, label
    err = _errors(got, exact)
    print("%-6s %-40s %s" % (who, label, " ".join("%s=%.2e" % kv for kv in err.items())))
    assert got.n == float(exact[0]), (who, label, got.n, exact[0])
    for k, v in err.items():
        assert v <= REL_TOL, (who, label, k, v, got)


def _check_metric(label, got, ostate):
    g, o = got.metricValue(), ostate.metric_value()
    assert math.isnan(g) == math.isnan(o), (label, g, o)


# ---------------------------------------------------------------- host tables
def _family(family, rng, n):
    """(x, y) as float64 arrays of exactly representable values."""
    k = rng.integers(-4096, 4097, n)
    j = rng.integers(-512, 513, n)
    if family == "big":          # offset 2^24 against a spread of ~2.4e3
        return 2.0 ** 24 + k, 2.0 ** 22 - 2 * k + j
    if family == "f32":          # integers below 2^24: exact in float32
        return 2.0 ** 20 + k, 2.0 ** 22 - 2 * k + j
    if family == "i16":
        return 30000.0 + k // 8, 2.0 ** 20 + 3 * (k // 8) + j
    if family == "frac":         # 20 significant bits: the squares are still exact
        return 1000 + k / 1024, 500 - 2 * k / 1024 + j / 1024
    if family == "frac_fine":    # 30 significant bits: no square is exactly representable; nearly
        kf = rng.integers(-2 ** 18, 2 ** 18 + 1, n)  # uncorrelated, so ck is small against its scale
        return 1000 + kf / 2.0 ** 20, 2.0 ** 20 + j  # (2^24 + j is beyond the oracle's own accuracy)
    raise ValueError(family)


# (x type, y type, family, the side whose NULLs unselect the prefix)
PAIRS8 = [("int64", "float64", "big", "x"), ("float64", "float64", "big", "y"),
          ("int32", "float32", "big", "x"), ("float64", "int64", "big", "xy"),
          ("int16", "int32", "i16", "y"), ("float32", "float64", "f32", "x"),
          ("float64", "float64", "frac", "x"), ("float64", "int64", "frac_fine", "y")]


def _prefix_keep(n):
    return (np.arange(n) % PERIOD) >= PERIOD // 2


class _Host:
    """A host table, its oracle twin and, per column, the exact doubles."""

    def __init__(self, n):
        self.n = n
        self.cols, self.ocols, self.values, self.valid = {}, {}, {}, {}

    def add(self, name, dtype, values, valid=None):
        arr = np.asarray(values, dtype=np.float64).astype(_NP[dtype])
        assert np.array_equal(arr.astype(np.float64), np.asarray(values, dtype=np.float64)), name
        valid = np.ones(self.n, dtype=bool) if valid is None else valid
        self.cols[name] = d.Column.from_numpy(arr, valid, dtype)
        self.values[name] = arr.astype(np.float64)
        self.valid[name] = valid
        self.ocols[name] = (dtype, arr.tolist())

    def flags(self, keep):
        """g2: 0 on unselected rows; g3: NULL there.  No `where` above selects more than `keep`."""
        self.add("g2", "int64", keep.astype(np.int64))
        self.add("g3", "int64", np.ones(self.n), keep)

    def table(self, rows=slice(None)):
        if rows == slice(None):
            return d.Table(self.cols)
        return d.Table({k: d.Column.from_numpy(c.values[rows], self.valid[k][rows], c.dtype)
                        for k, c in self.cols.items()})

    def selected(self, x, y, keep):
        s = self.valid[x] & self.valid[y] & keep
        return s, self.values[x][s], self.values[y][s]

    def oracle(self, x, y, keep):
        """pyoracle.correlation_state of the pair; rows the `where` leaves out are NULL inputs
        (conditionalSelection), so the oracle sees Spark's row sequence without re-evaluating the
        predicate for each of the plan's tasks."""
        def col(name):
            dtype, vals = self.ocols[name]
            ok = self.valid[name] & keep
            return O.OColumn(dtype, [v if s else None for v, s in zip(vals, ok.tolist())])
        return O.correlation_state({x: col(x), y: col(y)} if x != y else {x: col(x)}, x, y)


def _run_pairs(host, table, pairs, wheres, keep, premise=True, label=""):
    """One plan of len(pairs) * len(wheres) Correlation tasks; every task against the exact state
    of its pair, and the oracle against it once per pair (each `where` selects `keep`)."""
    analyzers = [d.Correlation(x, y, w) for x, y in pairs for w in wheres]
    if premise:
        for x, y in pairs:
            _assert_no_shift(host.selected(x, y, keep)[0], len(analyzers))
    states = d.run_scan(analyzers, table)
    for x, y in pairs:
        _, xs, ys = host.selected(x, y, keep)
        exact = _exact_state(xs, ys)
        ostate = host.oracle(x, y, keep)
        _check("%s %s,%s" % (label, x, y), ostate, exact, who="oracle")
        for w in wheres:
            a = d.Correlation(x, y, w)
            _check("%s %s,%s where %s" % (label, x, y, w), states[a], exact)
            _check_metric((label, x, y, w), states[a], ostate)
    return analyzers, states


def _pairs8_host(n, seed):
    rng = np.random.default_rng(seed)
    keep = _prefix_keep(n)
    host = _Host(n)
    for i, (xt, yt, family, nulls) in enumerate(PAIRS8):
        x, y = _family(family, rng, n)
        host.add("x%d" % i, xt, x, keep if "x" in nulls else None)
        host.add("y%d" % i, yt, y, keep if "y" in nulls else None)
    host.flags(keep)
    return host, keep, [("x%d" % i, "y%d" % i) for i in range(len(PAIRS8))]


# ---------------------------------------------------------------- unselected prefix, device
def _pack_bits(valid):
    import torch
    bits = torch.zeros(valid.numel() // 8, dtype=torch.uint8, device=valid.device)
    vb = valid.view(-1, 8).to(torch.uint8)
    for b in range(8):
        bits |= vb[:, b] << b
    return bits


@pytest.mark.parametrize("data", ["int64-float64", "float64-float64", "int32-float32", "fractional",
                                  "fractional_fine"])
@pytest.mark.parametrize("how", ["null_x", "null_y", "where"])
def test_unselected_prefix_one_task_device(gpu, how, data):
    """2^23 device-resident rows, one task: 2048 blocks of 4096 rows, each starting with 2048
    unselected rows.  x = 2^24 + k, y = 2^22 - 2k + j; "fractional": x = 1000 + k/1024,
    y = 500 + (j - 2k)/1024, whose squares are still exact doubles; "fractional_fine": the same
    over 2^20 with |k| <= 2^18, whose squares are not.  The exact state comes from int64 sums of k
    and j - 2k on the GPU."""
    import torch
    n = 1 << 23
    g = torch.Generator(device="cuda").manual_seed(zlib.crc32((how + data).encode()))
    wide = 64 if data == "fractional_fine" else 1
    k = torch.randint(-4096 * wide, 4096 * wide + 1, (n,), device="cuda", generator=g, dtype=torch.int64)
    j = torch.randint(-512 * wide, 512 * wide + 1, (n,), device="cuda", generator=g, dtype=torch.int64)
    keep = (torch.arange(n, device="cuda") % PERIOD) >= PERIOD // 2
    _assert_no_shift(keep.cpu().numpy(), 1)
    ky = j - 2 * k
    if data.startswith("fractional"):
        xt, yt, cx, cy, scale = "float64", "float64", 1000, 500, 1024 if data == "fractional" else 2 ** 20
    else:
        (xt, yt), cx, cy, scale = data.split("-"), 2 ** 24, 2 ** 22, 1
    tt = {"int32": torch.int32, "int64": torch.int64, "float32": torch.float32, "float64": torch.float64}

    def column(dtype, c, kk, valid):
        if dtype.startswith("int"):
            vals = (kk + c).to(tt[dtype])
        else:
            vals = (c + kk.to(torch.float64) / scale).to(tt[dtype])
        assert bool((vals.to(torch.float64) == c + kk.to(torch.float64) / scale).all())  # exact
        return d.Column(dtype, n, vals.contiguous(), _pack_bits(valid) if valid is not None else None, device=True)
    cols = {"x": column(xt, cx, k, keep if how == "null_x" else None),
            "y": column(yt, cy, ky, keep if how == "null_y" else None)}
    where = None
    if how == "where":
        cols["g"] = d.Column("int64", n, keep.to(torch.int64), None, device=True)
        where = "g > 0"
    z = torch.zeros_like(k)
    kx_s, ky_s = torch.where(keep, k, z), torch.where(keep, ky, z)
    exact = _state_from_sums(int(keep.sum()), cx, scale, cy, scale, int(kx_s.sum()), int(ky_s.sum()),
                             int((kx_s * kx_s).sum()), int((ky_s * ky_s).sum()), int((kx_s * ky_s).sum()))
    a = d.Correlation("x", "y", where)
    torch.cuda.synchronize()  # the library reads the buffers on its plan's own stream
    _check("2^23 %s %s" % (how, data), d.run_scan([a], d.Table(cols))[a], exact)


# ---------------------------------------------------------------- unselected prefix, host batch
def test_unselected_prefix_many_tasks_host(gpu):
    """2^18 rows, 8 column pairs x 4 `where`s in one plan: 64 blocks of 4096 rows per task."""
    n = 1 << 18
    host, keep, pairs = _pairs8_host(n, 2024)
    _run_pairs(host, host.table(), pairs, WHERES4, keep, label="2^18")


@pytest.mark.parametrize("selection", ["no_shift", "all_selected"])
@pytest.mark.parametrize("const", [0.1, 1.0 / 3.0, 2.0 ** 24 + 0.5], ids=["0.1", "third", "2^24+0.5"])
def test_constant_column(gpu, const, selection):
    """A constant x, a constant y, both: xMk / yMk (and ck) are exactly 0 and the metric is NaN, as
    the oracle's -- with no shift (4 pairs x 8 `where`s, blocks of 4096 rows starting unselected) and
    with every row selected."""
    n = 1 << 18
    rng = np.random.default_rng(int(const * 1000) % 9973)
    keep = _prefix_keep(n) if selection == "no_shift" else np.ones(n, dtype=bool)
    x, y = _family("big", rng, n)
    host = _Host(n)
    host.add("cx", "float64", np.full(n, const), keep)
    host.add("cy", "float64", np.full(n, const))
    host.add("vx", "int64", x, keep)
    host.add("vy", "float64", y)
    host.flags(keep)
    pairs = [("cx", "vy"), ("vx", "cy"), ("cx", "cy"), ("vx", "vy")]
    _, states = _run_pairs(host, host.table(), pairs, WHERES8, keep, premise=selection == "no_shift",
                           label="const " + selection)
    for w in WHERES8:
        for (px, py), zero in ((pairs[0], "x"), (pairs[1], "y"), (pairs[2], "xy")):
            st = states[d.Correlation(px, py, w)]
            assert ("x" not in zero or st.xMk == 0.0) and ("y" not in zero or st.yMk == 0.0) and st.ck == 0.0, st
            assert math.isnan(st.metricValue()), st
        assert not math.isnan(states[d.Correlation("vx", "vy", w)].metricValue())


# ---------------------------------------------------------------- the probe finds a bad shift
@pytest.mark.parametrize("layout", ["row0", "every_wave"])
def test_outlier_on_probe_rows(gpu, layout):
    """A +-1e8 value of x on the first probe row: row 0 only, or the first row of every wave."""
    n = 300_000
    rng = np.random.default_rng(zlib.crc32(layout.encode()))
    x = np.rint(rng.normal(0, 1, n) * 1024) / 1024
    y = np.rint((0.5 * x + rng.normal(0, 1, n)) * 1024) / 1024
    if layout == "row0":
        x[0] = 1e8
    else:
        rows = np.arange(0, n, 64)
        x[rows] = np.where((rows // 64) % 3 != 0, 1e8, -1e8)
    host = _Host(n)
    host.add("x", "float64", x)
    host.add("y", "float64", y)
    keep = np.ones(n, dtype=bool)
    _run_pairs(host, host.table(), [("x", "y")], [None], keep, premise=False, label="outlier " + layout)
    _run_pairs(host, host.table().to_device(0), [("y", "x")], [None], keep, premise=False,
               label="outlier(y) " + layout)


def test_non_finite_probe_rows(gpu):
    """The first 1024 rows of every 4096 hold +-Inf in x: valid and selected, so they count, but
    no probe may take one as the shift.  n and the metric's NaN-ness are the oracle's."""
    n = 1 << 18
    rng = np.random.default_rng(99)
    x, y = _family("big", rng, n)
    r = np.arange(n)
    inf_rows = (r % PERIOD) < 1024
    x[inf_rows] = np.where(r[inf_rows] % 2 == 0, np.inf, -np.inf)
    cols = {"y": d.Column.from_numpy(y, None, "float64"), "g2": d.Column.from_numpy(np.ones(n, dtype=np.int64))}
    cols["g3"] = cols["g2"]
    for i in range(8):  # 8 x 4 tasks over the same buffers: blocks of 4096 rows
        cols["x%d" % i] = d.Column.from_numpy(x, None, "float64")
    analyzers = [d.Correlation("x%d" % i, "y", w) for i in range(8) for w in WHERES4]
    assert _grid(n, len(analyzers))[1] == PERIOD
    states = d.run_scan(analyzers, d.Table(cols))
    ostate = O.correlation_state({"x": O.OColumn("float64", x.tolist()), "y": O.OColumn("float64", y.tolist())},
                                 "x", "y")
    assert ostate.n == float(n) and math.isnan(ostate.metric_value())
    for a in analyzers:
        assert states[a].n == ostate.n, a
        _check_metric(a, states[a], ostate)


# ---------------------------------------------------------------- ragged sizes
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1023, 1024, 1025, 4097])
def test_ragged_sizes_last_rows_selected(gpu, n):
    """Everything NULL but the last row, then but two rows (the last and the middle one).  One
    selected pair: xMk = yMk = ck = 0 exactly."""
    for rows in ([n - 1], [n // 2, n - 1]):
        if len(set(rows)) < len(rows):
            continue  # n = 1 has no second row
        x, y = [None] * n, [None] * n
        for i, r in enumerate(rows):
            x[r], y[r] = 2 ** 24 + 37 * i + 5, 2.0 ** 22 - 0.25 * i
        spec = {"x": ("int64", x), "y": ("float64", y)}
        ot = {k: O.OColumn(t, v) for k, (t, v) in spec.items()}
        xs = np.array([x[r] for r in rows], dtype=np.float64)
        ys = np.array([y[r] for r in rows], dtype=np.float64)
        exact = _exact_state(xs, ys)
        ostate = O.correlation_state(ot, "x", "y")
        _check("ragged n=%d pairs=%d" % (n, len(rows)), ostate, exact, who="oracle")
        a = d.Correlation("x", "y")
        for table in (d.Table.from_pydict(spec), d.Table.from_pydict(spec).to_device(0)):
            st = d.run_scan([a], table)[a]
            _check("ragged n=%d pairs=%d" % (n, len(rows)), st, exact)
            _check_metric((n, rows), st, ostate)
            if len(rows) == 1:
                assert (st.xAvg, st.yAvg, st.ck, st.xMk, st.yMk) == (float(x[n - 1]), y[n - 1], 0.0, 0.0, 0.0), st


# ---------------------------------------------------------------- batches
def test_unselected_prefix_three_batches(gpu):
    """The prefix layout as a PartitionedTable of 2^17 + 2^16 + 2^17 rows, 8 pairs x 8 `where`s (32
    blocks of 4096 rows per task in the outer batches); the middle batch has no selected pair.
    Within the bar of the exact state of the union, and bitwise equal on a second run."""
    n1, n2 = 1 << 17, 1 << 16
    n = 2 * n1 + n2
    host, keep, pairs = _pairs8_host(n, 4711)
    keep = keep & ~((np.arange(n) >= n1) & (np.arange(n) < n1 + n2))
    for name in list(host.cols):  # rebuild the NULL sides and the flags with the middle batch unselected
        if not host.valid[name].all() or name in ("g2", "g3"):
            dtype = host.cols[name].dtype
            vals = keep.astype(np.int64) if name == "g2" else host.values[name]
            host.add(name, dtype, vals, None if name == "g2" else keep)
    n_tasks = len(pairs) * len(WHERES8)
    for x, y in pairs:
        s = host.selected(x, y, keep)[0]
        assert not s[n1:n1 + n2].any()
        _assert_no_shift(s[:n1], n_tasks)
        _assert_no_shift(s[n1 + n2:], n_tasks)
    parts = d.PartitionedTable([host.table(slice(0, n1)), host.table(slice(n1, n1 + n2)),
                                host.table(slice(n1 + n2, n))])
    analyzers, first = _run_pairs(host, parts, pairs, WHERES8, keep, premise=False, label="3 batches")
    again = d.run_scan(analyzers, parts)
    for a in analyzers:
        assert first[a] == again[a], a
