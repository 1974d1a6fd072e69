"""Loop-carried state of every launch of dq_plan_consume, at a small size.

Below a few million rows every block of a scan gets one 2048-row chunk, so a main loop runs once
(int8's, whose iteration covers 4096 rows, not at all) and nothing carried from one iteration to
the next -- the `it > 0` addressing of values and bitmaps, the accumulators, the once-per-iteration
NaN re-test, the bits kernel's second step, a lane's second row in the regex / DataType / length /
Correlation kernels -- is ever exercised.  DQ_SCAN_MAX_BLOCKS caps the blocks per task of every
launch; with 1 or 3 blocks the 28 749-row tables of scan_plans give each block 15 or 5 chunks.  Each
test asserts from dq_diag_plan_groups that the cap took effect and that the loop in question runs at
least twice, checks the states against the references the uncapped tests use, and requires the
exact kinds to equal the uncapped plan's states bit for bit (the fp kinds are each within the bar
of the exact value: block boundaries move, so their last bits may differ)."""
import math
from collections import OrderedDict

import numpy as np
import pytest

import deequ_amd as d
import scan_plans as S
from scan_plans import BITS_ROWS_PER_STEP, BLOCK, CHUNK, CODE, N_ROWS, ROWS_PER_ITER, TYPES

pytestmark = pytest.mark.gpu

CAPS = (1, 3)
ROUNDS = (None, "0")  # DQ_SCAN_ROUNDS unset / 0 (grids from target_blocks instead of the occupancy)
TYPE_OF = {v: k for k, v in CODE.items()}
N_CHUNKS = (N_ROWS + CHUNK - 1) // CHUNK


def _env(cap, rounds=None, fast=None):
    return {"DQ_SCAN_MAX_BLOCKS": cap, "DQ_SCAN_ROUNDS": rounds, "DQ_SCAN_FAST": fast}


def _block_rows(bpt, n=N_ROWS):
    """Rows of a full block and of the last one (dq_scan_common.h chunk_of_block)."""
    per = ((n + CHUNK - 1) // CHUNK + bpt - 1) // bpt * CHUNK
    return per, n - (bpt - 1) * per


def _assert_scan_grids(groups, cap):
    """Every scan group ran `cap` blocks per task, each with at least two main-loop iterations
    (value scans) or two 8192-row steps (the bits kernel)."""
    assert groups
    for kind, ptype, np_, n_tasks, bpt, _ in groups:
        assert bpt == cap, (kind, ptype, np_, bpt)
        for rows in _block_rows(bpt):
            if kind == 0:
                assert -(-rows // BITS_ROWS_PER_STEP) >= 2, rows
            else:
                assert rows >= 2 * ROWS_PER_ITER[TYPE_OF[ptype]], (TYPE_OF[ptype], rows)


def _capped_vs_uncapped(monkeypatch, analyzers, tbl, cap, rounds, fast, want):
    env = _env(cap, rounds, fast)
    states, groups, _ = S.run_plan(analyzers, tbl.dev, monkeypatch, env)
    assert want <= S.keys(groups), (want, S.keys(groups))
    _assert_scan_grids(groups, cap)
    S.check_all(states, tbl)
    free, free_groups, _ = S.run_plan(analyzers, tbl.dev, monkeypatch, _env(None, rounds, fast))
    assert all(g[4] == N_CHUNKS for g in free_groups), free_groups  # one chunk per block
    S.check_all(free, tbl)
    for a in analyzers:
        if S.is_exact(a, tbl):
            assert states[a] == free[a], (a, states[a], free[a])
    return states


@pytest.mark.parametrize("rounds", ROUNDS, ids=["rounds-default", "rounds-0"])
@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("t", TYPES)
def test_value_scans(gpu, monkeypatch, t, cap, rounds):
    """Per type: the plain kernel with one predicate (statistics + HLL) and the EXT kernel with a
    `where` and mask predicates, on both tables."""
    c = "c_" + t
    plain = S.stats(c) + S.hll(c) + [S.compliance(t, 3)]
    _, ext, ext_key = S.ext_plans(t, "both")[2]
    for tbl in S.tables().values():
        _capped_vs_uncapped(monkeypatch, plain, tbl, cap, rounds, "0", {(1, CODE[t], 1)})
        _capped_vs_uncapped(monkeypatch, ext, tbl, cap, rounds, None, {ext_key})


@pytest.mark.parametrize("rounds", ROUNDS, ids=["rounds-default", "rounds-0"])
@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("t", S.FAST_TYPES)
def test_fast_scans(gpu, monkeypatch, t, cap, rounds):
    """Every predicate kind of the fast scan with statistics + HLL, and predicate-only."""
    for flags in ((True, True), (False, False)):
        for _, an, key in S.fast_plans(t, *flags):
            for tbl in S.tables().values():
                _capped_vs_uncapped(monkeypatch, an, tbl, cap, rounds, None, {key})


@pytest.mark.parametrize("rounds", ROUNDS, ids=["rounds-default", "rounds-0"])
@pytest.mark.parametrize("cap", CAPS)
def test_bits_scan(gpu, monkeypatch, cap, rounds):
    for tbl in S.tables().values():
        _capped_vs_uncapped(monkeypatch, S.bits_analyzers(), tbl, cap, rounds, None, {(0, 0, 0)})


# ------------------------------------------------------------------------------ special values
_SPECIAL = {}
ROW = 15000                 # block 1, iteration 2 of three 10240-row blocks; iteration 7 of one block
PROBE_ROWS = (0, 10240, 20480)  # the first row of each of three blocks: wave 0's first probe


def _special():
    """NaN, +Inf with -Inf in one lane's iteration, -0.0, int64 extremes, and outliers on probe rows,
    each in a column of its own (5 % NULLs elsewhere), and a filter column that drops the NaN row."""
    if not _SPECIAL:
        rng = np.random.default_rng(77)
        base = rng.normal(1e3, 1e2, N_ROWS)
        null = rng.random(N_ROWS) < 0.05
        null[[ROW, ROW + 1, ROW + 4096] + list(PROBE_ROWS)] = False

        def col(vals, dtype, put):
            v = [None if m else x for x, m in zip(vals, null)]
            for r, x in put.items():
                v[r] = x
            return [dtype, v]

        f32 = base.astype(np.float32).astype(np.float64).tolist()
        spec = {
            "f_nan": col(base.tolist(), "float64", {ROW: math.nan}),
            "f_inf": col(base.tolist(), "float64", {ROW: math.inf, ROW + 1: -math.inf}),
            "g_nan": col(f32, "float32", {ROW: math.nan}),
            "g_inf": col(f32, "float32", {ROW: math.inf, ROW + 1: -math.inf}),
            "f_nz": col(np.abs(base - 1e3).tolist(), "float64", {ROW: -0.0, ROW + 4096: 0.0}),
            "x_ext": col(rng.integers(-2 ** 40, 2 ** 40, N_ROWS).tolist(), "int64",
                         {ROW: 2 ** 63 - 1, ROW + 1: 2 ** 63 - 1, ROW + 4096: -(2 ** 63)}),
            "f_out": col(base.tolist(), "float64", {r: 1e15 for r in PROBE_ROWS}),
            "keep": ["int64", [0 if r == ROW else 1 for r in range(N_ROWS)]],
        }
        _SPECIAL["t"] = S.Tbl("special", spec)
    return _SPECIAL["t"]


def _nan_checks(states, c, tbl):
    vals = [v for v in tbl.spec[c][1] if v is not None and v == v]
    assert math.isnan(states[d.Maximum(c)].maxValue)          # a selected NaN wins max
    assert states[d.Minimum(c)].minValue == min(vals)
    assert math.isnan(states[d.Sum(c)].sum_value)
    w = "keep > 0"                                             # the NaN on a row the filter drops
    for a in (d.Maximum(c, w), d.Minimum(c, w), d.Sum(c, w)):
        S.check(a, states[a], tbl)
    assert not math.isnan(states[d.Sum(c, w)].sum_value)


def _inf_checks(states, c, tbl):
    assert states[d.Maximum(c)].maxValue == math.inf            # Σd is NaN, no value is
    assert states[d.Minimum(c)].minValue == -math.inf
    assert math.isnan(states[d.Sum(c)].sum_value)


@pytest.mark.parametrize("fast", [None, "0"], ids=["fast-on", "fast-off"])
@pytest.mark.parametrize("cap", (None,) + CAPS, ids=["uncapped", "1-block", "3-blocks"])
def test_special_values_past_the_first_iteration(gpu, monkeypatch, cap, fast):
    tbl = _special()
    env = _env(cap, None, fast)

    def run(an):
        states, groups, _ = S.run_plan(an, tbl.dev, monkeypatch, env)
        if cap:
            _assert_scan_grids(groups, cap)
        return states

    for c, special in (("f_nan", _nan_checks), ("g_nan", _nan_checks), ("f_inf", _inf_checks), ("g_inf", _inf_checks)):
        an = S.stats(c) + S.hll(c) + [d.Compliance("p", "%s > 1000" % c), d.Completeness(c)]
        if special is _nan_checks:
            an += [d.Maximum(c, "keep > 0"), d.Minimum(c, "keep > 0"), d.Sum(c, "keep > 0")]
        states = run(an)
        special(states, c, tbl)
        for a in (d.ApproxCountDistinct(c), d.Compliance("p", "%s > 1000" % c), d.Completeness(c), d.Minimum(c),
                  d.Maximum(c)):
            S.check(a, states[a], tbl)
    # -0.0 / 0.0, the int64 extremes (the sum wraps as Spark's LongType sum does), and outliers on
    # the rows the moments' shift is probed from (the cancellation guard redoes the block)
    for c, an in (("f_nz", S.stats("f_nz") + S.hll("f_nz") + [d.Compliance("z", "f_nz = 0")]),
                  ("x_ext", [d.Sum("x_ext"), d.Mean("x_ext"), d.Minimum("x_ext"), d.Maximum("x_ext"),
                             d.ApproxCountDistinct("x_ext"), d.Compliance("x", "x_ext > 3.5e0")]),
                  ("x_ext", [d.Sum("x_ext"), d.Minimum("x_ext"), d.Compliance("x", "x_ext >= 9223372036854775807")]),
                  ("f_out", S.stats("f_out") + [d.Compliance("o", "f_out < 1e15")])):
        S.check_all(run(an), tbl)


# ------------------------------------------------------------ every other launch the cap reaches
def _rows_per_lane(bpt, n=N_ROWS):
    """Rows the busiest lane of a row-per-lane kernel walks (per_block = ceil(n / blocks))."""
    return -(-(-(-n // bpt)) // BLOCK)


def _launch(launches, name, cap, per_chunk):
    bpt = launches[name]
    assert bpt == cap, (name, launches)
    if per_chunk:  # blocks walk whole chunks, a lane a row of every 256
        assert min(_block_rows(bpt)) >= 2 * CHUNK
    else:
        assert _rows_per_lane(bpt) >= 2


_PATTERN = {}


def _pattern_table():
    import test_gpu_pattern_match as PM
    if not _PATTERN:
        vals, idx = PM.rows(N_ROWS, seed=N_ROWS)
        ints = np.random.default_rng(3).integers(0, 8, N_ROWS)
        _PATTERN["t"] = (d.Table.from_pydict({"s": ("string", vals), "i": ("int64", ints.tolist())}).to_device(0),
                         idx, ints > 3)
    return _PATTERN["t"]


@pytest.mark.parametrize("cap", CAPS)
def test_pattern_match(gpu, monkeypatch, cap):
    """Three patterns of pattern_cases.PATTERNS, with and without a where, against its oracle."""
    import test_gpu_pattern_match as PM
    table, idx, sel = _pattern_table()
    an = [d.PatternMatch("s", p, w) for p in PM.PATS for w in (None, "i > 3")]
    got = {}
    for k in (cap, None):
        states, _, launches = S.run_plan(an, table, monkeypatch, _env(k))
        if k:
            _launch(launches, "regex", cap, per_chunk=False)
        for a in an:
            m, c = PM.expect(a.pattern, idx, sel if a.where else None)
            assert states[a] == d.NumMatchesAndCount(m, c), (a, states[a], m, c)
        got[k] = states
    assert got[cap] == got[None]


@pytest.mark.parametrize("cap", CAPS)
def test_string_kernels(gpu, monkeypatch, cap):
    """The fused string pass (HLL + DataType of one column), and the HLL, DataType and length
    kernels on their own, against pyoracle."""
    import pyoracle as O
    tbl = S.tables()["plain"]
    c = "s_mixed"
    acd, dt = d.ApproxCountDistinct(c, S.WHERE), d.DataType(c, S.WHERE)
    for an, name, per_chunk in (([acd, dt], "string_pass", True), ([acd], "hll", True), ([dt], "datatype", False),
                                ([d.MinLength(c, S.WHERE), d.MaxLength(c, S.WHERE)], "strlen", False),
                                ([d.ApproxCountDistinct("c_string"), d.DataType("c_string")], "string_pass", True)):
        capped, _, launches = S.run_plan(an, tbl.dev, monkeypatch, _env(cap))
        _launch(launches, name, cap, per_chunk)
        free, _, _ = S.run_plan(an, tbl.dev, monkeypatch, _env(None))
        for a in an:
            if isinstance(a, d.DataType):
                assert capped[a].counts() == O.datatype_state(tbl.ot, a.column, a.where), a
            else:
                S.check(a, capped[a], tbl)
            assert capped[a] == free[a], a


@pytest.mark.parametrize("cap", CAPS)
def test_hll_of_a_bool_column(gpu, monkeypatch, cap):
    tbl = S.tables()["plain"]
    an = [d.ApproxCountDistinct("c_bool"), d.ApproxCountDistinct("c_bool", S.WHERE)]
    states, _, launches = S.run_plan(an, tbl.dev, monkeypatch, _env(cap))
    assert launches["hll"] == cap
    for rows in _block_rows(cap):  # 32 rows per lane per step
        assert -(-rows // BITS_ROWS_PER_STEP) >= 2
    S.check_all(states, tbl)


@pytest.mark.parametrize("cap", CAPS)
def test_correlation(gpu, monkeypatch, cap):
    """Against the exact rational moments (test_gpu_parity._check_correlation)."""
    for tbl in S.tables().values():
        an = [d.Correlation("c_int64", "c_float64"), d.Correlation("c_float32", "c_int8", S.WHERE)]
        states, _, launches = S.run_plan(an, tbl.dev, monkeypatch, _env(cap))
        _launch(launches, "corr", cap, per_chunk=False)
        S.check_all(states, tbl)


_DECIMAL = {}


@pytest.mark.parametrize("rounds", ROUNDS, ids=["rounds-default", "rounds-0"])
@pytest.mark.parametrize("cap", CAPS)
def test_decimal_scan(gpu, monkeypatch, cap, rounds):
    """One decimal(38,10) column against Python's exact arithmetic (decimal_cases)."""
    import test_gpu_decimal as TD
    if not _DECIMAL:
        values = TD._moderate(N_ROWS, 41)
        _DECIMAL["e"] = TD._expect(N_ROWS, [v for v in values if v is not None], 38, 10)
        _DECIMAL["t"] = d.Table(OrderedDict([("m", TD._column(values, 38, 10))])).to_device(0)
    an = TD._stats("m")
    got = {}
    for k in (cap, None):
        states, _, launches = S.run_plan(an, _DECIMAL["t"], monkeypatch, _env(k, rounds))
        if k:
            _launch(launches, "dec", cap, per_chunk=True)
        TD._check([states[a] for a in an], _DECIMAL["e"], ("decimal(38,10)", k, rounds))
        got[k] = states
    for a in an:
        if not isinstance(a, d.StandardDeviation):
            assert got[cap][a] == got[None][a], a
