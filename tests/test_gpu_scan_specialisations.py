"""Every kernel of the fused scan's launch tables against the oracle, at a size where its main
loop runs, selected by the narrow plans a real Check produces.

dq_plan_create groups scan tasks by (kind, value type, np) and each group gets its own kernel:
dq_scan_values_kernel<T, NP, EXT> (6 types x NP in {0,1,2,3,4,8}, plus one EXT kernel per type),
dq_scan_fast_kernel<T, PK, STATS, HLL> (int64 / fp64) and dq_scan_bits_kernel.  Which one a column
gets depends on what else the plan asks of it, so the plans here ask for statistics only, HLL only,
both, or predicates only, with 0..8 inline predicates of every form fast_form recognises, a `where`,
mask predicates, and more predicates than one task holds (the sibling task).  dq_diag_plan_groups
says which kernel each plan ran; the last test asserts that the plans of this module reach every
instantiation (UNIVERSE), so a new specialisation fails the suite until a plan covers it.

Tables (scan_plans.tables): 14 * 2048 + 77 rows, one column per type, 5 % NULLs, and a copy whose
first 5000 rows are NULL in every numeric column (the masked loops of the fast scan).  References:
test_gpu_parity._check_state (pyoracle, exact Fraction / fsum values) -- bit-exact counts,
Compliance, Min / Max, integral Sum / Mean and HLL words; fp64 Sum / Mean / StdDev within 1e-12 of
the exact value."""
import numpy as np
import pytest

import deequ_amd as d
import scan_plans as S
from scan_plans import CODE, MODES, TYPES

pytestmark = pytest.mark.gpu

I8, I16, I32, I64, F32, F64 = (CODE[t] for t in TYPES)
GENERAL_NP = (-1, 0, 1, 2, 3, 4, 8)  # -1 = <T, kMaxPreds, true> (EXT); 5..8 predicates share NP = 8
# fast variants: predicate kind (0 none, 1 PK_LT_I, 2 PK_EQ_I, 3 PK_LT_F, 4 PK_EQ_F) | 8 STATS | 16 HLL
FAST_INT64 = (8, 16, 24, 1, 9, 17, 25, 2, 10, 18, 26, 3, 11, 19, 27, 4, 12, 20, 28)
FAST_FP64 = (8, 16, 24, 3, 11, 19, 27, 4, 12, 20, 28)  # (fp columns compare as fp: no PK_*_I)
UNIVERSE = ({(0, 0, 0)} | {(1, t, np_) for t in (I8, I16, I32, I64, F32, F64) for np_ in GENERAL_NP} |
            {(2, I64, v) for v in FAST_INT64} | {(2, F64, v) for v in FAST_FP64})
# instantiated but selected by no plan
UNREACHABLE = {
    (2, I64, 0): "dq_scan_fast_kernel<int64_t, PK_NONE, false, false>: a task reads values (TF_VALUES) only "
                 "for statistics, HLL or a compare predicate, and a sibling task always holds a predicate",
    (2, F64, 0): "dq_scan_fast_kernel<double, PK_NONE, false, false>: as for int64",
}
assert len(UNIVERSE) == 1 + 42 + 30 and not (set(UNREACHABLE) & UNIVERSE)


def _run(monkeypatch, env, analyzers, want, tbl):
    states, groups, _ = S.run_plan(analyzers, tbl.dev, monkeypatch, env)
    got = S.keys(groups)
    assert want <= got, (want, got, [str(a) for a in analyzers])
    assert got <= UNIVERSE, got - UNIVERSE
    S.check_all(states, tbl)
    return states


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("t", TYPES)
def test_general_kernels(gpu, monkeypatch, t, mode):
    """<T, NP, false> for NP = 0..4 and 8 (5..8 predicates), on both tables; int64 / fp64 with the
    fast scan on (the plans it declines) and off."""
    for env, an, key in S.general_plans(t, mode):
        for tbl in S.tables().values():
            _run(monkeypatch, env, an, {key}, tbl)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("t", TYPES)
def test_ext_kernels(gpu, monkeypatch, t, mode):
    """<T, kMaxPreds, true>: by a `where`, by mask predicates, by both."""
    for env, an, key in S.ext_plans(t, mode):
        for tbl in S.tables().values():
            _run(monkeypatch, env, an, {key}, tbl)


@pytest.mark.parametrize("flags", S.FAST_FLAGS, ids=["stats", "hll", "stats+hll", "predicate-only"])
@pytest.mark.parametrize("t", S.FAST_TYPES)
def test_fast_kernels(gpu, monkeypatch, t, flags):
    """All 30 reachable dq_scan_fast_kernel variants, every operator, on both tables."""
    for env, an, key in S.fast_plans(t, *flags):
        assert key[0] == 2
        for tbl in S.tables().values():
            _run(monkeypatch, env, an, {key}, tbl)


@pytest.mark.parametrize("where", [None, S.WHERE], ids=["all-rows", "where"])
@pytest.mark.parametrize("n_preds", [9, 10, 11])
@pytest.mark.parametrize("t", ["int32", "int64", "float64"])
def test_more_predicates_than_a_task_holds(gpu, monkeypatch, t, n_preds, where):
    """The ninth predicate on one (column, where) opens a sibling task without STATS / HLL: every
    Compliance is right, and the column's statistics and HLL are those of the plan without
    predicates (bit for bit for the exact kinds; StandardDeviation and fp Sum / Mean within the bar
    of the exact value in both plans)."""
    env, an, want = S.sibling_plans(t, n_preds, where)
    c = "c_" + t
    alone = S.stats(c, where) + S.hll(c, where)
    for tbl in S.tables().values():
        full = _run(monkeypatch, env, an, want, tbl)
        ref = _run(monkeypatch, env, alone, set(), tbl)
        assert sum(isinstance(a, d.Compliance) for a in full) == n_preds
        for a in alone:
            if S.is_exact(a, tbl):
                assert full[a] == ref[a], (a, full[a], ref[a])


def test_bits_kernel(gpu, monkeypatch):
    for tbl in S.tables().values():
        _run(monkeypatch, {}, S.bits_analyzers(), {(0, 0, 0)}, tbl)


# ------------------------------------------------------------------- order and composition
def _suite():
    out = []
    for t in TYPES:
        c = "c_" + t
        out += [d.Completeness(c), d.Sum(c), d.StandardDeviation(c), d.Maximum(c), d.ApproxCountDistinct(c),
                S.compliance(t, 2)]
    out += [d.Compliance(m, m) for m in S.MASKS]
    for t in ("int8", "int32", "float64"):
        c = "c_" + t
        out += [d.Sum(c, S.WHERE), d.Minimum(c, S.WHERE), d.ApproxCountDistinct(c, S.WHERE)]
    out += [d.Size(), d.Size(S.WHERE), d.Compliance(S.MASKS[0], S.MASKS[0], S.WHERE),
            d.Compliance(S.MASKS[3], S.MASKS[3], S.WHERE), d.Compliance("t", "TRUE"), d.Compliance("b", "c_bool"),
            d.Completeness("c_string"), d.ApproxCountDistinct("c_string"), d.ApproxCountDistinct("c_bool"),
            d.MinLength("c_string"), d.MaxLength("c_string")]
    assert len(out) == 60 and len(set(out)) == 60
    return out


_REFERENCE = {}


def _reference(monkeypatch, tbl):
    if tbl.key not in _REFERENCE:
        states, _, _ = S.run_plan(_suite(), tbl.dev, monkeypatch)
        S.check_all(states, tbl)
        _REFERENCE[tbl.key] = states
    return _REFERENCE[tbl.key]


@pytest.mark.parametrize("seed", range(20))
def test_order_and_composition(gpu, monkeypatch, seed):
    """Permutations and random subsets of one 60-analyzer suite: op order decides which column's
    task a mask predicate lands on (so which kernel becomes EXT) and what shares a group; every
    state must equal the reference plan's -- bit for bit for the exact kinds, both within the bar of
    the exact value for the fp kinds."""
    rng = np.random.default_rng(900 + seed)
    suite = _suite()
    order = [suite[i] for i in rng.permutation(len(suite))]
    if seed % 2:
        order = order[:int(rng.integers(8, 50))]
    tbl = S.tables()["plain" if seed % 4 < 2 else "prefix"]
    ref = _reference(monkeypatch, tbl)
    states, groups, _ = S.run_plan(order, tbl.dev, monkeypatch)
    assert S.keys(groups) <= UNIVERSE
    S.check_all(states, tbl)
    for a in order:
        if S.is_exact(a, tbl):
            assert states[a] == ref[a], (a, states[a], ref[a])


def test_mask_predicate_lands_on_the_last_task_with_its_filter(gpu, monkeypatch):
    """The same three analyzers in two orders: the mask predicate makes the kernel of whichever
    column's task came last EXT, and the other column keeps its plain kernel."""
    tbl = S.tables()["plain"]
    a8, a32 = d.Sum("c_int8"), d.Sum("c_int32")
    m = d.Compliance(S.MASKS[0], S.MASKS[0])
    for order, ext, plain in (([a8, a32, m], I32, I8), ([a32, a8, m], I8, I32), ([a8, m, a32], I8, I32)):
        _run(monkeypatch, {}, order, {(1, ext, -1), (1, plain, 0)}, tbl)


# ------------------------------------------------------------------------------- coverage
def test_every_specialisation_is_covered(gpu, monkeypatch):
    """The union of dq_diag_plan_groups over every plan of this module (created here, not
    consumed) is the set of instantiations of the two launch tables, minus UNREACHABLE."""
    host = S.tables()["plain"].host
    seen = set()
    for env, an in S.all_plan_specs():
        _, groups, _ = S.run_plan(an, host, monkeypatch, env, consume=False)
        seen |= S.keys(groups)
    assert seen == UNIVERSE, (sorted(UNIVERSE - seen), sorted(seen - UNIVERSE))
