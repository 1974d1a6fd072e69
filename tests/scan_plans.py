"""Shared by test_gpu_scan_specialisations.py and test_gpu_scan_blocks.py: the seeded tables, the
plans that between them select every kernel of the scan launch tables (dq_scan.hip's
launch_values_np, dq_scan_fast.hip's fast_ptr, the bits kernel), the kernel each plan is expected
to get, and a memo around test_gpu_parity._check_state so that hundreds of plans cost one oracle
evaluation per (analyzer, table).

A plan is run through engine.Plan directly (never the plan pool), so the environment knobs read at
plan creation (DQ_SCAN_FAST, DQ_SCAN_MAX_BLOCKS, DQ_SCAN_ROUNDS) hold for exactly that plan, and
dq_diag_plan_groups reports the kernels and grids it ran."""
import numpy as np

import deequ_amd as d
from deequ_amd import _lib as L
from deequ_amd.engine import Plan, op_spec_for
from helpers import oracle_table, random_table

N_ROWS = 14 * 2048 + 77  # 15 chunks, a ragged last one
NULL_PREFIX = 5000       # the second copy: the first waves of the first blocks see no valid value
TYPES = ["int8", "int16", "int32", "int64", "float32", "float64"]
CODE = {t: L.TYPE_CODES[t] for t in TYPES}
FAST_TYPES = ("int64", "float64")
PLANTED = {"int8": 100, "int16": 100, "int32": 100, "int64": 1000000000}  # `c = 1e2` / `c = 1e9` match
PLANT_ROWS = (7, 5003, 12345, 20481, N_ROWS - 3)

WHERE = "c_int32 > 0"
MASKS = ["c_int32 > 5 AND c_float64 < 1000", "c_int8 < 0 OR c_int16 > 0", "c_string IN ('k1', 'k2', 'k77')",
         "NOT (c_float32 >= 1000)"]

# the rows one main-loop iteration of a value scan covers (dq_scan.hip: kBlock * RPL * UNROLL)
ROWS_PER_ITER = {"int8": 4096, "int16": 2048, "int32": 2048, "int64": 2048, "float32": 2048, "float64": 2048}
BITS_ROWS_PER_STEP = 8192  # dq_scan_bits_kernel, hll_bool: 32 rows per lane per step
CHUNK = 2048
BLOCK = 256

_TABLES = {}


class Tbl:
    def __init__(self, key, spec):
        from helpers import product_table
        self.key = key
        self.spec = spec
        self.ot = oracle_table(spec)
        self.host = product_table(spec)
        self._dev = None

    @property
    def dev(self):
        if self._dev is None:
            self._dev = self.host.to_device(0)
        return self._dev


def tables():
    """{"plain", "prefix"}: built once per process, never modified."""
    if not _TABLES:
        rng = np.random.default_rng(20261020)
        spec = random_table(rng, N_ROWS, 0.05)
        for t, v in PLANTED.items():
            for r in PLANT_ROWS:
                spec["c_" + t][1][r] = v
        mixed = ["12", "-7", "3.5", "1e3", "true", "false", "abc", "", " 4", "0x1F", None]
        spec["s_mixed"] = ["string", [mixed[int(i)] for i in rng.integers(0, len(mixed), N_ROWS)]]
        _TABLES["plain"] = Tbl("plain", spec)
        pre = {k: [t, list(v)] for k, (t, v) in spec.items()}
        for t in TYPES:
            pre["c_" + t][1][:NULL_PREFIX] = [None] * NULL_PREFIX
        _TABLES["prefix"] = Tbl("prefix", pre)
    return _TABLES


def schema():
    return tables()["plain"].host.schema


# ------------------------------------------------------------------------------ running a plan
def run_plan(analyzers, table, monkeypatch, env=None, consume=True):
    """(states by analyzer, [(kind, type, np, tasks, blocks per task, per_cu)], launches) of one
    fresh plan created with the knobs of `env` set (None = unset) through the test's monkeypatch."""
    sch = table.schema
    with monkeypatch.context() as m:
        for k, v in (env or {}).items():
            if v is None:
                m.delenv(k, raising=False)
            else:
                m.setenv(k, str(v))
        plan = Plan([op_spec_for(a, sch) for a in analyzers], sch)
    try:
        states = None
        if consume:
            for b in table.batches():
                plan.consume(b)
            states = dict(zip(analyzers, plan.finish()))
        groups, launches = L.diag_plan_groups(plan.handle)
        return states, groups, launches
    finally:
        plan.close()


def keys(groups):
    return {(g[0], g[1], g[2]) for g in groups}


# ------------------------------------------------------------------------ memoised oracle checks
_VERIFIED = {}
EXACT = (d.Size, d.Completeness, d.Compliance, d.Minimum, d.Maximum, d.ApproxCountDistinct, d.MinLength,
         d.MaxLength)


def is_exact(a, tbl):
    """Kinds whose state is bit-exact whatever the grid: counts, Min/Max, HLL, integral Sum/Mean."""
    if isinstance(a, EXACT):
        return True
    return isinstance(a, (d.Sum, d.Mean)) and tbl.spec[a.column][0].startswith("int")


def check(a, got, tbl):
    """test_gpu_parity._check_state, evaluated once per (analyzer, table, state value)."""
    from test_gpu_parity import _check_state
    seen = _VERIFIED.setdefault((tbl.key, a), [])
    if any(got == s for s in seen):
        return
    _check_state(a, got, tbl.ot)
    seen.append(got)


def check_all(states, tbl):
    for a, got in states.items():
        check(a, got, tbl)


# ------------------------------------------------------------------------------ analyzer pools
def stats(c, w=None):
    return [d.Sum(c, w), d.Mean(c, w), d.StandardDeviation(c, w), d.Minimum(c, w), d.Maximum(c, w)]


def hll(c, w=None):
    return [d.ApproxCountDistinct(c, w)]


MODES = ("stats", "hll", "both", "preds")


def mode_analyzers(mode, c, w=None):
    return {"stats": stats(c, w), "hll": hll(c, w), "both": stats(c, w) + hll(c, w), "preds": []}[mode]


_LITS = {}


def _literals(t):
    """Literals inside the column's value range, from the (plain) table itself."""
    if t not in _LITS:
        vals = sorted(v for v in tables()["plain"].spec["c_" + t][1] if v is not None)
        lo, hi, eq = vals[len(vals) * 2 // 5], vals[len(vals) * 3 // 5], vals[len(vals) // 2]
        if t.startswith("int"):
            # (a DOUBLE literal compares as fp64; a fractional DECIMAL one is rewritten to an int bound)
            _LITS[t] = (str(lo), str(hi), str(eq), "%d.5e0" % lo, "1e9" if t == "int64" else "1e2", "%d.5" % lo)
        else:
            third = repr(vals[len(vals) // 3])
            _LITS[t] = (repr(lo), str(int(round(hi))), repr(eq), third, third, third)
    return _LITS[t]


N_POOL = 16
NO_VALUES = (9, 10, 14, 15)  # IS [NOT] NULL, TRUE, FALSE: these alone do not make a task read values
CONSTANTS = (14, 15)         # column-free: they ride on the last task with their filter


def inline_pool(t):
    """One predicate of every form dq_api.cpp's fast_form evaluates inline on the column: the six
    operators with int and fractional literals, `lit CMP col`, COALESCE, IS [NOT] NULL, and the
    constants TRUE / FALSE (a boolean column as the predicate is the bits kernel's: bits_analyzers)."""
    c = "c_" + t
    a, b, e, fr, de, dec = _literals(t)
    return ["%s < %s" % (c, a), "%s <= %s" % (c, a), "%s > %s" % (c, b), "%s >= %s" % (c, b),
            "%s = %s" % (c, e), "%s != %s" % (c, e), "%s < %s" % (c, fr), "%s < %s" % (b, c),
            "COALESCE(%s, %s) >= %s" % (c, a, b), "%s IS NULL" % c, "%s IS NOT NULL" % c,
            "%s >= %s" % (dec, c), "%s != %s" % (c, de), "%s = %s" % (c, de), "TRUE", "FALSE"]


def fast_pk(t, idx):
    """The predicate kind of dq_scan_fast.hip (PK_*) that pool entry idx becomes, None = not one."""
    if idx == 8 or idx in NO_VALUES:
        return None
    eq = idx in (4, 5, 12, 13)
    as_f64 = t == "float64" or idx in (6, 12, 13)
    return (4 if eq else 3) if as_f64 else (2 if eq else 1)


def compliance(t, idx, w=None):
    p = inline_pool(t)[idx]
    return d.Compliance(p, p, w)


def pick(mode, k):
    """k pool indices, a window whose start moves with (mode, k) so every entry gets its turn."""
    start = (3 * MODES.index(mode) + 5 * k) % N_POOL
    while k and all((start + j) % N_POOL in NO_VALUES for j in range(k)):
        start += 2
    idxs = [(start + j) % N_POOL for j in range(k)]
    # (a constant placed before the column's task exists would open a task of its own)
    return [i for i in idxs if i not in CONSTANTS] + [i for i in idxs if i in CONSTANTS]


def expected_key(t, mode, idxs, ext=False, fast_on=True):
    """The (kind, type, np) dq_plan_create gives the task of column c_t with these inline
    predicates (dq_api.cpp: fast_variant and the grouping loop)."""
    if ext:
        return (1, CODE[t], -1)
    n = len(idxs)
    if fast_on and t in FAST_TYPES and n <= 1:
        pk = 0 if n == 0 else fast_pk(t, idxs[0])
        if pk is not None:
            return (2, CODE[t], pk | (8 if mode in ("stats", "both") else 0) | (16 if mode in ("hll", "both") else 0))
    return (1, CODE[t], n if n <= 4 else 8)


NP_CASES = (0, 1, 2, 3, 4, {"stats": 5, "hll": 6, "both": 7, "preds": 8})


def general_plans(t, mode):
    """(env, analyzers, expected key) for every NP of the general kernel under one mode; int64 /
    fp64 plans run with the fast scan on and off."""
    c = "c_" + t
    out = []
    for k in NP_CASES:
        k = k[mode] if isinstance(k, dict) else k
        if mode == "preds" and k == 0:
            continue  # (no such task: nothing asks for the column)
        idxs = pick(mode, k)
        an = mode_analyzers(mode, c) + [compliance(t, i) for i in idxs]
        for fast_on in ((True, False) if t in FAST_TYPES else (True,)):
            env = {"DQ_SCAN_FAST": None if fast_on else "0"}
            out.append((env, an, expected_key(t, mode, idxs, fast_on=fast_on)))
    return out


EXT_HOW = ("where", "mask", "both")


def ext_plans(t, mode):
    """The EXT kernel of one type: by a `where`, by mask predicates (generic programs, which attach
    to the column's task because it is the only one with their filter), and by both."""
    c = "c_" + t
    out = []
    for n_how, how in enumerate(EXT_HOW):
        w = None if how == "mask" else WHERE
        idxs = pick(mode, 1 + n_how) if (mode == "preds" or how != "where") else []
        an = mode_analyzers(mode, c, w) + [compliance(t, i, w) for i in idxs]
        if how != "where":
            an += [d.Compliance(m, m, w) for m in MASKS[n_how - 1:n_how + 1]]
        out.append(({}, an, (1, CODE[t], -1)))
    return out


FAST_FLAGS = ((True, False), (False, True), (True, True), (False, False))  # (statistics, HLL)


def fast_plans(t, with_stats, with_hll):
    """Every predicate kind of the fast scan under one (STATS, HLL) pair: each operator, so the
    host's rewrites (<= to <, the negations) run too."""
    c = "c_" + t
    mode = {(True, False): "stats", (False, True): "hll", (True, True): "both", (False, False): "preds"}[
        (with_stats, with_hll)]
    out = []
    for idx in [None] + [i for i in range(N_POOL) if fast_pk(t, i) is not None]:
        if idx is None and mode == "preds":
            continue  # dq_scan_fast_kernel<T, PK_NONE, false, false>: unreachable (UNREACHABLE)
        idxs = [] if idx is None else [idx]
        an = mode_analyzers(mode, c) + [compliance(t, i) for i in idxs]
        out.append(({}, an, expected_key(t, mode, idxs)))
    return out


def sibling_plans(t, n_preds, w):
    """n_preds (9..11) inline predicates on one column beside its statistics and HLL: the ninth
    and each further one open a sibling task without STATS / HLL.  (env, analyzers, expected keys)."""
    c = "c_" + t
    idxs = [8, 9, 10, 0, 1, 2, 3, 4, 5, 6, 7][:n_preds]  # (the ninth is `c != lit`: a fast-scan shape)
    an = stats(c, w) + hll(c, w) + [compliance(t, i, w) for i in idxs]
    if w is not None:
        return {}, an, {(1, CODE[t], -1)}
    # (dq_plan_create looks the full task up again for every further predicate, so each one gets a
    # sibling of its own)
    return {}, an, {(1, CODE[t], 8)} | {expected_key(t, "preds", [i]) for i in idxs[8:]}


def all_plan_specs():
    """Every (env, analyzers) the specialisation tests run, for the coverage test."""
    out = []
    for t in TYPES:
        for mode in MODES:
            out += [(e, a) for e, a, _ in general_plans(t, mode) + ext_plans(t, mode)]
    for t in FAST_TYPES:
        for s, h in FAST_FLAGS:
            out += [(e, a) for e, a, _ in fast_plans(t, s, h)]
        for n in (9, 10, 11):
            for w in (None, WHERE):
                e, a, _ = sibling_plans(t, n, w)
                out.append((e, a))
    for n in (9, 10, 11):
        for w in (None, WHERE):
            e, a, _ = sibling_plans("int32", n, w)
            out.append((e, a))
    out.append(({}, bits_analyzers()))
    return out


def bits_analyzers():
    """Tasks that read no values (dq_scan_bits_kernel): every predicate kind it evaluates."""
    return [d.Completeness("c_string"), d.Completeness("c_int16", WHERE), d.Size(WHERE),
            d.Compliance("n", "c_int8 IS NULL"), d.Compliance("nn", "c_float32 IS NOT NULL", WHERE),
            d.Compliance("b", "c_bool"), d.Compliance("t", "TRUE"), d.Compliance("f", "FALSE", WHERE),
            d.Compliance("m", MASKS[0]), d.Compliance("m2", MASKS[2], WHERE), d.Completeness("c_bool")]
