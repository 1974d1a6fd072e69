"""Generated SQL predicates through real GPU plans, against the oracle's row verdicts.

The host test (test_pred_generated.py) pins the interpreter's semantics; this one pins what only
the device build has: the ballot-word assembly of dq_pred_kernel (a wave writes one 64-row mask
word, a 256-thread block four), the ragged last word, realigned validity bitmaps, the string
literal pool in device memory, and the single-comparison forms the fused scan evaluates inline
(dq_api.cpp fast_form) next to the generic mask path.

Row counts 1, 63, 64, 65 and 2049 (one row in the final word after 8 full blocks), host and device
tables.  Each family's texts go in as ONE plan: dq_plan_create sets no cap of its own on predicate
programs (identical ones are shared; the mask kernel's grid y, 65535, is the only bound, and a
packed plan takes 2^16 ops), so a plan holds every program of a run.  Even texts are
`Compliance(name, p)`, odd ones the `where` of Size, Completeness("l"), Sum("l"), Minimum("d") and
of a Compliance of the next text.  Expected: Compliance and Size from the oracle's verdict lists
exactly; the rest what test_gpu_parity._check_state expects for the oracle's selected rows.

The oracle's verdicts of a (row count, text) are computed once and shared by every test here.
"""
import re

import pytest

import deequ_amd as d
import hostile as H
import pyoracle as O
from deequ_amd.engine import Plan, op_spec_for
from deequ_amd.predicates import UnsupportedPredicate, compile_predicate
from helpers import oracle_table
from predicate_cases import generate, is_inline, table
from test_gpu_parity import _check_state

pytestmark = pytest.mark.gpu

FAMILIES = ("numeric", "string")
NS = (1, 63, 64, 65, 2049)
PER_FAMILY = 300
NAMES = ["l", "d", "g", "i", "b", "s"]
SCHEMA = {"l": "int64", "d": "float64", "g": "float32", "i": "int32", "b": "bool", "s": "string"}
_TEXTS = {}
_SPECS = {}
_VERDICTS = {}


def _texts(family):
    """The first 300 texts of the family's seed that the compiler accepts, with their programs."""
    if family not in _TEXTS:
        index = {nm: (k, SCHEMA[nm]) for k, nm in enumerate(NAMES)}
        out = []
        for text in generate(31 if family == "numeric" else 32, 400, family):
            try:
                out.append((text, compile_predicate(text, index)))
            except UnsupportedPredicate:
                continue
        assert len(out) >= 300, len(out)
        _TEXTS[family] = out[:300]
    return _TEXTS[family]


def _spec(n):
    """({name: [dtype, values]}, oracle table) of table(n, 7000 + n); made once, never modified."""
    if n not in _SPECS:
        spec = {k: [t, v] for k, (t, v) in table(n, 7000 + n).items()}
        assert list(spec) == NAMES
        _SPECS[n] = (spec, oracle_table(spec))
    return _SPECS[n]


_EVAL = O.eval_predicate  # (the tests below answer the module's own calls from _VERDICTS)


def _verdicts(key, text, ot):
    if (key, text) not in _VERDICTS:
        _VERDICTS[key, text] = _EVAL(text, ot)
    return _VERDICTS[key, text]


def _analyzers(family, count):
    texts = [t for t, _ in _texts(family)[:count]]
    out = []
    for k, p in enumerate(texts):
        if k % 2 == 0:
            out.append(d.Compliance("c%d" % k, p))
        else:
            q = texts[(k + 1) % len(texts)]
            out += [d.Size(p), d.Completeness("l", p), d.Sum("l", p), d.Minimum("d", p), d.Compliance("w%d" % k, q, p)]
    return out


def _run(analyzers, batches):
    plan = Plan([op_spec_for(a, SCHEMA) for a in analyzers], SCHEMA)
    try:
        for b in batches:
            plan.consume(b)
        return plan.finish()
    finally:
        plan.close()


def _check(analyzers, states, key, ot, monkeypatch):
    """Compliance and Size from the verdict lists; everything through _check_state, whose oracle
    calls are answered from the shared verdicts."""
    def shared(text, tbl):
        assert tbl is ot
        return _verdicts(key, text, ot)

    monkeypatch.setattr(O, "eval_predicate", shared)
    n = len(ot["l"].values)
    for a, st in zip(analyzers, states):
        w = _verdicts(key, a.where, ot) if a.where else [True] * n
        if isinstance(a, d.Size):
            want = None if all(v is None for v in w) else d.NumMatches(sum(1 for v in w if v is True))
            assert st == want, (a, st, want)
        elif isinstance(a, d.Compliance):
            p = [v for v, keep in zip(_verdicts(key, a.predicate, ot), w) if keep is True and v is not None]
            want = (None if not p or all(v is None for v in w)
                    else d.NumMatchesAndCount(sum(1 for v in p if v), sum(1 for v in w if v is True)))
            assert st == want, (a, st, want)
        _check_state(a, st, ot)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("n", NS)
def test_generated_predicates_through_plans(gpu, monkeypatch, n, family, device):
    spec, ot = _spec(n)
    t = d.Table.from_pydict({k: (v[0], v[1]) for k, v in spec.items()})
    analyzers = _analyzers(family, PER_FAMILY)
    states = _run(analyzers, [t.to_device(0) if device else t])
    _check(analyzers, states, n, ot, monkeypatch)


@pytest.mark.parametrize("family", FAMILIES)
def test_both_device_paths_are_exercised(family):
    """The Compliance half holds predicates the fused scan evaluates inline and predicates that
    go through dq_pred_kernel, the inline ones over every numeric column."""
    dtypes = [SCHEMA[nm] for nm in NAMES]
    progs = [prog for k, (_, prog) in enumerate(_texts(family)) if k % 2 == 0]
    inline = [p for p in progs if is_inline(p, dtypes)]
    assert len(inline) >= 20 and len(progs) - len(inline) >= 20, (len(inline), len(progs))
    from deequ_amd import _lib as L
    cols = {ins[1] for p in inline for ins in p if ins[0] == L.DQ_P_COLUMN}
    assert {NAMES.index(c) for c in "ldgi"} <= cols, cols


_NULL_LEANING = re.compile(r"\bIS\s+(NOT\s+)?NULL\b|\bCOALESCE\b|<=>|\bNOT\b|\bOR\b|\bNULL\b")


@pytest.mark.parametrize("flavour,shift", [("digits", 0), ("high", 1)])
def test_generated_predicates_on_hostile_sliced_columns(gpu, monkeypatch, flavour, shift):
    """n = 2049 on device, every column sliced at one of the offsets 1, 7, 61, 2051 (validity
    realigned by the kernel) in hostile buffers: NULL slots and rows outside the window hold NaN,
    +-Inf, INT_MAX, set bits and non-empty strings.  The predicates are those that lean on
    IS NULL, COALESCE, <=>, NOT, OR and the NULL literal: a NULL slot's bytes reach no verdict."""
    spec, ot = _spec(2049)
    offs = (1, 7, 61, 2051)
    offsets = {nm: offs[(j + shift) % 4] for j, nm in enumerate(NAMES)}
    t = H.hostile_table(spec, offset=offsets, device=True, flavour=flavour)
    for nm in NAMES:
        assert t.columns[nm].offset == offsets[nm] and t.columns[nm].validity is not None
    for family in FAMILIES:
        analyzers = [a for a in _analyzers(family, PER_FAMILY)
                     if _NULL_LEANING.search((a.where or a.predicate).upper())]
        assert len(analyzers) >= 100, len(analyzers)
        _check(analyzers, _run(analyzers, [t]), 2049, ot, monkeypatch)


def test_two_batches_through_one_plan(gpu, monkeypatch):
    """65 and 2049 rows consumed by one plan (a host batch, then a device batch): the states are
    the oracle's over the concatenation, whose verdicts are those of the two tables in a row."""
    (s1, o1), (s2, o2) = _spec(65), _spec(2049)
    both = {k: [s1[k][0], s1[k][1] + s2[k][1]] for k in NAMES}
    ot = oracle_table(both)
    key = (65, 2049)
    t1 = d.Table.from_pydict({k: (v[0], v[1]) for k, v in s1.items()})
    t2 = d.Table.from_pydict({k: (v[0], v[1]) for k, v in s2.items()}).to_device(0)
    for family in FAMILIES:
        analyzers = _analyzers(family, PER_FAMILY)
        for a in analyzers:
            for text in filter(None, (a.where, getattr(a, "predicate", None))):
                _VERDICTS.setdefault((key, text), _verdicts(65, text, o1) + _verdicts(2049, text, o2))
        _check(analyzers, _run(analyzers, [t1, t2]), key, ot, monkeypatch)
