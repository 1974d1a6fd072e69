"""Generated regular expressions on the GPU: about 200 of test_regex_generated.py's cases (the 8
largest tables, every table within 512 bytes of the LDS budget, every ninth of the rest) through
both kernels that walk the compiler's tables.

dq_regex_kernel: 16 PatternMatch ops per plan on one string column -- DFA images of very different
sizes side by side at their dfa_off -- over the union of the 16 patterns' strings with ~5 % NULLs;
host- and device-resident tables, one sliced hostile column, and once every string behind a 16-,
17- and 19-byte prefix, so that the deciding bytes fall in the 16-byte, 4-byte and 1-byte loops.
dq_schema_eval_kernel: RowLevelSchemaValidator with `matches`, row by row against
schema_cases.mirror, a quarter of the patterns again with minLength / maxLength (the walk then goes
on past the accept state).  The expected values are pattern_cases.oracle's throughout, computed
once per session.  The size boundary: a table within 60 bytes of the budget runs on both kernels, the
same pattern one repetition longer is declined, not run.
"""
import functools
import random
import statistics
from collections import OrderedDict

import numpy as np
import pytest

import hostile as H
import pattern_cases as C
import regex_gen as G
import schema_cases as S
import test_regex_generated as T
from test_gpu_pattern_match import run_plan
from test_pattern_match import regex_match

pytestmark = pytest.mark.gpu

MAX_TABLE_BYTES = 48 * 1024   # regex::kMaxTableBytes
PER_PLAN = 16
PADS = (16, 17, 19)


@functools.lru_cache(maxsize=None)
def selected():
    """The GPU's share of the CPU test's accepted cases, largest tables first."""
    accepted = sorted((c for c in T.all_cases() if c.accepted), key=lambda c: (-c.table_bytes, c.seed, c.index))
    near = [c for c in accepted if c.table_bytes > MAX_TABLE_BYTES - 512]
    assert near, "no generated table within 512 bytes of the budget: add a hand-made one"
    picked = accepted[:8] + [c for c in accepted[8:] if c in near]
    rest = [c for c in accepted if c not in picked]
    picked += sorted(rest, key=lambda c: (c.seed, c.index))[::9]
    assert 180 <= len(picked) <= 230 and sum(c.table_bytes > 40 * 1024 for c in picked) >= 8
    assert sum(c.table_bytes < 1024 for c in picked) >= 20   # small images beside the large ones
    return tuple(picked)


def groups():
    """Plans of 16: each of the first eight holds one of the eight largest tables."""
    sel = list(selected())
    n_groups = (len(sel) + PER_PLAN - 1) // PER_PLAN
    return [sel[g::n_groups] for g in range(n_groups)]


@functools.lru_cache(maxsize=None)
def group_rows(g, pads=False):
    """(values with NULLs, [(matches, count) per pattern]) of group g: the union of its patterns'
    strings (behind each of the prefixes when `pads`), the oracle's answer on every row."""
    group = groups()[g]
    rng = random.Random(9000 + g)
    values = []
    for c in group:
        if pads:
            fill = G.complement_alphabet(c.pattern)
            for n in PADS:
                values += ["".join(rng.choice(fill) for _ in range(n)) + s for s in c.strings]
        else:
            values += c.strings
    rng.shuffle(values)
    values = [None if rng.random() < 0.05 else v for v in values]
    assert any(v is None for v in values)
    want = [(sum(C.oracle(c.text, v) for v in values if v is not None), len(values)) for c in group]
    return values, want


def check_plans(make_table, pads=False, only=None):
    import deequ_amd as d
    hit = total = 0
    for g, group in enumerate(groups()):
        if only is not None and g not in only:
            continue
        values, want = group_rows(g, pads)
        table = make_table(d, values)
        got = run_plan(d, [d.PatternMatch("s", c.text) for c in group], [table], table.schema)
        for c, state, (m, n) in zip(group, got, want):
            assert state == (14, 1, m, n), "pattern %r (table %d bytes): kernel %r, oracle (%d, %d)" % (
                c.text, c.table_bytes, state[2:], m, n)
            hit, total = hit + m, total + n
    return hit / total


def host_table(d, values):
    return d.Table.from_pydict({"s": ("string", values)})


def test_selection(gpu):
    sel = selected()
    sizes = [c.table_bytes for c in sel]
    print("%d patterns in %d plans; table bytes: smallest %d, median %d, largest %s" % (
        len(sel), len(groups()), min(sizes), sorted(sizes)[len(sizes) // 2], sorted(sizes)[-8:]))
    assert len(set(c.text for c in sel)) == len(sel)
    for c in sel:   # the per-pattern strings give both verdicts nearly everywhere
        assert len(c.want) == len(c.strings)
    assert sum(0.1 <= c.rate <= 0.9 for c in sel) >= 0.85 * len(sel)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_pattern_match_plans_of_sixteen(gpu, device):
    rate = check_plans(lambda d, v: host_table(d, v).to_device(0) if device else host_table(d, v))
    print("match rate over all (pattern, row) pairs: %.3f" % rate)
    assert 0.02 < rate < 0.9


def test_pattern_match_sliced_hostile_column(gpu):
    def make(d, values):
        col = H.hostile_column("string", values, offset=61, device=True, flavour="digits")
        return d.Table(OrderedDict([("s", col)]))
    check_plans(make, only=(0, 1))


def test_pattern_match_behind_prefixes(gpu):
    """Every string behind 16, 17 and 19 bytes the pattern's characters do not take (where it leaves
    any): the oracle is asked again, nothing is assumed unchanged."""
    rate = check_plans(lambda d, v: host_table(d, v).to_device(0), pads=True)
    print("match rate behind the prefixes: %.3f" % rate)
    assert 0.01 < rate < 0.9


def string_def(pattern, **bounds):
    return [dict({"kind": "string", "name": "s", "matches": pattern}, **bounds)]


def check_rows(cols, defs, device=True):
    """validate's two index vectors against the restatement's."""
    import deequ_amd as d
    m = S.mirror(cols, defs)
    table = d.Table.from_pydict(cols)
    res = d.RowLevelSchemaValidator.validate(table.to_device(0) if device else table, S.build_schema(defs),
                                             withRowIndices=True)
    got_valid, got_invalid = res.validRowIndices.tolist(), res.invalidRowIndices.tolist()
    if got_valid != m.valid_idx or got_invalid != m.invalid_idx:
        values = cols["s"][1]
        wrong = sorted(set(got_valid) ^ set(m.valid_idx) | set(got_invalid) ^ set(m.invalid_idx))
        raise AssertionError("schema %r: rows %r differ: %s" % (defs, wrong[:8], [
            (values[r], "kernel valid" if r in got_valid else "kernel invalid",
             "oracle valid" if r in m.valid_idx else "oracle invalid") for r in wrong[:8]]))
    assert (res.numValidRows, res.numInvalidRows) == (len(m.valid_idx), len(m.invalid_idx))
    return m


def case_column(c):
    rng = random.Random(c.seed * 1000 + c.index)
    return OrderedDict([("s", ("string", [None if rng.random() < 0.05 else s for s in c.strings] + [None]))])


@pytest.mark.parametrize("part", range(4))
def test_rows_through_the_schema_validator(gpu, part):
    """Row by row, what the aggregate count cannot show, through the second kernel's copy of the
    walker.  NULL rows are valid (isNullable defaults to true)."""
    both = 0
    mine = selected()[part::4]
    for c in mine:
        cols = case_column(c)
        m = check_rows(cols, string_def(c.text), device=(c.index % 2 == 0))
        nulls = [r for r, v in enumerate(cols["s"][1]) if v is None]
        assert set(nulls) <= set(m.valid_idx) and not m.null_idx
        assert len(m.valid_idx) - len(nulls) == sum(w for w, v in zip(c.want, cols["s"][1]) if v is not None)
        both += bool(len(m.valid_idx) > len(nulls) and m.invalid_idx)
    assert both >= 0.85 * len(mine)


def test_rows_with_length_bounds_walk_past_the_accept_state(gpu):
    """minLength / maxLength beside `matches`: the loop reads on after the DFA has accepted
    (count || (walk && s != accept)).  The bounds come from the strings' median character count, so
    that a matching row fails for its length and a row of the right length for the pattern."""
    verdicts = set()
    for k, c in enumerate(selected()[::4]):
        cols = case_column(c)
        med = int(statistics.median(len(s) for s in c.strings))
        bounds = ({"minLength": med}, {"maxLength": med}, {"minLength": max(1, med - 3), "maxLength": med + 3})[k % 3]
        defs = string_def(c.text, **bounds)
        m = check_rows(cols, defs, device=(k % 2 == 0))
        only_pattern = S.mirror(cols, string_def(c.text))
        only_length = S.mirror(cols, [dict({"kind": "string", "name": "s"}, **bounds)])
        verdicts.add("length fails a matching row" if set(only_pattern.valid_idx) - set(m.valid_idx) else "")
        verdicts.add("pattern fails a row of the right length" if set(only_length.valid_idx) - set(m.valid_idx) else "")
        verdicts.add("valid" if len(m.valid_idx) > 3 else "")
    assert verdicts >= {"length fails a matching row", "pattern fails a row of the right length", "valid"}


# ---------------------------------------------------------------- the size boundary
HEAD = "kqzjxvwbpfmg@#%&=<>;:!~_/,"


def boundary_pattern(j):
    """26 distinct literals, j digits and a 'Z': a search DFA of about j + 30 states by about 30
    columns, which a longer counted repetition grows 2 * n_cols bytes at a time."""
    return HEAD + "\\d{%d}Z" % j


@functools.lru_cache(maxsize=None)
def boundary():
    """(j, table bytes): the longest repetition that fits, found on the host."""
    lo, hi = 1, 1000   # regex::kMaxRepeat
    assert regex_match(boundary_pattern(lo), "")[0] == 0 and regex_match(boundary_pattern(hi), "")[0] != 0
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if regex_match(boundary_pattern(mid), "")[0] == 0:
            lo = mid
        else:
            hi = mid
    _, _, n_states, n_cols, _ = regex_match(boundary_pattern(lo), "")
    return lo, 2 * n_states * n_cols


def boundary_strings(j):
    rng = random.Random(j)
    digits = lambda n: "".join(rng.choice("0123456789") for _ in range(n))  # noqa: E731
    out = []
    for n in (j, j - 1, j, j + 1, j, 1, j, j):
        out += [HEAD + digits(n) + "Z", "xx" + HEAD + digits(n) + "Zyy", HEAD + digits(n), HEAD[1:] + digits(n) + "Z",
                HEAD[:9] + HEAD + digits(n) + "Z", HEAD + digits(n) + "z", HEAD + digits(n // 2) + "é" + digits(n - n // 2) + "Z"]
    return out + ["", None, "Z", HEAD, None]


def test_size_boundary(gpu):
    import deequ_amd as d
    from deequ_amd import _lib as L
    j, size = boundary()
    print("\\d{%d}: table of %d bytes, %d under the budget" % (j, size, MAX_TABLE_BYTES - size))
    assert MAX_TABLE_BYTES - 512 < size <= MAX_TABLE_BYTES
    fits, too_large = boundary_pattern(j), boundary_pattern(j + 1)
    st, _, _, _, msg = regex_match(too_large, "")
    assert st == L.DQ_ERR_UNSUPPORTED and "LDS budget" in msg, msg
    values = boundary_strings(j)
    want = [C.oracle(fits, v) for v in values if v is not None]
    assert 0.2 < sum(want) / len(want) < 0.8
    for device in (False, True):
        table = host_table(d, values)
        table = table.to_device(0) if device else table
        got = run_plan(d, [d.PatternMatch("s", fits), d.PatternMatch("s", "a")], [table], table.schema)
        assert got[0] == (14, 1, sum(want), len(values)), (got[0], sum(want))
        assert got[1] == (14, 1, sum(C.oracle("a", v) for v in values if v is not None), len(values))
    cols = OrderedDict([("s", ("string", values))])
    check_rows(cols, string_def(fits))
    check_rows(cols, string_def(fits, minLength=len(HEAD) + j + 1, maxLength=len(HEAD) + j + 3))
    # one state too many: declined where the plan is made, nothing runs
    with pytest.raises(L.UnsupportedOnGpu) as e:
        run_plan(d, [d.PatternMatch("s", too_large)], [host_table(d, values)], {"s": "string"})
    assert "LDS budget" in str(e.value)
    with pytest.raises(L.UnsupportedOnGpu) as e:
        d.RowLevelSchemaValidator.validate(host_table(d, values), S.build_schema(string_def(too_large)))
    assert "LDS budget" in str(e.value)


def test_many_workgroups_stage_the_largest_tables(gpu):
    """20 001 rows: several workgroups of each task stage the same 40-48 KiB table."""
    import deequ_amd as d
    largest = list(selected()[:8])
    assert all(c.table_bytes > 40 * 1024 for c in largest)
    base = [s for c in largest for s in c.strings] + [None] * 17
    n = 20001
    values = [base[r % len(base)] for r in range(n)]
    answers = {c.text: np.array([0 if v is None else C.oracle(c.text, v) for v in base]) for c in largest}
    times = np.bincount(np.arange(n) % len(base), minlength=len(base))
    table = host_table(d, values).to_device(0)
    got = run_plan(d, [d.PatternMatch("s", c.text) for c in largest], [table], table.schema)
    for c, state in zip(largest, got):
        assert state == (14, 1, int((answers[c.text] * times).sum()), n), c.text
    near = largest[0]
    assert near.table_bytes > MAX_TABLE_BYTES - 512
    res = d.RowLevelSchemaValidator.validate(table, S.build_schema(string_def(near.text)), withRowIndices=True)
    want_valid = [r for r in range(n) if values[r] is None or answers[near.text][r % len(base)]]
    assert res.validRowIndices.tolist() == want_valid
    assert res.numInvalidRows == n - len(want_valid) and 0 < len(want_valid) < n
    valid_set = set(want_valid)
    assert res.invalidRowIndices.tolist() == [r for r in range(n) if r not in valid_set]
