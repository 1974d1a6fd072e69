"""LIKE / RLIKE predicates on the GPU (dq_match_mask_kernel + the predicate interpreter reading its
masks), through real plans on host- and device-resident tables, against like_cases.py's references:
the hand-written wildcard matcher for LIKE, re.search for RLIKE, Kleene logic over them and the
oracle for combined predicates.  Row counts around the wave, string lengths around the 16- / 4- /
1-byte load tiers, the heap's last byte, multi-byte code points across a 16-byte boundary, NULLs,
sliced hostile columns, task sharing inside one plan, `where` filters, batches and merges, DFA
images next to the 48 KiB bound, the generated set, the runner and the profiler."""
import ctypes
import functools
from collections import OrderedDict

import numpy as np
import pytest

import hostile as H
import like_cases as K
import pattern_cases as C

from oracle import pyoracle as O

pytestmark = pytest.mark.gpu


def q(pattern):
    return K.sql_quote(pattern)


def counts(kind, pattern, values):
    """(TRUE rows, all rows, NULL rows) of the reference."""
    v = [K.verdict(kind, pattern, s) for s in values]
    return v.count(True), len(v), v.count(None)


def run_plan(d, analyzers, batches, schema):
    """([(num_matches, count, has_value) per analyzer], (match tasks, DFA images)) of one plan."""
    from deequ_amd import _lib as L
    from deequ_amd.engine import Plan, op_spec_for
    plan = Plan([op_spec_for(a, schema) for a in analyzers], schema)
    try:
        for b in batches:
            plan.consume(b)
        states = [(s.num_matches, s.count, s.has_value) for s in plan.finish_raw()][:len(analyzers)]
        return states, L.diag_plan_match_tasks(plan.handle)
    finally:
        plan.close()


def both_residences(d, data):
    t = d.Table.from_pydict(data)
    return [("host", t), ("device", t.to_device(0))]


def check_compliance(d, table, kind, pattern, values, label=""):
    """Compliance of the predicate and of its negation: NULL rows are in `count` and in neither."""
    op = "LIKE" if kind == "like" else "RLIKE"
    a = d.Compliance("p", "s %s %s" % (op, q(pattern)))
    b = d.Compliance("n", "s NOT %s %s" % (op, q(pattern)))
    t, n, nulls = counts(kind, pattern, values)
    got = d.run_scan([a, b], table)
    if nulls == n:   # no row decides: the oracle's (Spark's) state of a column of NULL verdicts
        ot = {"v": O.OColumn("bool", [None] * n)}
        assert O.compliance_state(ot, "v") is None and got[a] is None and got[b] is None, (label, got)
        return
    assert got[a] == d.NumMatchesAndCount(t, n), (label, kind, pattern, got[a], t, n)
    assert got[b] == d.NumMatchesAndCount(n - t - nulls, n), (label, kind, pattern, got[b])


# ---------------------------------------------------------------------------- rows, lengths, heap end
@pytest.mark.parametrize("n", [1, 63, 64, 65, 2049])
def test_row_counts(gpu, n):
    import deequ_amd as d
    rng = np.random.default_rng(n)
    strings = K.like_inputs("%keyword%", max(n, 2), rng)[:n]
    values = [None if (n > 1 and rng.random() < 0.1) else s for s in strings]
    values[-1] = "a keyword"   # the last row of the ragged word decides
    for label, table in both_residences(d, {"s": ("string", values)}):
        check_compliance(d, table, "like", "%keyword%", values, label)
        check_compliance(d, table, "like", "%keyword", values, label)
        check_compliance(d, table, "rlike", "keyword$", values, label)
        check_compliance(d, table, "rlike", "^[^k]*$", values, label)


LENGTHS = [0, 1, 3, 4, 5, 15, 16, 17, 31, 32, 33, 100]


def length_rows():
    """Per byte length: filler only, the deciding character first, last, and (full mode) a text
    that matches but for one extra trailing byte."""
    rows = []
    for n in LENGTHS:
        rows += ["x" * n, ("K" + "x" * (n - 1))[:n], ("x" * (n - 1) + "K")[-n:] if n else "", "x" * n + "K", "K" + "x" * n,
                 "K" + "x" * n + "y", "x" * n + "Ky"]
    return rows


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_string_lengths_around_the_load_tiers(gpu, device):
    import deequ_amd as d
    values = length_rows()
    table = d.Table.from_pydict({"s": ("string", values)})
    table = table.to_device(0) if device else table
    for n in LENGTHS:   # full mode: exactly n + 1 bytes with K first / last; one more byte fails it
        check_compliance(d, table, "like", "K" + "_" * n, values)
        check_compliance(d, table, "like", "_" * n + "K", values)
    for kind, pattern in (("like", "K%"), ("like", "%K"), ("like", "%K%"), ("like", "%x"), ("rlike", "K"), ("rlike", "^K"),
                          ("rlike", "K$"), ("rlike", "^x*K$"), ("rlike", "^x{16}K?$"), ("rlike", "^x{31,33}$")):
        check_compliance(d, table, kind, pattern, values)
    # the reference itself tells the text that is one byte too long from the one that matches
    assert "x" * 16 + "K" in values and "x" * 16 + "Ky" in values
    assert K.like_match("_" * 16 + "K", "x" * 16 + "K") and not K.like_match("_" * 16 + "K", "x" * 16 + "Ky")


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_last_row_ends_at_the_end_of_the_heap(gpu, device):
    """The buffer resource's bound is the heap's last byte, and the pattern needs that byte."""
    import deequ_amd as d
    for tail in (1, 4, 16, 17, 35):
        values = ["q" * 7, None, "", "z" * (tail - 1) + "K"]
        padded = d.Column.from_pylist(values, "string")
        end = int(padded.offsets[-1])
        col = d.Column("string", len(values), np.array(padded.values[:end]), padded.validity, padded.offsets)
        assert len(col.values) == end == 7 + tail, "the heap must end with the last row"
        table = d.Table(OrderedDict([("s", col)]))
        table = table.to_device(0) if device else table
        check_compliance(d, table, "like", "%K", values)
        check_compliance(d, table, "like", "z" * (tail - 1) + "_", values)
        check_compliance(d, table, "rlike", "K$", values)
        check_compliance(d, table, "like", "%K_", values)   # would need a byte past the heap: FALSE


def test_code_points_across_a_load_boundary(gpu):
    """2-, 3- and 4-byte code points under `_` and `.`, their bytes on both sides of byte 16."""
    import deequ_amd as d
    values = []
    for ch in ("é", "例", "😀"):
        width = len(ch.encode("utf-8"))
        for lead in range(16 - width, 17):   # the code point starts at byte `lead`
            values += ["a" * lead + ch + "b", "a" * lead + ch, "a" * lead + ch + ch + "b"]
    values += [None, "a" * 15 + "\n" + "b", "a" * 16 + "\r\n"]
    for label, table in both_residences(d, {"s": ("string", values)}):
        for lead in (12, 13, 14, 15, 16):
            check_compliance(d, table, "like", "a" * lead + "_b", values, label)
            check_compliance(d, table, "like", "a" * lead + "_", values, label)
            check_compliance(d, table, "like", "%a__b", values, label)
            check_compliance(d, table, "rlike", "^a{%d}.b$" % lead, values, label)
            check_compliance(d, table, "rlike", "a..b", values, label)


# ---------------------------------------------------------------------------- NULLs and slices
def test_nulls(gpu):
    import deequ_amd as d
    rng = np.random.default_rng(3)
    base = K.like_inputs("a%b_c", 700, rng)
    scattered = [None if rng.random() < 0.3 else s for s in base]
    runs = list(base)
    runs[64:256] = [None] * 192       # three whole waves of NULLs
    runs[300:333] = [None] * 33
    for values in (scattered, [None] * 130, runs):
        for label, table in both_residences(d, {"s": ("string", values)}):
            check_compliance(d, table, "like", "a%b_c", values, label)
            check_compliance(d, table, "rlike", "a.*b.c$", values, label)
            # as a filter: NULL rows are out of scope
            size = d.Size("s LIKE 'a%b_c'")
            other = d.Size("s NOT LIKE 'a%b_c'")
            got = d.run_scan([size, other], table)
            t, n, nulls = counts("like", "a%b_c", values)
            if nulls == n:   # (the oracle: a filter that is NULL on every row)
                assert O.size_state({"v": O.OColumn("bool", [None] * n)}, "v") is None
                assert got[size] is None and got[other] is None, (label, got)
            else:
                assert got[size] == d.NumMatches(t) and got[other] == d.NumMatches(n - t - nulls), (label, got)


@pytest.mark.parametrize("offset", [1, 7, 61])
def test_sliced_hostile_column(gpu, offset):
    """An Arrow offset that is no multiple of 8 (the bitmap is realigned), a first string offset
    that is not zero, and heap bytes around the window that would complete a match."""
    import deequ_amd as d
    rng = np.random.default_rng(offset)
    strings = K.like_inputs("%1true%", 333, rng)
    values = [None if rng.random() < 0.1 else s for s in strings]
    for device in (False, True):
        col = H.hostile_column("string", values, offset=offset, device=device, flavour="text")
        table = d.Table(OrderedDict([("s", col)]))
        check_compliance(d, table, "like", "%1true%", values)
        check_compliance(d, table, "like", "%e", values)
        check_compliance(d, table, "rlike", "true0k$", values)
        check_compliance(d, table, "rlike", "^1", values)


# ---------------------------------------------------------------------------- one plan, shared tasks
def test_one_plan_shares_tasks(gpu):
    import deequ_amd as d
    rng = np.random.default_rng(17)
    n = 3000
    strings = K.like_inputs("a%keyword%b", n, rng)
    s = [None if rng.random() < 0.07 else v for v in strings]
    s[3], s[700], s[2999] = "x%keyword%y", "%keyword%", "a%keyword%b"   # what the same text finds as a regex
    t = [None if rng.random() < 0.07 else v for v in K.like_inputs("%b", n, rng)]
    num = [None if rng.random() < 0.1 else int(v) for v in rng.integers(0, 10, n)]
    data = {"s": ("string", s), "t": ("string", t), "n": ("int64", num)}
    ot = {k: O.OColumn(ty, list(v)) for k, (ty, v) in data.items()}
    an = [
        d.Compliance("k1", "s LIKE '%keyword%'"),                        # task 1
        d.Compliance("k2", "s LIKE '%keyword%' AND n > 3"),              # ... again
        d.Completeness("n", "s LIKE '%keyword%'"),                       # ... and as a filter
        d.Compliance("two", "s LIKE 'a%' OR s LIKE '%b'"),               # tasks 2 and 3, one program
        d.Compliance("r", "s RLIKE '%keyword%'"),                        # task 4: same text, other mode
        d.Compliance("other column", "t LIKE '%keyword%'"),              # task 5: same image, other column
        d.Compliance("num", "n > 3 AND n < 8"),
        d.Compliance("inline", "n >= 5"),                                # fast_form
        d.PatternMatch("s", "keyword"),
        d.Size(),
    ]
    kw = [K.verdict("like", "%keyword%", v) for v in s]
    n_gt3 = O.eval_predicate("n > 3", ot)
    want = [
        (kw.count(True), n),
        ([K.k_and(a, b) for a, b in zip(kw, n_gt3)].count(True), n),
        (sum(1 for a, v in zip(kw, num) if a is True and v is not None), kw.count(True)),
        ([K.k_or(K.verdict("like", "a%", v), K.verdict("like", "%b", v)) for v in s].count(True), n),
        ([K.verdict("rlike", "%keyword%", v) for v in s].count(True), n),
        ([K.verdict("like", "%keyword%", v) for v in t].count(True), n),
        (O.eval_predicate("n > 3 AND n < 8", ot).count(True), n),
        (O.eval_predicate("n >= 5", ot).count(True), n),
        (sum(C.oracle("keyword", v) for v in s if v is not None), n),
    ]
    assert want[0][0] > 100 and want[4][0] > 0 and want[4][0] != want[0][0]
    for label, table in both_residences(d, data):
        states, (tasks, images) = run_plan(d, an, [table], table.schema)
        assert [(m, c) for m, c, _ in states[:9]] == want, (label, states, want)
        assert (tasks, images) == (5, 4), (tasks, images)
        alone, (tasks, images) = run_plan(d, [an[8], an[7], an[9]], [table], table.schema)
        assert (tasks, images) == (0, 0) and alone[0] == states[8] and alone[1] == states[7]


# ---------------------------------------------------------------------------- as `where`
def test_as_where_of_other_analyzers(gpu):
    """The reference's verdicts as a boolean column of the oracle's table, which it filters by."""
    import deequ_amd as d
    from test_gpu_parity import _check_state
    rng = np.random.default_rng(29)
    n = 2500
    s = [None if rng.random() < 0.1 else v for v in K.like_inputs("%ab_c%", n, rng)]
    num = [None if rng.random() < 0.1 else int(v) for v in rng.integers(-50, 50, n)]
    x = [None if rng.random() < 0.1 else float(v) for v in rng.normal(0, 10, n)]
    data = {"s": ("string", s), "i": ("int64", num), "x": ("float64", x)}
    filters = [("s LIKE '%ab_c%'", lambda v: K.verdict("like", "%ab_c%", v)),
               ("s NOT RLIKE 'ab.c'", lambda v: K.k_not(K.verdict("rlike", "ab.c", v))),
               ("s LIKE 'zzzz%'", lambda v: K.verdict("like", "zzzz%", v))]     # selects nothing
    for label, table in both_residences(d, data):
        for where, fn in filters:
            keep = [fn(v) is True for v in s]
            ot = {k: O.OColumn(ty, list(vals)) for k, (ty, vals) in data.items()}
            ot["keep"] = O.OColumn("bool", [fn(v) for v in s])
            pairs = [(d.Size(where), d.Size("keep")), (d.Completeness("i", where), d.Completeness("i", "keep")),
                     (d.Sum("i", where), d.Sum("i", "keep")), (d.Minimum("x", where), d.Minimum("x", "keep")),
                     (d.MinLength("s", where), d.MinLength("s", "keep"))]
            pm = d.PatternMatch("s", "b.c", where)
            got = d.run_scan([a for a, _ in pairs] + [pm], table)
            for a, plain in pairs:
                _check_state(plain, got[a], ot)
            sel = [v for v, kp in zip(s, keep) if kp]
            if sel:
                assert got[pm] == d.NumMatchesAndCount(sum(C.oracle("b.c", v) for v in sel), len(sel)), (label, where)
            else:
                assert got[pm] is None


# ---------------------------------------------------------------------------- batches and merges
def test_two_batches_and_a_merge_of_states(gpu):
    import deequ_amd as d
    rng = np.random.default_rng(41)
    s = [None if rng.random() < 0.1 else v for v in K.like_inputs("CATEGORY%", 1500, rng)]
    cut = 777
    whole = d.Table.from_pydict({"s": ("string", s)})
    parts = [d.Table.from_pydict({"s": ("string", s[:cut])}), d.Table.from_pydict({"s": ("string", s[cut:])})]
    a = d.Compliance("c", "s LIKE 'CATEGORY%'")
    b = d.Compliance("r", "s RLIKE '^CATEGORY' OR s IS NULL")
    t, n, nulls = counts("like", "CATEGORY%", s)
    one = d.run_scan([a, b], whole)
    assert one[a] == d.NumMatchesAndCount(t, n) and one[b] == d.NumMatchesAndCount(t + nulls, n)
    for tables in (parts, [p.to_device(0) for p in parts]):
        batched = d.run_scan([a, b], d.PartitionedTable(tables))
        assert batched[a] == one[a] and batched[b] == one[b]
        first, second = d.run_scan([a, b], tables[0]), d.run_scan([a, b], tables[1])
        assert first[a].sum(second[a]) == one[a] and first[b].sum(second[b]) == one[b]


def test_reference_fixture(gpu):
    """IncrementalAnalysisTest.scala:69-71 over :108-160: the metrics are the hand matcher's counts,
    and the merged initial + delta states equal the states over everything (the reference's own
    assertion, :77-83)."""
    import deequ_amd as d
    fx = K.known_answers()

    def make(rows):
        return d.Table.from_pydict({nm: (t, list(c)) for nm, t, c in zip(fx["columns"], fx["types"], zip(*rows))})
    tables = {"initial": make(fx["initial"]), "delta": make(fx["delta"]), "everything": make(fx["initial"] + fx["delta"])}
    rows = {"initial": fx["initial"], "delta": fx["delta"], "everything": fx["initial"] + fx["delta"]}
    an = [d.Compliance(a["instance"], a["predicate"]) for a in fx["analyzers"]]
    states = {}
    for label, table in tables.items():
        ctx = d.AnalysisRunner.onData(table.to_device(0)).addAnalyzers(an).run()
        states[label] = d.run_scan(an, table)
        attr = [r[2] for r in rows[label]]
        want = [1.0, sum(K.like_match("CATEGORY%", v) for v in attr) / len(attr),
                sum(K.like_match("%keyword%", v) for v in attr) / len(attr)]
        assert [ctx.metric(a).value.get() for a in an] == want, label
    assert [states["everything"][a].numMatches for a in an] == [40, 12, 20]
    for a in an:
        merged = states["initial"][a].sum(states["delta"][a])
        assert merged == states["everything"][a]
        assert a.computeMetricFrom(merged).value.get() == a.computeMetricFrom(states["everything"][a]).value.get()


# ---------------------------------------------------------------------------- next to the 48 KiB bound
HEAD = "kqzjxvwbpfmg@#%&=<>;:!~_/,"
TAIL = "bcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789"


@functools.lru_cache(maxsize=None)
def largest(kind):
    """(pattern, image bytes): the largest image of a short list that still compiles."""
    from deequ_amd import _lib as L
    if kind == "rlike":
        cands = [HEAD + "\\d{%d}Z" % j for j in (700, 740, 760, 770, 780, 790, 800, 820)]
    else:
        cands = ["%a______" + TAIL[:k] for k in (20, 30, 36, 40, 42, 45, 50)]
    best = None
    for p in cands:
        try:
            size = len(L.diag_regex_match(p.encode(), b"", "find" if kind == "rlike" else "full", want_image=True)[3])
        except L.UnsupportedOnGpu:
            continue
        if best is None or size > best[1]:
            best = (p, size)
    return best


@pytest.mark.parametrize("kind", ["like", "rlike"])
def test_large_table_with_an_image_near_the_bound(gpu, kind):
    import deequ_amd as d
    pattern, size = largest(kind)
    print("%s %r: image of %d bytes" % (kind, pattern[:40], size))
    assert 32 * 1024 < size <= 48 * 1024 + 256 + 16 + 16
    rng = np.random.default_rng(5)
    if kind == "rlike":
        j = int(pattern[len(HEAD) + 3:-2])
        digits = lambda k: "".join(rng.choice(list("0123456789"), k))  # noqa: E731
        base = [HEAD + digits(j) + "Z", "xx" + HEAD + digits(j) + "Zyy", HEAD + digits(j - 1) + "Z", HEAD + digits(j) + "z",
                HEAD[1:] + digits(j) + "Z", "", None, HEAD + digits(j + 1) + "Z"]
    else:
        tail = pattern[len("%a______"):]
        fill = lambda k: "".join(rng.choice(list("a0é例"), k))  # noqa: E731
        base = ["a" + fill(6) + tail, fill(9) + "a" + fill(6) + tail, "a" + fill(5) + tail, "a" + fill(6) + tail + "x",
                "aa" + fill(5) + tail, "", None, "a" + fill(7) + tail, tail]
    n = 100003
    values = [base[r % len(base)] for r in range(n)]
    answers = [K.verdict(kind, pattern, v) for v in base]
    assert True in answers and False in answers
    times = np.bincount(np.arange(n) % len(base), minlength=len(base))
    want = int(sum(t for a, t in zip(answers, times) if a is True))
    op = "LIKE" if kind == "like" else "RLIKE"
    a = d.Compliance("big", "s %s %s" % (op, q(pattern)))
    small = d.Compliance("small", "s %s 'a%%'" % op)
    table = d.Table.from_pydict({"s": ("string", values)}).to_device(0)
    got = d.run_scan([a, small], table)
    assert got[a] == d.NumMatchesAndCount(want, n), (got[a], want)
    assert got[small] == d.NumMatchesAndCount(counts(kind, "a%", base * 1)[0] and sum(
        t for v, t in zip(base, times) if K.verdict(kind, "a%", v) is True), n)


def test_over_the_bound_is_declined_by_every_door(gpu):
    import deequ_amd as d
    from deequ_amd import _lib as L
    from deequ_amd.engine import Plan, op_spec_for
    from deequ_amd.predicates import UnsupportedPredicate
    pattern = "%a" + "_" * 14
    schema = {"s": "string"}
    with pytest.raises(UnsupportedPredicate, match="more than 2048 states"):
        op_spec_for(d.Compliance("c", "s LIKE '%s'" % pattern), schema)
    # past the front end: the library's own answer, by dq_op_supported and by plan creation
    b = pattern.encode()
    code = (L.DqPredInsn * 3)()
    for k, (op, arg) in enumerate(((L.DQ_P_COLUMN, 0), (L.DQ_P_LIT_STRING, len(b)), (L.DQ_P_LIKE, 0))):
        code[k].opcode, code[k].arg, code[k].i64, code[k].f64 = op, arg, 0, 0.0
    pool = ctypes.create_string_buffer(b, len(b))
    op = L.DqOp()
    op.kind = L.DQ_OP_COMPLIANCE
    op.predicate.code = ctypes.cast(code, ctypes.POINTER(L.DqPredInsn))
    op.predicate.n_insns = 3
    op.predicate.strings = ctypes.cast(pool, ctypes.c_void_p)
    op.predicate.strings_len = len(b)
    types = (ctypes.c_int32 * 1)(L.DQ_T_UTF8)
    assert L.lib().dq_op_supported(ctypes.byref(op), types, 1) == L.DQ_ERR_UNSUPPORTED
    assert "more than 2048 states" in L.lib().dq_last_error().decode()
    h = ctypes.c_void_p()
    st = L.lib().dq_plan_create(L.Context.get(d.current_device()).handle, ctypes.byref(op), 1, types, 1, ctypes.byref(h))
    assert st == L.DQ_ERR_UNSUPPORTED and not h.value
    op.predicate.strings_len = 3   # '%a_' fits: the same program is accepted
    code[1].arg = 3
    assert L.lib().dq_op_supported(ctypes.byref(op), types, 1) == L.DQ_OK


def test_packed_plan_answers_as_the_struct_plan(gpu):
    import deequ_amd as d
    from deequ_amd import _lib as L
    from deequ_amd.engine import OpSpec, Plan, op_spec_for, pack_ops
    from deequ_amd.predicates import CompiledPredicate
    from deequ_amd.table import dq_columns
    rng = np.random.default_rng(71)
    values = [None if rng.random() < 0.1 else v for v in K.like_inputs("%ab%", 900, rng)]
    table = d.Table.from_pydict({"s": ("string", values)})
    an = [d.Compliance("l", "s LIKE '%ab%'"), d.Completeness("s", "s RLIKE '^.?a'"), d.Compliance("n", "s NOT LIKE '_%b'")]
    specs = [op_spec_for(a, table.schema) for a in an]
    ref = Plan(specs, table.schema)
    ref.consume(table)
    want = bytes(ref.finish_raw())
    ref.close()
    blob = pack_ops(specs)
    types = (ctypes.c_int32 * 1)(L.DQ_T_UTF8)
    ctx = L.Context.get(d.current_device()).handle
    h = ctypes.c_void_p()
    L.check(L.lib().dq_plan_create_packed(ctx, blob, len(blob), types, 1, ctypes.byref(h)))
    try:
        assert L.diag_plan_match_tasks(h) == (3, 3)
        L.check(L.lib().dq_plan_consume(h, dq_columns(table, ["s"]), 1, table.num_rows))
        out = (L.DqState * 3)()
        L.check(L.lib().dq_plan_finish(h, out, 3))
        assert bytes(out) == want
        assert (out[0].num_matches, out[0].count) == counts("like", "%ab%", values)[:2]
    finally:
        L.lib().dq_plan_destroy(h)
    pattern = ("%a" + "_" * 14).encode()
    code = [(L.DQ_P_COLUMN, 0, 0, 0.0), (L.DQ_P_LIT_STRING, len(pattern), 0, 0.0), (L.DQ_P_LIKE, 0, 0, 0.0)]
    bad = pack_ops([OpSpec(L.DQ_OP_COMPLIANCE, -1, CompiledPredicate(code, pattern), None)])
    st = L.lib().dq_plan_create_packed(ctx, bad, len(bad), types, 1, ctypes.byref(h))
    assert st == L.DQ_ERR_UNSUPPORTED and "more than 2048 states" in L.lib().dq_last_error().decode()


# ---------------------------------------------------------------------------- the generated set
@pytest.mark.parametrize("family", ["like", "combined"])
def test_generated_set_as_one_plan(gpu, family):
    """test_like.py's generated patterns (two of its seeds), all in ONE plan over 2049 rows."""
    import deequ_amd as d
    cases = K.generated_like(11, 40, 52) + K.generated_like(12, 40, 52)
    strings = [s for _, ss in cases for s in ss][:2049]
    assert len(strings) == 2049
    data = K.combined_table(strings, 7)
    s = data["s"][1]
    ot = {k: O.OColumn(ty, list(v)) for k, (ty, v) in data.items()}
    rng = np.random.default_rng(99)
    an, want = [], []
    for k, (pattern, _) in enumerate(cases):
        text = "s LIKE " + q(pattern)
        verdicts = [K.verdict("like", pattern, v) for v in s]
        if family == "like":
            sql, truth = text, verdicts
        else:
            other = K.OTHERS[int(rng.integers(len(K.OTHERS)))]
            sql, fn = K.combine(k % 4, text, other)
            truth = [fn(a, b) for a, b in zip(verdicts, O.eval_predicate(other, ot))]
        an.append(d.Compliance("g%d" % k, sql))
        want.append((truth.count(True), len(s)))
    for label, table in both_residences(d, data):
        states, (tasks, images) = run_plan(d, an, [table], table.schema)
        assert tasks == len({p for p, _ in cases}) == images
        bad = [(a.predicate, g[:2], w) for a, g, w in zip(an, states, want) if g[:2] != w]
        assert not bad, (label, bad[:5])
    assert sum(1 for m, _ in want if 0 < m < len(s)) >= 0.7 * len(want)


# ---------------------------------------------------------------------------- runner and profiler
def test_runner_with_frequency_analyzers_and_profiler_unaffected(gpu):
    import deequ_amd as d
    from deequ_amd.profiles import ColumnProfilerRunner
    rng = np.random.default_rng(61)
    n = 4000
    s = [None if rng.random() < 0.05 else v for v in K.like_inputs("%keyword%", n, rng)]
    cat = [("a", "b", "c")[int(v)] for v in rng.integers(0, 3, n)]
    num = [int(v) for v in rng.integers(0, 100, n)]
    table = d.Table.from_pydict({"s": ("string", s), "cat": ("string", cat), "n": ("int64", num)}).to_device(0)
    like = [d.Compliance("kw", "s LIKE '%keyword%'"), d.Compliance("re", "s RLIKE 'key.ord' AND n < 50"),
            d.Completeness("cat", "s NOT LIKE '%keyword%'")]
    others = [d.Size(), d.Completeness("s"), d.Uniqueness(["cat"]), d.Distinctness(["cat"]), d.Entropy("cat"),
              d.CountDistinct(["cat"]), d.Mean("n"), d.ApproxCountDistinct("s"), d.PatternMatch("s", "keyword")]
    mixed = d.AnalysisRunner.onData(table).addAnalyzers(like + others).run()
    plain = d.AnalysisRunner.onData(table).addAnalyzers(others).run()
    for a in others:
        assert mixed.metric(a).value.get() == plain.metric(a).value.get(), a
    t, total, nulls = counts("like", "%keyword%", s)
    assert mixed.metric(like[0]).value.get() == t / total
    want_re = sum(1 for v, k in zip(s, num) if v is not None and K.rlike_match("key.ord", v) and k < 50)
    assert mixed.metric(like[1]).value.get() == want_re / total
    assert mixed.metric(like[2]).value.get() == 1.0
    before = ColumnProfilerRunner().onData(table).run().profiles
    d.AnalysisRunner.onData(table).addAnalyzers(like).run()
    after = ColumnProfilerRunner().onData(table).run().profiles
    for name in ("s", "cat", "n"):
        assert repr(before[name]) == repr(after[name]), name
        assert before[name].completeness == after[name].completeness
