"""PatternMatch on the GPU (dq_regex_kernel) against the oracle of test_pattern_match.py --
Python's re.search(p, s, re.ASCII) with a non-empty group 0: row counts around the wave and
workgroup sizes, 0..70-character strings with ~5 % NULLs and one 64 KiB row, host and device
buffers, a sliced column, `where` filters (one selecting nothing), several PatternMatch ops beside
other analyzers in one plan, batches, reset, the reference's known answers through AnalysisRunner,
and a 2-rank run."""
import ctypes
import os
import socket

import numpy as np
import pytest

import pattern_cases as C

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SSN_SHAPE = r"\d{3}-\d{2}-\d{4}"
PATS = (C.URL, C.EMAIL, SSN_SHAPE)

_POOL = {}


def pool():
    """3 x 1500 strings (mutated URLs, e-mail addresses, number shapes) and the oracle's answer for
    each of PATS on each string: computed once, shared by every test, never modified."""
    if not _POOL:
        strings = []
        for k, p in enumerate(PATS):
            seeds = next(s for q, s in C.PATTERNS if q == p)
            strings += C.make_strings(seeds, 1500, np.random.default_rng(77 + k))
        _POOL["strings"] = strings
        _POOL["want"] = {p: np.array([C.oracle(p, s) for s in strings], dtype=np.int64) for p in PATS}
        for p in PATS:
            assert 0.1 <= _POOL["want"][p].mean() <= 0.9, p
    return _POOL["strings"], _POOL["want"]


def rows(n, seed, null_frac=0.05):
    """n rows drawn from the pool (NULL with probability null_frac): (values, pool indices or -1)."""
    strings, _ = pool()
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, len(strings), n)
    idx[rng.random(n) < null_frac] = -1
    if n >= 1000:
        assert (idx < 0).any()
    return [None if i < 0 else strings[i] for i in idx], idx


def expect(pattern, idx, selected=None):
    """(matches, count) of the oracle over the drawn rows (NULL rows count, and match nothing)."""
    _, want = pool()
    sel = np.ones(len(idx), dtype=bool) if selected is None else np.asarray(selected, dtype=bool)
    hit = np.where(idx >= 0, want[pattern][np.maximum(idx, 0)], 0)
    return int(hit[sel].sum()), int(sel.sum())


def run_plan(d, analyzers, batches, schema):
    from deequ_amd.engine import Plan, op_spec_for
    plan = Plan([op_spec_for(a, schema) for a in analyzers], schema)
    try:
        for b in batches:
            plan.consume(b)
        return [(s.kind, s.has_value, s.num_matches, s.count) for s in plan.finish_raw()][:len(analyzers)]
    finally:
        plan.close()


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000, 100003])
def test_row_counts_against_oracle(gpu, n, device):
    import deequ_amd as d
    vals, idx = rows(n, seed=n)
    if n == 1:
        assert vals[0] is not None
    table = d.Table.from_pydict({"s": ("string", vals)})
    if device:
        table = table.to_device(0)
    an = [d.PatternMatch("s", p) for p in PATS]
    got = run_plan(d, an, [table], table.schema)
    for p, g in zip(PATS, got):
        m, c = expect(p, idx)
        print("n=%d %s: %r, oracle (%d, %d)" % (n, "device" if device else "host", g, m, c))
        assert g == (14, 1, m, c), (p[:20], g, m, c)
    if n == 100003:  # more than one workgroup per task took part
        assert got[0][3] == 100003 and 0 < got[0][2] < 100003


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_long_rows(gpu, device):
    """64 KiB rows: the match in the last bytes, no match at all, a match in the first bytes (the
    lane leaves the loop), beside short rows and an empty one; byte lengths that end in the
    16-byte, 4-byte and 1-byte load loops."""
    import deequ_amd as d
    long_hit = "z" * (65536 - 11) + "111-05-1130"
    long_miss = "9-" * 32768
    long_early = "078-05-1120" + "é" * 32000
    vals = [long_hit, "", None, long_miss, "111-05-113", long_early, "x111-05-1130", "1" * 15 + "111-05-1130" + "y" * 6,
            "例" * 5 + "111-05-11301", "111-05-1", "111-05-1130", "111-05-1130\n"]
    assert len(long_hit.encode()) == 65536 and len(long_miss.encode()) == 65536
    table = d.Table.from_pydict({"s": ("string", vals)})
    if device:
        table = table.to_device(0)
    want = sum(C.oracle(SSN_SHAPE, v) for v in vals if v is not None)
    assert want == 7
    got = run_plan(d, [d.PatternMatch("s", SSN_SHAPE), d.PatternMatch("s", "^" + SSN_SHAPE + "$")], [table], table.schema)
    assert got[0] == (14, 1, want, len(vals))
    assert got[1] == (14, 1, sum(C.oracle("^" + SSN_SHAPE + "$", v) for v in vals if v is not None), len(vals))


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_sliced_column(gpu, device):
    """A column whose Arrow `offset` is not zero (nor a multiple of 8: the validity bitmap is realigned)."""
    import deequ_amd as d
    n, k = 5000, 13
    vals, idx = rows(n, seed=5)
    whole = d.Column.from_pylist(vals, "string")
    assert whole.validity is not None
    sliced = d.Column("string", n - k, whole.values, whole.validity, whole.offsets, offset=k)
    if device:
        sliced = sliced.to_device(0)
    table = d.Table({"s": sliced})
    got = run_plan(d, [d.PatternMatch("s", p) for p in PATS], [table], table.schema)
    for p, g in zip(PATS, got):
        m, c = expect(p, idx[k:])
        assert g == (14, 1, m, c), (p[:20], g, m, c)


def test_where_filters(gpu):
    import deequ_amd as d
    n = 4000
    vals, idx = rows(n, seed=9)
    rng = np.random.default_rng(10)
    iv = rng.integers(0, 10, n)
    inull = rng.random(n) < 0.1
    table = d.Table.from_pydict({"s": ("string", vals),
                                 "i": ("int64", [None if z else int(x) for x, z in zip(iv, inull)])}).to_device(0)
    some = (iv > 5) & ~inull
    an = [d.PatternMatch("s", C.URL, "i > 5"), d.PatternMatch("s", C.URL, "i > 1000"), d.PatternMatch("s", C.URL),
          d.PatternMatch("s", C.EMAIL, "i > 5"), d.PatternMatch("s", C.EMAIL, "i IS NULL")]
    got = run_plan(d, an, [table], table.schema)
    assert got[0] == (14, 1) + expect(C.URL, idx, some)
    assert got[1][:2] == (14, 0)  # no row selected: the sum over zero rows is NULL -> None
    assert got[2] == (14, 1) + expect(C.URL, idx)
    assert got[3] == (14, 1) + expect(C.EMAIL, idx, some)
    assert got[4] == (14, 1) + expect(C.EMAIL, idx, inull)
    ctx = d.AnalysisRunner.onData(table).addAnalyzers(an).run()
    m, c = expect(C.URL, idx, some)
    assert ctx.metric(an[0]).value.get() == m / c
    none = ctx.metric(an[1]).value
    assert none.isFailure and isinstance(none.exception, d.EmptyStateException)
    # an empty table: no row at all, also None
    empty = d.Table.from_pydict({"s": ("string", []), "i": ("int64", [])})
    assert run_plan(d, an[2:3], [empty], empty.schema)[0][:2] == (14, 0)


def test_three_patterns_beside_other_analyzers(gpu):
    """Two patterns on one column and one on another in one plan, with Completeness and MinLength:
    the other ops' states are, byte for byte, those of a plan without PatternMatch."""
    import deequ_amd as d
    from deequ_amd.engine import Plan, op_spec_for
    n = 30000
    v1, i1 = rows(n, seed=21)
    v2, i2 = rows(n, seed=22)
    table = d.Table.from_pydict({"a": ("string", v1), "b": ("string", v2)}).to_device(0)
    others = [d.Completeness("a"), d.MinLength("a"), d.MinLength("b"), d.ApproxCountDistinct("b"), d.DataType("b")]
    pm = [d.PatternMatch("a", C.URL), d.PatternMatch("a", C.EMAIL), d.PatternMatch("b", C.URL)]
    mixed = [pm[0], others[0], pm[1], others[1], others[2], pm[2], others[3], others[4], d.PatternMatch("a", C.URL)]

    def states(an):
        plan = Plan([op_spec_for(a, table.schema) for a in an], table.schema)
        try:
            plan.consume(table)
            return [bytes(s) for s in plan.finish_raw()][:len(an)]
        finally:
            plan.close()
    with_pm, without = dict(zip(map(str, mixed), states(mixed))), dict(zip(map(str, others), states(others)))
    for a in others:
        assert with_pm[str(a)] == without[str(a)], a
    got = run_plan(d, pm, [table], table.schema)
    assert got[0] == (14, 1) + expect(C.URL, i1)
    assert got[1] == (14, 1) + expect(C.EMAIL, i1)
    assert got[2] == (14, 1) + expect(C.URL, i2)
    full = run_plan(d, mixed, [table], table.schema)
    assert [full[0], full[2], full[5], full[8]] == [got[0], got[1], got[2], got[0]]
    assert full[1][0] == 2 and full[3][0] == 11


def test_batches_accumulate_and_reset_clears(gpu):
    import deequ_amd as d
    from deequ_amd.engine import Plan, op_spec_for
    n = 9001
    vals, idx = rows(n, seed=31)
    cuts = [0, 2999, 3000, n]
    parts = [d.Table.from_pydict({"s": ("string", vals[a:b])}) for a, b in zip(cuts, cuts[1:])]
    whole = d.Table.from_pydict({"s": ("string", vals)})
    an = [d.PatternMatch("s", C.URL), d.PatternMatch("s", C.EMAIL)]
    one = run_plan(d, an, [whole], whole.schema)
    assert one == run_plan(d, an, parts, whole.schema)
    assert one == run_plan(d, an, [p.to_device(0) for p in parts], whole.schema)
    assert one[0] == (14, 1) + expect(C.URL, idx)
    plan = Plan([op_spec_for(a, whole.schema) for a in an], whole.schema)
    try:
        plan.consume(whole)
        plan.consume(parts[0])
        first = [(s.num_matches, s.count) for s in plan.finish_raw()][:2]
        assert first[0] == tuple(x + y for x, y in zip(expect(C.URL, idx), expect(C.URL, idx[:2999])))
        plan.reset()
        assert [(s.has_value, s.num_matches, s.count) for s in plan.finish_raw()][:2] == [(0, 0, 0), (0, 0, 0)]
        plan.reset()
        plan.consume(parts[1])
        assert [(s.has_value, s.num_matches, s.count) for s in plan.finish_raw()][0] == (1,) + expect(C.URL, idx[2999:3000])
    finally:
        plan.close()


def test_packed_plan_equals_struct_plan(gpu):
    import deequ_amd as d
    from deequ_amd import _lib as L
    from deequ_amd.engine import Plan, op_spec_for, pack_ops
    from deequ_amd.table import dq_columns
    n = 2000
    vals, idx = rows(n, seed=41)
    table = d.Table.from_pydict({"s": ("string", vals)})
    an = [d.PatternMatch("s", C.URL), d.Completeness("s"), d.PatternMatch("s", C.EMAIL, "s IS NOT NULL")]
    specs = [op_spec_for(a, table.schema) for a in an]
    ref = Plan(specs, table.schema)
    ref.consume(table)
    want = bytes(ref.finish_raw())
    ref.close()
    blob = pack_ops(specs)
    types = (ctypes.c_int32 * 1)(L.DQ_T_UTF8)
    h = ctypes.c_void_p()
    L.check(L.lib().dq_plan_create_packed(L.Context.get(d.current_device()).handle, blob, len(blob), types, 1, ctypes.byref(h)))
    try:
        L.check(L.lib().dq_plan_consume(h, dq_columns(table, ["s"]), 1, n))
        out = (L.DqState * 3)()
        L.check(L.lib().dq_plan_finish(h, out, 3))
        assert bytes(out) == want
        assert (out[0].num_matches, out[0].count) == expect(C.URL, idx)
    finally:
        L.lib().dq_plan_destroy(h)
    bad = pack_ops([op_spec_for(d.PatternMatch("s", C.SSN), table.schema)])
    st = L.lib().dq_plan_create_packed(L.Context.get(d.current_device()).handle, bad, len(bad), types, 1, ctypes.byref(h))
    assert st == L.DQ_ERR_UNSUPPORTED and "look-around" in L.lib().dq_last_error().decode()


def test_known_answers_through_the_runner(gpu):
    """AnalyzerTests.scala:664-753: the reference's own expectations; the two patterns outside the
    exact subset are declined (the JVM caller routes them to Spark), never approximated."""
    import deequ_amd as d
    from deequ_amd import _lib as L
    fx = C.known_answers()
    assert len(fx["cases"]) == 6
    for case in fx["cases"]:
        table = d.Table.from_pydict({fx["column"]: ("string", case["values"])})
        a = d.PatternMatch(fx["column"], case["pattern"])
        value = d.AnalysisRunner.onData(table).addAnalyzers([a, d.Size()]).run().metric(a).value
        if case["expect"] == "DQ_ERR_UNSUPPORTED":
            # (the failure metric wraps the library's status, MetricCalculationException.wrapIfNecessary)
            assert value.isFailure and isinstance(value.exception.__cause__, L.UnsupportedOnGpu), (case["id"], value)
            assert value.exception.__cause__.status == L.DQ_ERR_UNSUPPORTED
        else:
            assert value.get() == case["expect"], (case["id"], value.get())
            assert a.calculate(table).value.get() == case["expect"]
            want = sum(C.oracle(case["pattern"], v) for v in case["values"] if v is not None) / len(case["values"])
            assert want == case["expect"], case["id"]  # the oracle agrees with the reference


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


N_SHARDED = 20000


def _sharded_analyzers(d):
    return [d.PatternMatch("s", C.URL), d.PatternMatch("s", C.EMAIL, "i > 5"), d.PatternMatch("s", SSN_SHAPE, "i > 1000"),
            d.Completeness("s"), d.Size()]


def _sharded_spec(lo, hi):
    vals, idx = rows(N_SHARDED, seed=51)
    iv = np.random.default_rng(52).integers(0, 10, N_SHARDED)
    return {"s": ("string", vals[lo:hi]), "i": ("int64", [int(x) for x in iv[lo:hi]])}, idx, iv


def _values(ctx, analyzers):
    out = []
    for a in analyzers:
        v = ctx.metric(a).value
        out.append(v.get() if v.isSuccess else ("failure", type(v.exception).__name__))
    return out


def _worker(rank, world, port, q):
    import sys
    sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
    import torch.distributed as dist
    import deequ_amd as d
    from deequ_amd.distributed import ShardedTable
    d.set_device(0)
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=world)
    lo, hi = rank * N_SHARDED // world, (rank + 1) * N_SHARDED // world
    an = _sharded_analyzers(d)
    shard = d.Table.from_pydict(_sharded_spec(lo, hi)[0])
    res = {"sharded": _values(d.AnalysisRunner.onData(ShardedTable(shard)).addAnalyzers(an).run(), an)}
    if rank == 0:
        whole = d.Table.from_pydict(_sharded_spec(0, N_SHARDED)[0])
        res["whole"] = _values(d.AnalysisRunner.onData(whole).addAnalyzers(an).run(), an)
    q.put((rank, res))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_equal_one(gpu):
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    results = dict(q.get(timeout=240) for _ in range(2))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    _, idx, iv = _sharded_spec(0, N_SHARDED)
    m, c = expect(C.URL, idx)
    m2, c2 = expect(C.EMAIL, idx, iv > 5)
    assert results[0]["whole"][:2] == [m / c, m2 / c2]
    assert results[0]["whole"][2] == ("failure", "EmptyStateException")
    assert results[0]["sharded"] == results[0]["whole"] == results[1]["sharded"]
