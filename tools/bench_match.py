"""Cross-table checks on one MI355X: dataset match and referential integrity of a table A against a
reference B, next to B's group-by and to what a caller did before the kernels existed:

    (a) dataset_match(A, B, keys, compare): the whole call, and its steps on their own -- B's
        group-by (c), the index step (dq_freq_index_rows) and the match pass (dq_freq_match_rows)
    (b) referential_integrity(A, keys, reference_state=state of (c)): the probe pass alone
    (c) B's group-by: FrequencyTable consume + summary
    (d) int64 keys only, what (a) replaces: torch argsort of B's keys, searchsorted of A's, gather of
        B's cells, compare

    python tools/bench_match.py [--rows 100000000] [--kinds int64,digits12] [--steps 5] [--warmup 1]
                                [--limit 540] [--profile]

`rows` rows in A and in B, generated in HBM: B's keys are a permutation of A's, 1 % of A's keys are
absent from B, 1 % of A's cells differ.  int64 keys or 12-digit string keys; compare columns int64,
float64 and a 12-byte string.  Every kind runs in a process of its own under --limit seconds; the
first failure stops the script.  The clocks are host clocks around calls that end in a device
synchronise.  (a) and (d) must select the same rows.  Prints one JSON line per kind: the median,
minimum and maximum of each route in ms, and the ratios of (a), (b) and (c) to (d) and to (c).  No
gate: the numbers are reported ("Cross-table checks").

Per row of A the match pass reads, at least: its key (8 or 12 + 4 B), one 32-B slot and one 8-B
row_of_slot entry at a random address (issued together), then B's cells at a second random address
(8 + 8 + 12 B and 8 B of offsets), A's cells in order (8 + 8 + 12 + 4 B); it writes 1 bit: about 130 B,
in two dependent random reads (a key that sits past its first probe position pays a third).

--profile runs (c), the index and the match once, untimed, for a kernel trace of its own:

    rocprofv3 --kernel-trace --stats -d OUT --output-format csv -- python tools/bench_match.py --profile --kinds int64
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

POW10 = [10 ** (11 - j) for j in range(12)]
MUL, MOD = 7_919_999_983, 999_999_999_989  # (a prime modulus: distinct indices give distinct keys)


def digits_column(torch, d, keys):
    """int64 values below 10^12 as a 12-digit string column, slice by slice."""
    rows = keys.numel()
    pow10 = torch.tensor(POW10, device="cuda", dtype=torch.int64)
    chars = torch.empty((rows, 12), device="cuda", dtype=torch.uint8)
    step = 1 << 24
    for s in range(0, rows, step):
        chars[s:s + step] = ((keys[s:s + step, None] // pow10[None, :]) % 10 + 48).to(torch.uint8)
    offsets = torch.arange(rows + 1, device="cuda", dtype=torch.int32) * 12
    return d.Column("string", rows, chars.view(-1), None, offsets=offsets, device=True)


def make_tables(torch, d, rows, kind):
    """(A, B, A's keys and B's keys as int64 tensors)."""
    g = torch.Generator(device="cuda").manual_seed(5)
    idx = torch.arange(rows, device="cuda", dtype=torch.int64)
    keys = (idx * MUL) % MOD
    ci = keys ^ 0x5555
    cf = keys.double() * 0.5
    cs = (keys * 31) % (10 ** 12)
    perm = torch.randperm(rows, device="cuda", generator=g)
    b_keys, b_ci, b_cf, b_cs = keys[perm], ci[perm], cf[perm], cs[perm]
    n1 = max(1, rows // 100)
    absent = torch.randint(0, rows, (n1,), device="cuda", generator=g, dtype=torch.int64)
    a_keys = keys.clone()
    a_keys[absent] = ((absent + rows) * MUL) % MOD  # (indices past `rows`: keys no row of B has)
    for t, bump in ((ci, 1), (cf, 0.25), (cs, 1)):
        rows_hit = torch.randint(0, rows, (max(1, n1 // 3),), device="cuda", generator=g, dtype=torch.int64)
        t[rows_hit] = (t[rows_hit] + bump) % (10 ** 12) if t is cs else t[rows_hit] + bump

    def table(k, i, f, s):
        kcol = d.Column("int64", rows, k, None, device=True) if kind == "int64" else digits_column(torch, d, k)
        return d.Table({"k": kcol, "i": d.Column("int64", rows, i, None, device=True),
                        "f": d.Column("float64", rows, f, None, device=True), "s": digits_column(torch, d, s)})
    return table(a_keys, ci, cf, cs), table(b_keys, b_ci, b_cf, b_cs), a_keys, b_keys


def spread(ms):
    s = sorted(ms)
    return {"median": round(s[len(s) // 2], 2), "min": round(s[0], 2), "max": round(s[-1], 2)}


def run_one(kind, rows, steps, warmup, profile):
    import torch
    import deequ_amd as d
    from deequ_amd import comparison
    from deequ_amd.frequencies import FrequenciesAndNumRows
    if not torch.cuda.is_available():
        raise SystemExit("bench_match.py needs the GPU: there is no CPU path to time")
    d.set_device(0)
    A, B, a_keys, b_keys = make_tables(torch, d, rows, kind)
    compare = [("i", "i"), ("f", "f"), ("s", "s")]
    b_key_table = comparison._as_table(B, ["k"])
    torch.cuda.synchronize()
    out = {"kind": kind, "rows": rows, "steps": steps, "warmup": warmup, "algorithmic_bytes_per_row": 130,
           "dependent_random_reads_per_row": 2}

    def group_by():
        table, _ = comparison._reference_table(B, ["k"], "bench")
        table.summary()
        return table

    def index(table):
        comparison._index(table, b_key_table)
        return table

    def match(table):
        return comparison._match(A, table, ["k"], ["k"], compare, B, None, False)

    def join():
        order = torch.argsort(b_keys)
        sorted_keys = b_keys[order]
        pos = torch.searchsorted(sorted_keys, a_keys).clamp_(max=rows - 1)
        ok = sorted_keys[pos] == a_keys
        j = order[pos]
        ok &= A.columns["i"].values == B.columns["i"].values[j]
        ok &= A.columns["f"].values == B.columns["f"].values[j]
        ok &= (A.columns["s"].values.view(-1, 12) == B.columns["s"].values.view(-1, 12)[j]).all(dim=1)
        true_rows = torch.nonzero(ok).view(-1)
        torch.cuda.synchronize()
        return true_rows

    if profile:
        res = match(index(group_by()))
        out["counts"] = res.counts._asdict()
        return out

    def timed(route, fn, close=None):
        ms, last = [], None
        for step in range(warmup + steps):
            if close is not None and last is not None:  # (one table at a time: 10^8 groups are 8.6 GB of slots)
                close(last)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            last = fn()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            if step >= warmup:
                ms.append((t1 - t0) * 1e3)
        out[route + "_ms"] = spread(ms)
        return last

    table = timed("c_group_by", group_by, close=lambda t: t.close())
    # (the warm-up step allocates the map and fills it with -1; every step writes all its entries again)
    timed("a_index", lambda: index(table))
    res = timed("a_match", lambda: match(table))
    out["counts"] = res.counts._asdict()
    state = FrequenciesAndNumRows(table)
    ri = timed("b_referential_integrity", lambda: d.referential_integrity(A, ["k"], reference_state=state))
    out["ri_counts"] = ri.counts._asdict()
    true_rows = res.rows("true")
    table.close()
    total = timed("a_dataset_match_total", lambda: d.dataset_match(A, B, ["k"], compare))
    assert total.counts == res.counts
    del total
    if kind == "int64":
        joined = timed("d_torch_join", join)
        assert torch.equal(true_rows, joined), "the match and the torch join select different rows"
    c = out["counts"]
    assert c["matched"] + c["key_null"] + c["key_absent"] + c["cells_differ"] == c["selected"] == rows
    assert out["ri_counts"]["matched"] == rows - c["key_absent"] - c["key_null"]
    med = lambda r: out[r + "_ms"]["median"]  # noqa: E731
    out["a_steps_ms"] = round(med("c_group_by") + med("a_index") + med("a_match"), 2)
    for route in ("a_dataset_match_total", "a_index", "a_match", "b_referential_integrity"):
        out[route + "_over_c"] = round(med(route) / med("c_group_by"), 3)
    if kind == "int64":
        for route in ("a_dataset_match_total", "b_referential_integrity", "c_group_by"):
            out[route + "_over_d"] = round(med(route) / med("d_torch_join"), 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--kinds", default="int64,digits12")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--limit", type=int, default=540, help="seconds allowed to one kind's process")
    ap.add_argument("--profile", action="store_true", help="one untimed pass (for a kernel trace)")
    ap.add_argument("--one", metavar="KIND", help="(internal) run one kind in this process")
    args = ap.parse_args()
    if args.one:
        print(json.dumps(run_one(args.one, args.rows, args.steps, args.warmup, args.profile)), flush=True)
        return 0
    for kind in args.kinds.split(","):
        if kind not in ("int64", "digits12"):
            raise SystemExit("unknown kind %r (of int64, digits12)" % kind)
        if args.profile:  # (in this process: the profiler traces the program it was given)
            print(json.dumps(run_one(kind, args.rows, args.steps, args.warmup, True)), flush=True)
            continue
        cmd = [sys.executable, os.path.abspath(__file__), "--one", kind, "--rows", str(args.rows),
               "--steps", str(args.steps), "--warmup", str(args.warmup)]
        try:
            p = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=args.limit)
        except subprocess.TimeoutExpired:
            print(json.dumps({"failed": kind, "reason": "time limit of %d s" % args.limit}), flush=True)
            return 1
        if p.returncode != 0:
            print(json.dumps({"failed": kind, "exit_status": p.returncode}), flush=True)
            return 1
        print(p.stdout.decode().strip().splitlines()[-1], flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
