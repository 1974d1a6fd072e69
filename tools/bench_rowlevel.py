"""Row-level Uniqueness ("which rows hold a duplicated key?") on one MI355X, next to the group-by
that precedes it and to what a caller did before the probe existed:

    (a) the probe pass: row_level_results(data, [Uniqueness(k)], states={...}) over the state of (b),
        then .counts() and .failing_rows() (dq_rows_select), each timed on its own
    (b) the group-by: FrequencyTable consume + summary
    (c) what (a) replaces: export_flat(device=True) of the state and a torch join back to the rows
        (sort the groups' keys, searchsorted every row's key, gather its count, count == 1)

    python tools/bench_rowlevel.py [--rows 100000000] [--kinds int64,digits12] [--steps 5] [--warmup 1]
                                   [--limit 540] [--profile]

`rows` rows generated in HBM, int64 keys or 12-digit string keys, every key distinct but for 1 % of
the rows, which repeat another row's key.  Every kind runs in a process of its own under --limit
seconds; the first failure stops the script.  The clocks are host clocks around calls that end in a
device synchronise.  (a) and (c) must select the same rows.  Prints one JSON line per kind: the
median, minimum and maximum of each route in ms.  No gate: the numbers are reported (DESIGN.md,
"Row-level outcomes").

--profile runs (b), (a) and the selection once, untimed, for a kernel trace of its own:

    rocprofv3 --kernel-trace --stats -d OUT --output-format csv -- python tools/bench_rowlevel.py --profile --kinds int64

whose dq_rows_combine_kernel / dq_rows_select_* / dq_freq_probe_rows_kernel lines are the kernels'
times."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

POW10 = [10 ** (11 - j) for j in range(12)]


def make_keys(torch, rows):
    """Distinct int64 keys below 10^12 in a scrambled order; 1 % of the rows repeat their neighbour's."""
    g = torch.Generator(device="cuda").manual_seed(5)
    keys = (torch.arange(rows, device="cuda", dtype=torch.int64) * 7_919_999_983) % 999_999_999_989
    dup = torch.randint(1, rows, (max(1, rows // 100),), device="cuda", generator=g, dtype=torch.int64)
    keys[dup] = keys[dup - 1]
    return keys


def digits_column(torch, d, keys):
    rows = keys.numel()
    pow10 = torch.tensor(POW10, device="cuda", dtype=torch.int64)
    chars = torch.empty((rows, 12), device="cuda", dtype=torch.uint8)
    step = 1 << 24  # (the int64 digit matrix of a slice, not of the whole column)
    for s in range(0, rows, step):
        chars[s:s + step] = ((keys[s:s + step, None] // pow10[None, :]) % 10 + 48).to(torch.uint8)
    offsets = torch.arange(rows + 1, device="cuda", dtype=torch.int32) * 12
    return d.Column("string", rows, chars.view(-1), None, offsets=offsets, device=True)


def digits_to_int(torch, chars):
    """12-digit keys (n x 12 bytes) back to int64, slice by slice."""
    pow10 = torch.tensor(POW10, device="cuda", dtype=torch.int64)
    out = torch.empty(chars.shape[0], device="cuda", dtype=torch.int64)
    step = 1 << 24
    for s in range(0, chars.shape[0], step):
        out[s:s + step] = ((chars[s:s + step].to(torch.int64) - 48) * pow10[None, :]).sum(dim=1)
    return out


def spread(ms):
    s = sorted(ms)
    return {"median": round(s[len(s) // 2], 2), "min": round(s[0], 2), "max": round(s[-1], 2)}


def run_one(kind, rows, steps, warmup, profile):
    import torch
    import deequ_amd as d
    from deequ_amd.frequencies import FrequenciesAndNumRows, FrequencyTable
    if not torch.cuda.is_available():
        raise SystemExit("bench_rowlevel.py needs the GPU: there is no CPU path to time")
    d.set_device(0)
    keys = make_keys(torch, rows)
    dtype = "int64" if kind == "int64" else "string"
    col = d.Column("int64", rows, keys, None, device=True) if kind == "int64" else digits_column(torch, d, keys)
    data = d.Table({"k": col})
    analyzer = d.Uniqueness(["k"])
    torch.cuda.synchronize()
    out = {"kind": kind, "rows": rows, "steps": steps, "warmup": warmup}

    def group_by():
        t = FrequencyTable(["k"], {"k": dtype})
        t.reserve(rows)
        t.consume(data)
        t.summary()
        return FrequenciesAndNumRows(t)

    def probe(state):
        return d.row_level_results(data, [analyzer], states={analyzer: state})

    def join(state):
        counts, offs, blob = state.table.export_flat(device=True)
        gk = blob.view(torch.int64) if kind == "int64" else digits_to_int(torch, blob.view(-1, 12))
        order = torch.argsort(gk)
        pos = torch.searchsorted(gk[order], keys)
        unique = counts[order][pos] == 1
        failing = torch.nonzero(~unique).view(-1)
        torch.cuda.synchronize()
        return failing

    if profile:
        state = group_by()
        res = probe(state)
        out["counts"] = res.counts(analyzer)
        out["failing"] = int(res.failing_rows(analyzer).numel())
        return out

    def timed(route, fn):
        ms, last = [], None
        for step in range(warmup + steps):
            if hasattr(last, "table"):  # (one state at a time: a table of 10^8 groups is 8.6 GB)
                last.table.close()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            last = fn()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            if step >= warmup:
                ms.append((t1 - t0) * 1e3)
        out[route + "_ms"] = spread(ms)
        return last

    state = timed("b_group_by", group_by)
    res = timed("a_probe", lambda: probe(state))

    def fresh_counts():
        res._counts.clear()
        return res.counts(analyzer)
    out["counts"] = timed("a_counts", fresh_counts)
    failing = timed("a_failing_rows", lambda: res.failing_rows(analyzer))
    joined = timed("c_export_and_join", lambda: join(state))
    assert torch.equal(failing, joined), "the probe and the join select different rows"
    s = state.summary()
    assert out["counts"][0] == s.num_unique and out["counts"][0] + out["counts"][1] == s.num_rows
    out["failing"] = int(failing.numel())
    out["groups"] = s.num_groups
    out["a_probe_over_b"] = round(out["a_probe_ms"]["median"] / out["b_group_by_ms"]["median"], 3)
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
