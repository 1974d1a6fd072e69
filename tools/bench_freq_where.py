"""A filtered frequency group-by (`where` folded into the key's validity on the GPU) next to what a
caller did before it existed and to the unfiltered group-by:

    (a) FrequencyTable(..., where="v > 0"): consume + summary
    (b) the surviving rows built with torch boolean indexing (a string column: its offsets and bytes
        gathered), then an unfiltered consume + summary
    (c) an unfiltered consume + summary of all rows

    python tools/bench_freq_where.py [--rows 100000000] [--kinds int64,digits12] [--steps 5]
                                     [--warmup 1] [--limit 540] [--only a,b,c]

`rows` rows generated in HBM: `--distinct` (default rows / 5) keys, int64 or 12-digit strings, and
an int64 column v with both signs, so `v > 0` keeps about half of the rows.  Every kind runs in a
process of its own under --limit seconds; the first failure stops the script.  The clocks are host
clocks around calls that end in the summary's read-back.  (a) and (b) must give the same summary.
(d), the unfiltered group-by of the parent commit, is measured from a checkout of that commit: an
older library lacks dq_freq_set_filter, which this tree's binding requires, so DEEQU_AMD_LIB cannot
name it here.  Build the parent in a directory of its own, copy this script into its tools/ (route
(c) uses nothing the parent lacks) and run both on one box, alternated:

    git worktree add ../parent HEAD~1 && make -C ../parent/deequ_amd/csrc -j8
    cp tools/bench_freq_where.py ../parent/tools/
    for i in 1 2 3; do python tools/bench_freq_where.py --only c
                       python ../parent/tools/bench_freq_where.py --only c; done

and compare the spreads.
Prints one JSON line per kind: the median, minimum and maximum of each route in ms.  No gate: the
numbers are reported ("Filtered frequencies")."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]


def make_columns(torch, d, kind, rows, distinct):
    g = torch.Generator(device="cuda").manual_seed(5)
    keys = torch.randint(0, distinct, (rows,), device="cuda", generator=g, dtype=torch.int64)
    v = torch.randint(-1000, 1000, (rows,), device="cuda", generator=g, dtype=torch.int64)
    if kind == "int64":
        k = d.Column("int64", rows, keys, None, device=True)
    else:
        pow10 = torch.tensor([10 ** (11 - j) for j in range(12)], device="cuda", dtype=torch.int64)
        chars = torch.empty((rows, 12), device="cuda", dtype=torch.uint8)
        step = 1 << 24  # (the int64 digit matrix of a slice, not of the whole column)
        for s in range(0, rows, step):
            chars[s:s + step] = ((keys[s:s + step, None] // pow10[None, :]) % 10 + 48).to(torch.uint8)
        offsets = torch.arange(rows + 1, device="cuda", dtype=torch.int32) * 12
        k = d.Column("string", rows, chars.view(-1), None, offsets=offsets, device=True)
    return k, d.Column("int64", rows, v, None, device=True), v


def gather(torch, d, kind, k, v):
    """What a caller does today: the rows where v > 0, materialised."""
    keep = v > 0
    m = int(keep.sum())
    if kind == "int64":
        return d.Table({"k": d.Column("int64", m, k.values[keep], None, device=True)}), m
    chars = k.values.view(-1, 12)[keep].contiguous().view(-1)
    offsets = torch.arange(m + 1, device="cuda", dtype=torch.int32) * 12
    return d.Table({"k": d.Column("string", m, chars, None, offsets=offsets, device=True)}), m


def spread(ms):
    s = sorted(ms)
    return {"median": round(s[len(s) // 2], 2), "min": round(s[0], 2), "max": round(s[-1], 2)}


def run_one(kind, rows, distinct, steps, warmup, only):
    import torch
    import deequ_amd as d
    from deequ_amd.frequencies import FrequencyTable
    if not torch.cuda.is_available():
        raise SystemExit("bench_freq_where.py needs the GPU: there is no CPU path to time")
    d.set_device(0)
    k, vcol, v = make_columns(torch, d, kind, rows, distinct)
    dtype = "int64" if kind == "int64" else "string"
    both = d.Table({"k": k, "v": vcol})
    torch.cuda.synchronize()
    out = {"kind": kind, "rows": rows, "distinct": distinct, "steps": steps, "warmup": warmup}
    sums = {}

    def timed(route, fn):
        ms = []
        for step in range(warmup + steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            s = fn()
            t1 = time.perf_counter()
            if step >= warmup:
                ms.append((t1 - t0) * 1e3)
        sums[route] = (s.num_rows, s.num_groups, s.num_unique, s.grouped_rows, s.entropy)
        out[route + "_ms"] = spread(ms)

    def filtered():
        t = FrequencyTable(["k"], {"k": dtype, "v": "int64"}, where="v > 0")
        t.reserve(rows)
        t.consume(both)
        s = t.summary()
        t.close()
        return s

    def gathered():
        sub, m = gather(torch, d, kind, k, v)
        t = FrequencyTable(["k"], {"k": dtype})
        t.reserve(m)
        t.consume(sub)
        s = t.summary()
        t.close()
        return s

    def unfiltered():
        t = FrequencyTable(["k"], {"k": dtype, "v": "int64"})
        t.reserve(rows)
        t.consume(both)
        s = t.summary()
        t.close()
        return s

    if "a" in only:
        timed("a_filtered", filtered)
    if "b" in only:
        timed("b_gather_then_unfiltered", gathered)
    if "c" in only:
        timed("c_unfiltered", unfiltered)
    if "a" in only and "b" in only:
        assert sums["a_filtered"] == sums["b_gather_then_unfiltered"], sums
        out["selected_rows"] = sums["a_filtered"][0]
        out["groups"] = sums["a_filtered"][1]
    if "a" in only and "c" in only:
        out["a_over_c"] = round(out["a_filtered_ms"]["median"] / out["c_unfiltered_ms"]["median"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--distinct", type=int, default=0, help="distinct keys (default: rows / 5)")
    ap.add_argument("--kinds", default="int64,digits12")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--only", default="a,b,c", help="the routes to time")
    ap.add_argument("--limit", type=int, default=540, help="seconds allowed to one kind's process")
    ap.add_argument("--one", metavar="KIND", help="(internal) run one kind in this process")
    args = ap.parse_args()
    distinct = args.distinct or max(1, args.rows // 5)
    only = args.only.split(",")
    if args.one:
        print(json.dumps(run_one(args.one, args.rows, distinct, args.steps, args.warmup, only)), flush=True)
        return 0
    for kind in args.kinds.split(","):
        if kind not in ("int64", "digits12"):
            raise SystemExit("unknown kind %r (of int64, digits12)" % kind)
        cmd = [sys.executable, os.path.abspath(__file__), "--one", kind, "--rows", str(args.rows), "--distinct",
               str(distinct), "--steps", str(args.steps), "--warmup", str(args.warmup), "--only", args.only]
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
