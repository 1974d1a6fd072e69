"""PatternMatch timing on the GPU: EMAIL, URL and \\d{3}-\\d{2}-\\d{4}, each as a plan of its own, a
plan holding all three, and a plan holding only MinLength on the same column (it reads the same
offsets and bytes: the yardstick).  All in one process, on strings generated in HBM.

    python tools/bench_pattern.py [--rows 100000000] [--steps 10] [--warmup 2]

A utf8 batch addresses its bytes with int32 offsets (2 GiB), so the rows are consumed as batches
of at most --batch-rows rows of 16..32 bytes; one step = consume every batch, then finish.  The
timed interval is the consumes (every kernel of the step), between two HIP events on the plan's
stream; dq_plan_finish's read-back of a few counters follows the second event and is not in it.  Prints one
JSON line: ms per step, the ratio to MinLength, string bytes per second, every pattern's table
shape (states x columns) and match rate."""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]


def fixture_pattern(case_id):
    with open(os.path.join(ROOT, "tests", "golden", "pattern_match_known_answers.json"), encoding="utf-8") as f:
        return next(c["pattern"] for c in json.load(f)["cases"] if c["id"] == case_id)


def make_batch(torch, d, rows, seed):
    """`rows` strings of 16..32 bytes over letters, digits and the punctuation the patterns look for."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    lens = torch.randint(16, 33, (rows,), device="cuda", generator=g, dtype=torch.int32)
    offsets = torch.zeros(rows + 1, device="cuda", dtype=torch.int32)
    offsets[1:] = torch.cumsum(lens, 0, dtype=torch.int64).to(torch.int32)
    total = int(offsets[-1].item())
    alphabet = torch.tensor(list(b"abcdefghijklmnopqrstuvwxyz0123456789@.-/:"), device="cuda", dtype=torch.uint8)
    values = torch.empty(total + 16, device="cuda", dtype=torch.uint8)
    step = 1 << 26
    for lo in range(0, total, step):
        n = min(step, total - lo)
        values[lo:lo + n] = alphabet[torch.randint(0, len(alphabet), (n,), device="cuda", generator=g)]
    col = d.Column("string", rows, values, None, offsets, 0, device=True)
    return d.Table({"s": col}), total


def table_shape(L, pattern):
    pb = pattern.encode("utf-8")
    m, ns, nc = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
    L.check(L.lib().dq_diag_regex_match(pb, len(pb), b"", 0, ctypes.byref(m), ctypes.byref(ns), ctypes.byref(nc)))
    return [ns.value, nc.value]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--batch-rows", type=int, default=25_000_000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    import torch
    import deequ_amd as d
    from deequ_amd import _lib as L
    from deequ_amd.engine import Plan, op_spec_for
    if not torch.cuda.is_available():
        raise SystemExit("bench_pattern.py needs the GPU: there is no CPU path to time")
    d.set_device(0)
    batch_rows = min(args.batch_rows, args.rows)
    n_batches = (args.rows + batch_rows - 1) // batch_rows
    batches, string_bytes = [], 0
    for b in range(n_batches):
        rows = min(batch_rows, args.rows - b * batch_rows)
        t, nbytes = make_batch(torch, d, rows, seed=b)
        batches.append(t)
        string_bytes += nbytes
    torch.cuda.synchronize()
    schema = batches[0].schema
    patterns = {"email": fixture_pattern("pattern_email"), "url": fixture_pattern("pattern_url"),
                "ssn_shape": r"\d{3}-\d{2}-\d{4}"}
    plans = {name: [d.PatternMatch("s", p)] for name, p in patterns.items()}
    plans["all_three"] = [d.PatternMatch("s", p) for p in patterns.values()]
    plans["min_length"] = [d.MinLength("s")]

    def time_plan(analyzers):
        plan = Plan([op_spec_for(a, schema) for a in analyzers], schema)
        stream = torch.cuda.ExternalStream(plan.stream)
        times, states = [], None
        try:
            for step in range(args.warmup + args.steps):
                plan.reset()
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record(stream)
                for t in batches:
                    plan.consume(t)
                t1.record(stream)
                out = plan.finish_raw()
                t1.synchronize()
                if step >= args.warmup:
                    times.append(t0.elapsed_time(t1))
                states = [(s.has_value, s.num_matches, s.count, s.value) for s in out][:len(analyzers)]
        finally:
            plan.close()
        times.sort()
        return times, states

    result = {"rows": args.rows, "batches": n_batches, "string_bytes": string_bytes, "steps": args.steps,
              "warmup": args.warmup, "plans": {}}
    for name, analyzers in plans.items():
        times, states = time_plan(analyzers)
        med = times[len(times) // 2]
        result["plans"][name] = {"ms_median": round(med, 3), "ms_min": round(times[0], 3), "ms_max": round(times[-1], 3),
                                 "string_GBps": round(string_bytes / med / 1e6, 1)}
        if name != "min_length":
            result["plans"][name]["match_rate"] = [round(s[1] / s[2], 6) for s in states]
            assert all(s[2] == args.rows for s in states), states
    base = result["plans"]["min_length"]["ms_median"]
    for name in plans:
        result["plans"][name]["ratio_to_min_length"] = round(result["plans"][name]["ms_median"] / base, 3)
    result["tables"] = {name: table_shape(L, p) for name, p in patterns.items()}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
