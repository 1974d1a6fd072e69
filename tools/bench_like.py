"""LIKE / RLIKE predicate timing on the GPU, next to PatternMatch of the same keyword on the same
build and the same bytes:

    (a) Compliance(_, "s LIKE '%keyword%'")     dq_match_mask_kernel + dq_pred_kernel + the mask scan
    (b) Compliance(_, "s RLIKE 'keyword'")      the same, the DFA compiled in find mode
    (c) PatternMatch("s", "keyword")            dq_regex_kernel, the counting kernel: the yardstick

    python tools/bench_like.py [--rows 100000000] [--steps 10] [--warmup 2]

One string column resident in HBM.  Its values are the six distinct `attribute` strings of the
reference's IncrementalAnalysisTest fixture (tests/golden/like_known_answers.json: 15 to 30 bytes,
one of the six holds "keyword"), drawn uniformly per row, consumed as batches of at most
--batch-rows rows (a utf8 batch addresses 2 GiB).  One step = every batch once, timed between two
HIP events on the plan's stream.  Prints one JSON line: medians in ms and the ratios (a)/(c), (b)/(c)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]


def attribute_shapes():
    with open(os.path.join(ROOT, "tests", "golden", "like_known_answers.json"), encoding="utf-8") as f:
        fx = json.load(f)
    seen = []
    for row in fx["initial"] + fx["delta"]:
        if row[2] not in seen:
            seen.append(row[2])
    return seen


def make_batch(torch, d, rows, seed, shapes):
    g = torch.Generator(device="cuda").manual_seed(seed)
    texts = [s.encode("utf-8") for s in shapes]
    tmpl = torch.tensor(list(b"".join(texts)), device="cuda", dtype=torch.uint8)
    lens = torch.tensor([len(t) for t in texts], device="cuda", dtype=torch.int64)
    starts = torch.cumsum(lens, 0) - lens
    pick = torch.randint(0, len(texts), (rows,), device="cuda", generator=g)
    row_len = lens[pick]
    offsets = torch.zeros(rows + 1, device="cuda", dtype=torch.int64)
    offsets[1:] = torch.cumsum(row_len, 0)
    total = int(offsets[-1])
    row_of_byte = torch.repeat_interleave(torch.arange(rows, device="cuda"), row_len)
    src = starts[pick][row_of_byte] + (torch.arange(total, device="cuda") - offsets[:-1][row_of_byte])
    heap = tmpl[src]
    col = d.Column("string", rows, heap, None, offsets.to(torch.int32), 0, device=True)
    return d.Table({"s": col}), total, pick


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--batch-rows", type=int, default=25_000_000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    import torch
    import deequ_amd as d
    from deequ_amd.engine import Plan, op_spec_for
    if not torch.cuda.is_available():
        raise SystemExit("bench_like.py needs the GPU: there is no CPU path to time")
    d.set_device(0)
    shapes = attribute_shapes()
    batch_rows = min(args.batch_rows, args.rows)
    n_batches = (args.rows + batch_rows - 1) // batch_rows
    batches, string_bytes, keyword_rows = [], 0, 0
    hit = [k for k, s in enumerate(shapes) if "keyword" in s]
    for b in range(n_batches):
        t, nbytes, pick = make_batch(torch, d, min(batch_rows, args.rows - b * batch_rows), b, shapes)
        batches.append(t)
        string_bytes += nbytes
        keyword_rows += sum(int((pick == k).sum()) for k in hit)
    torch.cuda.synchronize()

    def time_plan(analyzers):
        schema = batches[0].schema
        plan = Plan([op_spec_for(a, schema) for a in analyzers], schema)
        stream = torch.cuda.ExternalStream(plan.stream)
        times, state = [], None
        try:
            for step in range(args.warmup + args.steps):
                plan.reset()
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record(stream)
                for t in batches:
                    plan.consume(t)
                t1.record(stream)
                state = plan.finish_raw()[0]
                t1.synchronize()
                if step >= args.warmup:
                    times.append(t0.elapsed_time(t1))
            assert (state.num_matches, state.count) == (keyword_rows, args.rows), (state.num_matches, state.count)
        finally:
            plan.close()
        times.sort()
        return {"ms_median": round(times[len(times) // 2], 3), "ms_min": round(times[0], 3), "ms_max": round(times[-1], 3)}

    plans = {"like": [d.Compliance("like", "s LIKE '%keyword%'")],
             "rlike": [d.Compliance("rlike", "s RLIKE 'keyword'")],
             "pattern_match": [d.PatternMatch("s", "keyword")]}
    result = {"rows": args.rows, "batches": n_batches, "string_bytes": string_bytes, "keyword_rows": keyword_rows,
              "shapes_bytes": [len(s.encode("utf-8")) for s in shapes], "steps": args.steps, "warmup": args.warmup,
              "mask_bytes": (args.rows + 7) // 8}
    result["plans"] = {name: time_plan(a) for name, a in plans.items()}
    base = result["plans"]["pattern_match"]["ms_median"]
    result["like_over_pattern_match"] = round(result["plans"]["like"]["ms_median"] / base, 3)
    result["rlike_over_pattern_match"] = round(result["plans"]["rlike"]["ms_median"] / base, 3)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
