"""RowLevelSchemaValidator timing on the GPU: `validate` of a three-column schema -- an int column, a
decimal(10, 2) column and a string column with maxLength and the EMAIL pattern -- at about 90 % valid
rows, next to two existing plans run in the same process on the same columns: MinLength (the
read-once floor the PatternMatch table already uses; over the string column alone and over all three
columns) and PatternMatch of the same pattern.

    python tools/bench_schema.py [--rows 100000000] [--steps 10] [--warmup 2]

The rows are generated in HBM and consumed as batches of at most --batch-rows rows (a utf8 batch
addresses 2 GiB).  One step = every batch once.  Timed between two HIP events: the whole `validate`
(evaluate, select, allocation of the outputs, gather), and separately dq_schema_validate alone
(evaluate, combine, scans, select, the output offsets: everything but the gathers).  Prints one JSON
line: medians in ms, ratios to the two plans, and the bytes compaction writes against the bytes of
the selected rows."""
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


def fixed_width_column(torch, d, rows, g, template, classes, bad_rate, bad_at, bad_byte):
    """`rows` cells of len(template) bytes: template byte 'a' = a random letter, '0' = a random digit,
    anything else itself; a share `bad_rate` of the cells gets `bad_byte` at position `bad_at`."""
    width = len(template)
    cells = torch.empty((rows, width), device="cuda", dtype=torch.uint8)
    for k, ch in enumerate(template):
        if ch in classes:
            lo, hi = classes[ch]
            cells[:, k] = torch.randint(lo, hi + 1, (rows,), device="cuda", generator=g, dtype=torch.uint8)
        else:
            cells[:, k] = ord(ch)
    bad = torch.rand(rows, device="cuda", generator=g) < bad_rate
    cells[bad, bad_at] = bad_byte
    offsets = torch.arange(0, (rows + 1) * width, width, device="cuda", dtype=torch.int64).to(torch.int32)
    return d.Column("string", rows, cells.reshape(-1), None, offsets, 0, device=True), rows * width


def make_batch(torch, d, rows, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    classes = {"a": (ord("a"), ord("z")), "0": (ord("0"), ord("9"))}
    ident, b0 = fixed_width_column(torch, d, rows, g, "000000", classes, 0.03, 0, ord("x"))
    amount, b1 = fixed_width_column(torch, d, rows, g, "00000.00", classes, 0.03, 2, ord("#"))
    email, b2 = fixed_width_column(torch, d, rows, g, "aaaaaaaa@aaaaaa.org", classes, 0.04, 8, ord("-"))
    return d.Table({"id": ident, "amount": amount, "email": email}), b0 + b1 + b2


def table_bytes(table):
    total = 0
    for c in table.columns.values():
        for buf in (c.values, c.validity, c.offsets):
            if buf is not None:
                total += buf.numel() * buf.element_size()
    return total


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
    from deequ_amd.schema import _Validator
    from deequ_amd.table import dq_columns
    if not torch.cuda.is_available():
        raise SystemExit("bench_schema.py needs the GPU: there is no CPU path to time")
    d.set_device(0)
    batch_rows = min(args.batch_rows, args.rows)
    n_batches = (args.rows + batch_rows - 1) // batch_rows
    batches, string_bytes = [], 0
    for b in range(n_batches):
        t, nbytes = make_batch(torch, d, min(batch_rows, args.rows - b * batch_rows), seed=b)
        batches.append(t)
        string_bytes += nbytes
    torch.cuda.synchronize()
    data = d.PartitionedTable(batches)
    email = fixture_pattern("pattern_email")
    schema = d.RowLevelSchema().withIntColumn("id").withDecimalColumn("amount", 10, 2) \
        .withStringColumn("email", maxLength=32, matches=email)

    def timed(fn):
        times, last = [], None
        for step in range(args.warmup + args.steps):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            last = fn()
            t1.record()
            t1.synchronize()
            if step >= args.warmup:
                times.append(t0.elapsed_time(t1))
            if step < args.warmup + args.steps - 1:
                last = None  # (the outputs of one step are freed before the next)
        times.sort()
        return {"ms_median": round(times[len(times) // 2], 3), "ms_min": round(times[0], 3),
                "ms_max": round(times[-1], 3)}, last

    result = {"rows": args.rows, "batches": n_batches, "string_bytes": string_bytes, "steps": args.steps,
              "warmup": args.warmup}
    # the whole validate
    result["validate"], res = timed(lambda: d.RowLevelSchemaValidator.validate(data, schema))
    result["valid_fraction"] = round(res.numValidRows / args.rows, 4)
    result["invalid_fraction"] = round(res.numInvalidRows / args.rows, 4)
    out_bytes = sum(table_bytes(t) for t in res.validRows.parts + res.invalidRows.parts)
    widths = {"id": 6, "amount": 8, "email": 19}
    selected = (res.numValidRows + res.numInvalidRows) * (sum(widths.values()) + 4 * len(widths))
    result["compaction"] = {"output_bytes": out_bytes, "selected_rows_input_bytes": selected,
                            "ratio": round(out_bytes / selected, 3)}
    res = None

    # dq_schema_validate alone: evaluate + combine + scans + select + output offsets, no gather
    v = _Validator(schema, data.schema, 0)
    nv, ni = ctypes.c_int64(), ctypes.c_int64()

    def evaluate_only():
        for t in batches:
            L.check(L.lib().dq_schema_validate(v.handle, dq_columns(t, v.names), len(v.names), t.num_rows,
                                               ctypes.byref(nv), ctypes.byref(ni), None))
    result["evaluate_and_select"], _ = timed(evaluate_only)
    v.close()

    def time_plan(analyzers):
        table_schema = batches[0].schema
        plan = Plan([op_spec_for(a, table_schema) for a in analyzers], table_schema)
        stream = torch.cuda.ExternalStream(plan.stream)
        times = []
        try:
            for step in range(args.warmup + args.steps):
                plan.reset()
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record(stream)
                for t in batches:
                    plan.consume(t)
                t1.record(stream)
                plan.finish_raw()
                t1.synchronize()
                if step >= args.warmup:
                    times.append(t0.elapsed_time(t1))
        finally:
            plan.close()
        times.sort()
        return {"ms_median": round(times[len(times) // 2], 3), "ms_min": round(times[0], 3),
                "ms_max": round(times[-1], 3)}

    plans = {"min_length_email": [d.MinLength("email")],
             "min_length_all_three": [d.MinLength("id"), d.MinLength("amount"), d.MinLength("email")],
             "pattern_match_email": [d.PatternMatch("email", email)]}
    result["plans"] = {name: time_plan(a) for name, a in plans.items()}
    for key in ("validate", "evaluate_and_select"):
        for name in plans:
            result[key]["ratio_to_" + name] = round(result[key]["ms_median"] / result["plans"][name]["ms_median"], 3)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
