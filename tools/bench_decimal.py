"""The decimal scan's timing on the GPU: the profiler's seven analyzers of one column
(Completeness, ApproxCountDistinct, Minimum, Maximum, Mean, StandardDeviation, Sum) over rows
resident in HBM, for three columns of the same length:

  (a) decimal(12,2): every row's cast takes the one-divide tier, the hash is hashLong;
  (b) decimal(38,10) holding values of about 30 digits: every row's cast takes the exact long
      division, the hash runs over BigInteger.toByteArray;
  (c) a float64 column holding (a)'s values: the existing 8-byte value scan, the yardstick.

    python tools/bench_decimal.py [--rows 100000000] [--steps 10] [--warmup 2]

One step = dq_plan_reset, dq_plan_consume of the column, dq_plan_finish (which waits for the
device), timed with a host clock around the three calls.  Prints one JSON line: per case the median
and best step in ms and the bytes per second over the bytes the scan must read (16 B of values for
a decimal row, 8 B for a float64 row, plus one validity bit); for (a) and (b) the share of the
16.125 B/row HBM roofline at the 6.3 TB/s a streaming read sustains on this card; and (a) against
(c) per byte."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

HBM_BYTES_PER_S = 6.3e12  # sustained streaming read (8 TB/s is the specification's peak)


def make_columns(torch, d, rows, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    valid = torch.rand(rows, device="cuda", generator=g) >= 0.05
    nbytes = (rows + 7) // 8
    pad = torch.zeros(nbytes * 8, device="cuda", dtype=torch.uint8)
    pad[:rows] = valid.to(torch.uint8)
    weights = torch.tensor([1, 2, 4, 8, 16, 32, 64, 128], device="cuda", dtype=torch.uint8)
    validity = (pad.reshape(-1, 8) * weights).sum(dim=1).to(torch.uint8)
    del pad
    # (a) unscaled values within +-(10^12 - 1): the low word, the high word its sign
    small = torch.randint(-(10 ** 12 - 1), 10 ** 12, (rows,), device="cuda", generator=g, dtype=torch.int64)
    a = torch.stack([small, small >> 63], dim=1).contiguous()
    # (b) non-negative values below 2^99 (about 6.3e29: 30 digits): a random low word, 35 high bits
    lo = torch.randint(-(2 ** 63), 2 ** 63 - 1, (rows,), device="cuda", generator=g, dtype=torch.int64)
    hi = torch.randint(2 ** 31, 2 ** 35, (rows,), device="cuda", generator=g, dtype=torch.int64)
    b = torch.stack([lo, hi], dim=1).contiguous()
    del lo, hi
    c = small.to(torch.float64) / 100.0
    return {
        "a_decimal(12,2)": (d.Column("decimal(12,2)", rows, a, validity, device=True), 16),
        "b_decimal(38,10)": (d.Column("decimal(38,10)", rows, b, validity, device=True), 16),
        "c_float64": (d.Column("float64", rows, c, validity, device=True), 8),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()

    import torch
    import deequ_amd as d
    from deequ_amd.engine import Plan, op_spec_for

    from deequ_amd import _lib
    if _lib.device_count() < 1:
        raise SystemExit("bench_decimal.py needs an MI355X: no gfx950 device is visible")
    d.set_device(0)
    columns = make_columns(torch, d, args.rows, seed=1)
    torch.cuda.synchronize()
    result = {"rows": args.rows, "steps": args.steps, "warmup": args.warmup, "cases": {}}
    for name, (col, width) in columns.items():
        table = d.Table({"x": col})
        analyzers = [d.Completeness("x"), d.ApproxCountDistinct("x"), d.Minimum("x"), d.Maximum("x"), d.Mean("x"),
                     d.StandardDeviation("x"), d.Sum("x")]
        plan = Plan([op_spec_for(a, table.schema) for a in analyzers], table.schema)
        times = []
        for step in range(args.warmup + args.steps):
            t0 = time.perf_counter()
            plan.reset()
            plan.consume(table)
            plan.finish()  # waits for the device; raises if an op was declined
            t1 = time.perf_counter()
            if step >= args.warmup:
                times.append((t1 - t0) * 1e3)
        plan.close()
        nbytes = args.rows * (width + 0.125)
        med = statistics.median(times)
        case = {"ms_median": med, "ms_best": min(times), "bytes": nbytes, "bytes_per_s": nbytes / (med * 1e-3)}
        if width == 16:
            case["hbm_roofline_share"] = (nbytes / HBM_BYTES_PER_S) / (med * 1e-3)
        result["cases"][name] = case
    ca, cb, cc = (result["cases"][k] for k in ("a_decimal(12,2)", "b_decimal(38,10)", "c_float64"))
    result["a_over_c_per_byte"] = (ca["ms_median"] / ca["bytes"]) / (cc["ms_median"] / cc["bytes"])
    result["b_over_a"] = cb["ms_median"] / ca["ms_median"]
    print(json.dumps(result))


if __name__ == "__main__":
    main()
