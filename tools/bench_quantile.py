"""ApproxQuantile timing: the digest of one float64 column built on the GPU at relativeError 0.01 and
0.001, over four distributions of the same size.

    python tools/bench_quantile.py [--rows 100000000] [--steps 5] [--warmup 1]

The column is generated in HBM, no NULLs: uniform random; constant; two-valued; keys that differ
only in their lowest byte (every pass is needed and all rows stay in the active prefixes).  One step
= dq_aq_consume of the whole column (every pass of the radix select, the read-back of the keys at the
target ranks and the host merge; the call is synchronous, so the step is timed on the host clock)
and the export.  The bytes model is passes x 8 B per row over the 8 TB/s HBM peak bench.py uses,
with the most passes the relativeError can take (8 at 0.01, 14 at 0.001: the digit narrows with the
number of active prefixes, DESIGN.md §3 ApproxQuantile); a column with few distinct values needs
fewer (a constant one 5).  Prints one JSON line per relativeError: per distribution the best and
median ms, the time over the model's, and the ratio to uniform; and whether the median answer is
within ceil(relativeError * n) ranks (checked for the uniform column by counting on the GPU)."""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

HBM_PEAK_GBS = 8000.0  # as bench.py


def max_passes(eps):
    ranks = min(2048, int(math.floor(2.0 / eps)) + 2)
    narrow = 15 - max(0, math.ceil(math.log2(ranks)))
    return 1 + -(-(64 - 15) // narrow)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args()
    import torch
    import deequ_amd as d
    from deequ_amd.quantiles import QuantileSketcher

    d.set_device(0)
    n = args.rows
    g = torch.Generator(device="cuda").manual_seed(11)

    def make(kind):
        if kind == "uniform":
            return torch.rand(n, device="cuda", dtype=torch.float64, generator=g)
        if kind == "constant":
            return torch.full((n,), 42.5, device="cuda", dtype=torch.float64)
        if kind == "two_valued":
            pick = torch.rand(n, device="cuda", generator=g) < 0.3
            return torch.where(pick, torch.tensor(-1.5, device="cuda", dtype=torch.float64),
                               torch.tensor(7.25, device="cuda", dtype=torch.float64))
        low = torch.randint(0, 256, (n,), device="cuda", dtype=torch.int64, generator=g)
        return (low | 0x40590000DEADBE00).view(torch.float64)

    for eps in (0.01, 0.001):
        passes = max_passes(eps)
        model_ms = passes * 8.0 * n / (HBM_PEAK_GBS * 1e9) * 1e3
        out = {"rows": n, "relativeError": eps, "passes_max": passes, "model_ms": round(model_ms, 3), "kinds": {}}
        for kind in ("uniform", "constant", "two_valued", "low_byte"):
            values = make(kind)
            table = d.Table({"x": d.Column("float64", n, values, None, None, 0, device=True)})
            times, state = [], None
            for step in range(args.warmup + args.steps):
                sk = QuantileSketcher(table.schema, [("x", eps)])
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                sk.consume(table)
                state = sk.finish()[0]
                t1 = time.perf_counter()
                sk.close()
                if step >= args.warmup:
                    times.append((t1 - t0) * 1e3)
            dig = state.percentileDigest
            row = {"ms_best": round(min(times), 3), "ms_median": round(statistics.median(times), 3),
                   "over_model": round(statistics.median(times) / model_ms, 2), "entries": len(dig.sampled),
                   "count_ok": dig.count == n}
            if kind == "uniform":
                (median,) = dig.getPercentiles([0.5])
                rank = int((values <= median).sum().item())
                row["median_rank_error"] = abs(rank - math.ceil(0.5 * n))
                row["rank_bound"] = math.ceil(eps * n)
            out["kinds"][kind] = row
            del table, values
            torch.cuda.empty_cache()
        base = out["kinds"]["uniform"]["ms_median"]
        for kind, row in out["kinds"].items():
            row["vs_uniform"] = round(row["ms_median"] / base, 2)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
