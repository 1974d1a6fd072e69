"""correlation_matrix on one MI355X next to what a caller did before it existed: one run_scan plan of
the same k (k + 1) / 2 Correlation analyzers (the pair kernel, unchanged code of this same commit)
over the same device-resident buffers.

    python tools/bench_corrmatrix.py [--rows 100000000] [--reps 5] [--pair-reps 2] [--only matrix|pairs]
                                     [--workloads f64_2,f64_8,...] [--hbm-tbs 6.29] [--mfma-per-s N]

Workloads (rows device-resident rows each): k = 2, 8, 16, 32, 64 float64 columns; k = 16 mixed
int64 / float64 columns with 5 % NULLs per column; k = 16 float64 with a `where` keeping half the
rows.  Per workload one JSON line: the whole matrix call (dq_corrmat_reset, _consume, _finish on one
handle; host clock around the synchronous calls; median, minimum and maximum over --reps after a
warm-up), the pair plan the same way (--pair-reps), their ratio, the algorithmic bytes (each selected
column, its validity and the filter's column read once) and fp64 MFMA instructions (rows / 4 per
16 x 16 tile product), and the two lower bounds they give against the measured ceilings --hbm-tbs
(TB/s of a streaming read) and --mfma-per-s (tools/ubench/mfma_f64_rate.hip): the larger one names
what bounds the workload.  The matrix kernel alone comes from a run of its own under the profiler:

    rocprofv3 --kernel-trace --stats -d OUT -- python tools/bench_corrmatrix.py --only matrix --reps 3

(dq_corrmat_kernel<false> is the fast form, <true> the masked one)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

WORKLOADS = ["f64_2", "f64_8", "f64_16", "f64_32", "f64_64", "mixed_16_nulls", "f64_16_where"]


def spread(ms):
    s = sorted(ms)
    return {"median": round(s[len(s) // 2], 3), "min": round(s[0], 3), "max": round(s[-1], 3)}


def build(torch, d, name, rows):
    """(Table, columns, where, algorithmic bytes, MFMAs) of one workload."""
    g = torch.Generator(device="cuda").manual_seed(len(name))
    kind, k = name.split("_")[0], int(name.split("_")[1])
    cols, nbytes = {}, 0
    masked = name.endswith("nulls") or name.endswith("where")
    for i in range(k):
        validity = None
        if name.endswith("nulls"):
            validity = torch.randint(0, 256, ((rows + 7) // 8 + 8,), device="cuda", generator=g, dtype=torch.uint8)
            validity |= torch.randint(0, 256, (validity.numel(),), device="cuda", generator=g, dtype=torch.uint8)
            validity |= torch.randint(0, 256, (validity.numel(),), device="cuda", generator=g, dtype=torch.uint8)
            validity |= torch.randint(0, 256, (validity.numel(),), device="cuda", generator=g, dtype=torch.uint8)  # ~6 % zeros
            nbytes += rows // 8
        if kind == "mixed" and i % 2:
            v = torch.randint(-1 << 20, 1 << 20, (rows,), device="cuda", generator=g, dtype=torch.int64)
            cols["c%d" % i] = d.Column("int64", rows, v, validity, device=True)
        else:
            v = torch.rand(rows, device="cuda", generator=g, dtype=torch.float64)
            if i:
                v += 0.25 * cols["c0"].values if cols["c0"].dtype == "float64" else 0.0
            cols["c%d" % i] = d.Column("float64", rows, v, validity, device=True)
        nbytes += rows * 8
    names, where = list(cols), None
    if name.endswith("where"):
        cols["g"] = d.Column("int64", rows, torch.randint(0, 2, (rows,), device="cuda", generator=g, dtype=torch.int64),
                             None, device=True)
        where = "g > 0"
        nbytes += rows * 8
    t = (k + 15) // 16
    tiles = t * (t + 1) // 2
    mfmas = (rows // 4) * (6 * tiles if masked else tiles + t)
    return d.Table(cols), names, where, nbytes, mfmas


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--pair-reps", type=int, default=2)
    ap.add_argument("--only", choices=["matrix", "pairs"], default=None)
    ap.add_argument("--workloads", default=",".join(WORKLOADS))
    ap.add_argument("--hbm-tbs", type=float, default=6.29)
    ap.add_argument("--mfma-per-s", type=float, default=0.0, help="chip-wide fp64 MFMA instructions per second (0: not given)")
    args = ap.parse_args()
    import torch
    import deequ_amd as d
    from deequ_amd.correlation import _Corrmat
    from deequ_amd.engine import schema_index
    from deequ_amd.predicates import compile_predicate
    from deequ_amd.table import dq_columns
    if not torch.cuda.is_available():
        raise SystemExit("bench_corrmatrix.py needs the GPU: there is no CPU path to time")
    d.set_device(0)
    for name in args.workloads.split(","):
        table, names, where, nbytes, mfmas = build(torch, d, name, args.rows)
        torch.cuda.synchronize()
        k = len(names)
        out = {"workload": name, "rows": args.rows, "k": k, "pairs": k * (k + 1) // 2, "algorithmic_bytes": nbytes,
               "mfma_instructions": mfmas, "hbm_bound_ms": round(nbytes / (args.hbm_tbs * 1e12) * 1e3, 3)}
        if args.mfma_per_s > 0:
            out["mfma_bound_ms"] = round(mfmas / args.mfma_per_s * 1e3, 3)
            out["bound_by"] = "mfma" if out["mfma_bound_ms"] > out["hbm_bound_ms"] else "hbm"
        if args.only != "pairs":
            program = compile_predicate(where, schema_index(table.schema)) if where else None
            run = _Corrmat(table.schema, names, program, 0)
            cols = dq_columns(table, list(table.schema.keys()))
            ms, fb = [], 0
            for i in range(args.reps + 1):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run.reset()
                run.consume(cols, args.rows)
                states, fb = run.finish()
                if i:
                    ms.append((time.perf_counter() - t0) * 1e3)
            run.close()
            med = sorted(ms)[len(ms) // 2]
            out.update(matrix_ms=spread(ms), fallback_pairs=fb, matrix_gb_per_s=round(nbytes / (med * 1e-3) / 1e9, 1),
                       matrix_mfma_per_s=float("%.4g" % (mfmas / (med * 1e-3))), n_first_pair=float(states[0][0]))
        if args.only != "matrix":
            analyzers = [d.Correlation(x, y, where) for i, x in enumerate(names) for y in names[i:]]
            ps = []
            for i in range(args.pair_reps + (1 if k <= 16 else 0)):  # (the large plans take seconds: no warm-up run)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                got = d.run_scan(analyzers, table)
                if i or k > 16:
                    ps.append((time.perf_counter() - t0) * 1e3)
            out.update(pair_plan_ms=spread(ps), pair_plan_bytes=2 * 8 * args.rows * len(analyzers))
            if "matrix_ms" in out:
                out["pair_plan_over_matrix"] = round(out["pair_plan_ms"]["median"] / out["matrix_ms"]["median"], 2)
                out["same_n"] = got[analyzers[0]] is None or got[analyzers[0]].n == out["n_first_pair"]
        print(json.dumps(out), flush=True)
        del table
        torch.cuda.empty_cache()
        d._lib.lib().dq_release_cached_memory(0)
    return 0


if __name__ == "__main__":
    sys.exit(main())
