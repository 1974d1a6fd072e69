"""take ("give me the failing rows as a table") on one MI355X, per column and selection, next to
what a caller did before it existed:

    (a) fixed-width columns against torch.index_select on the same tensor (no validity, slices or
        -1 there: a ratio, not a gate)
    (b) string columns against copying the column to the host and pyarrow's take, copy included
        (the gate, in direction only: take must be faster)
    (c) --sweep: the string columns and a skewed column (one 1 MiB cell per 10^6 short ones) under
        the libraries of --libs (variant builds of the two byte-copy thresholds,
        tools/build_variant.sh take_w64 "-DDQ_TAKE_WAVE_BYTES=64"), one process per library

    python tools/bench_take.py [--rows 100000000] [--reps 20] [--host-reps 2] [--chunks 16]
    python tools/bench_take.py --sweep --libs default,LIB[,LIB...]    (LIB: a path build_variant.sh printed)

One device-resident table of `rows` rows in `chunks` batches (a utf8 batch holds at most 2 GiB):
int64, float64, bool, decimal(12,2), 12-digit strings, strings of 5 to 200 bytes.  Selections:
ascending 1 %, ascending 50 %, 10^6 random rows, and 10^6 random rows of which 10 % are -1 (what
reference_rows looks like).  Per column and selection: device events around the synchronous
layout + gather (after a warm-up, `reps` repetitions; the median, minimum and maximum in ms) and
the achieved rate over the algorithmic bytes -- the 8-byte index, the cells read and the cells
written (utf8: also 8 offset bytes read and 4 written per row).  A utf8 output above 2 GiB is
declined (DQ_ERR_SPACE) and reported as such.  (a) and (b) alternate with take in this process.
Prints one JSON line per measurement."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]


def spread(ms):
    s = sorted(ms)
    return {"median": round(s[len(s) // 2], 3), "min": round(s[0], 3), "max": round(s[-1], 3)}


def cuts(rows, chunks):
    return [rows * k // chunks for k in range(chunks + 1)]


def string_chunk(torch, d, n, lo, hi, seed):
    """n strings of lo..hi random bytes ('0'..'9' when lo == hi == 12)."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    if lo == hi:
        offsets = torch.arange(n + 1, device="cuda", dtype=torch.int32) * lo
        total = n * lo
    else:
        lens = torch.randint(lo, hi + 1, (n,), device="cuda", generator=g, dtype=torch.int32)
        offsets = torch.zeros(n + 1, device="cuda", dtype=torch.int32)
        offsets[1:] = torch.cumsum(lens, 0, dtype=torch.int64).to(torch.int32)
        total = int(offsets[-1])
    heap = torch.randint(48, 58, (total + 8,), device="cuda", generator=g, dtype=torch.uint8)
    return d.Column("string", n, heap, None, offsets=offsets, device=True)


def skewed_chunk(torch, d, n):
    """n one-byte cells but for one 1 MiB cell per 10^6 rows."""
    lens = torch.ones(n, device="cuda", dtype=torch.int64)
    lens[500_000::1_000_000] = 1 << 20
    offsets = torch.zeros(n + 1, device="cuda", dtype=torch.int32)
    offsets[1:] = torch.cumsum(lens, 0).to(torch.int32)
    heap = torch.randint(48, 58, (int(offsets[-1]) + 8,), device="cuda", dtype=torch.uint8)
    return d.Column("string", n, heap, None, offsets=offsets, device=True)


def selections(torch, rows):
    g = torch.Generator(device="cuda").manual_seed(9)
    few = min(rows, 1_000_000)
    asc1 = torch.arange(0, rows, 100, device="cuda", dtype=torch.int64)
    asc50 = torch.arange(0, rows, 2, device="cuda", dtype=torch.int64)
    rand = torch.randint(0, rows, (few,), device="cuda", generator=g, dtype=torch.int64)
    ref = rand.clone()
    ref[::10] = -1
    return {"ascending_1pct": asc1, "ascending_50pct": asc50, "random_1e6": rand, "reference_rows_10pct_null": ref}


def timed(torch, fn, reps, warmup=1):
    ms = []
    for i in range(warmup + reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        if i >= warmup:
            ms.append(a.elapsed_time(b))
        del out
    return ms


def take_column(torch, d, chunks, rows, reps):
    """(ms of layout + gather, output bytes, m) of one column, or ("space", message)."""
    from deequ_amd import _lib as L
    from deequ_amd.take import _Take
    dev = torch.device("cuda", 0)
    t = _Take(rows, [c.length for c in chunks], 0)
    try:
        try:
            col = t.column(chunks[0].dtype, chunks, dev)
        except L.DeequAmdError as e:
            if e.status != L.DQ_ERR_SPACE:
                raise
            return "space", str(e)
        nbytes = int(col.offsets[-1]) if col.offsets is not None else col.values.numel() * col.values.element_size()
        del col
        return timed(torch, lambda: t.column(chunks[0].dtype, chunks, dev), reps), nbytes, rows.numel()
    finally:
        t.close()


def host_arrow_take(torch, chunks, rows):
    """What a caller does today for a string column: every chunk to the host, pyarrow.take."""
    import numpy as np
    import pyarrow as pa
    arrs = []
    for c in chunks:
        offs, heap = c.offsets.cpu().numpy(), c.values.cpu().numpy()
        arrs.append(pa.Array.from_buffers(pa.string(), c.length, [None, pa.py_buffer(offs), pa.py_buffer(heap)]))
    idx = rows.cpu().numpy()
    mask = idx < 0
    col = pa.chunked_array(arrs)
    if sum(int(c.offsets[-1]) for c in chunks) > 0x7fffffff:  # (pyarrow's take concatenates: int32 offsets overflow)
        col = col.cast(pa.large_string())
    return col.take(pa.array(np.where(mask, 0, idx), mask=mask))


def run_main(args):
    import torch
    import deequ_amd as d
    if not torch.cuda.is_available():
        raise SystemExit("bench_take.py needs the GPU: there is no CPU path to time")
    d.set_device(0)
    rows, bounds = args.rows, cuts(args.rows, args.chunks)
    g = torch.Generator(device="cuda").manual_seed(1)
    whole = {
        "int64": torch.randint(-1 << 40, 1 << 40, (rows,), device="cuda", generator=g, dtype=torch.int64),
        "float64": torch.rand(rows, device="cuda", generator=g, dtype=torch.float64),
        "bool": torch.randint(0, 256, ((rows + 7) // 8 + 8,), device="cuda", generator=g, dtype=torch.uint8),
        "decimal(12,2)": torch.randint(0, 10 ** 12, (rows, 2), device="cuda", generator=g, dtype=torch.int64),
    }
    whole["decimal(12,2)"][:, 1] = 0
    columns = {}
    for name, t in whole.items():
        if name == "bool":  # (one bitmap, every batch a slice of it at its bit offset)
            columns[name] = [d.Column("bool", b - a, t, None, offset=a, device=True) for a, b in zip(bounds, bounds[1:])]
        else:
            columns[name] = [d.Column(name, b - a, t[a:b], None, device=True) for a, b in zip(bounds, bounds[1:])]
    columns["digits12"] = [string_chunk(torch, d, b - a, 12, 12, 100 + k) for k, (a, b) in enumerate(zip(bounds, bounds[1:]))]
    columns["bytes5to200"] = [string_chunk(torch, d, b - a, 5, 200, 200 + k) for k, (a, b) in enumerate(zip(bounds, bounds[1:]))]
    sels = selections(torch, rows)
    torch.cuda.synchronize()
    for sname, sel in sels.items():
        for cname, chunks in columns.items():
            out = {"column": cname, "selection": sname, "rows": rows, "m": sel.numel(), "chunks": args.chunks}
            res = take_column(torch, d, chunks, sel, args.reps)
            if res[0] == "space":
                out["declined"] = res[1]
                print(json.dumps(out), flush=True)
                continue
            ms, nbytes, m = res
            is_str = chunks[0].dtype == "string"
            algo = 8 * m + 2 * nbytes + (12 * m if is_str else 0)
            out.update(take_ms=spread(ms), output_bytes=nbytes, algorithmic_bytes=algo,
                       gb_per_s=round(algo / (sorted(ms)[len(ms) // 2] * 1e-3) / 1e9, 1))
            if cname in ("int64", "float64", "decimal(12,2)") and sname != "reference_rows_10pct_null":
                t = whole[cname]
                ts = timed(torch, lambda: torch.index_select(t, 0, sel), args.reps)
                ms2 = take_column(torch, d, chunks, sel, max(1, args.reps // 2))[0]  # (alternated: take once more)
                out.update(index_select_ms=spread(ts), take_again_ms=spread(ms2),
                           take_over_index_select=round(spread(ms)["median"] / spread(ts)["median"], 3))
            if is_str and sname in ("ascending_1pct", "random_1e6") and args.host_reps > 0:
                import time
                hs = []
                for _ in range(args.host_reps):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    got = host_arrow_take(torch, chunks, sel)
                    hs.append((time.perf_counter() - t0) * 1e3)
                    again = take_column(torch, d, chunks, sel, 1)  # (alternated)
                    hs_take = again[0]
                out.update(host_pyarrow_ms=spread(hs), take_between_ms=spread(hs_take),
                           pyarrow_over_take=round(spread(hs)["median"] / spread(ms)["median"], 1),
                           same_rows=len(got) == m)
            print(json.dumps(out), flush=True)
    return 0


def run_sweep_one(args):
    """The string columns and the skewed column under the library DEEQU_AMD_LIB names."""
    import torch
    import deequ_amd as d
    from deequ_amd import _lib as L
    d.set_device(0)
    rows = min(args.rows, 20_000_000)
    bounds = cuts(rows, 4)
    cols = {"bytes5to200": [string_chunk(torch, d, b - a, 5, 200, 200 + k) for k, (a, b) in enumerate(zip(bounds, bounds[1:]))],
            "skewed": [skewed_chunk(torch, d, b - a) for a, b in zip(bounds, bounds[1:])]}
    sel = torch.arange(0, rows, 4, device="cuda", dtype=torch.int64)
    out = {"lib": os.environ.get("DEEQU_AMD_LIB", "default"), "constants": L.diag_take_constants(), "rows": rows,
           "m": sel.numel()}
    for name, chunks in cols.items():
        ms, nbytes, _ = take_column(torch, d, chunks, sel, args.reps)
        out[name + "_ms"] = spread(ms)
        out[name + "_bytes"] = nbytes
    print(json.dumps(out), flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--chunks", type=int, default=16)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--libs", default="default")
    ap.add_argument("--passes", type=int, default=2, help="--sweep: times the list of libraries is gone through")
    ap.add_argument("--limit", type=int, default=300, help="--sweep: seconds allowed to one library's process")
    ap.add_argument("--sweep-one", action="store_true", help="(internal) one library in this process")
    args = ap.parse_args()
    if args.sweep_one:
        return run_sweep_one(args)
    if not args.sweep:
        return run_main(args)
    for _ in range(args.passes):  # (alternated: every library once per pass)
        for lib in args.libs.split(","):
            env = dict(os.environ)
            env.pop("DEEQU_AMD_LIB", None)
            if lib != "default":
                env["DEEQU_AMD_LIB"] = os.path.abspath(lib)
            cmd = [sys.executable, os.path.abspath(__file__), "--sweep-one", "--rows", str(args.rows), "--reps", str(args.reps)]
            try:
                p = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=args.limit, env=env)
            except subprocess.TimeoutExpired:
                print(json.dumps({"failed": lib, "reason": "time limit of %d s" % args.limit}), flush=True)
                return 1
            if p.returncode != 0:
                print(json.dumps({"failed": lib, "exit_status": p.returncode}), flush=True)
                return 1
            print(p.stdout.decode().strip().splitlines()[-1], flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
