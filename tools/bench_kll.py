"""KLLSketch timing: one float64 column sketched on the GPU at the defaults (sketchSize 2048,
shrinkingFactor 0.64, the library's slab size), beside the host sketch on the same data.

    python tools/bench_kll.py [--rows 100000000] [--steps 5] [--warmup 1] [--host-rows N]

The column is generated in HBM (normal values, no NULLs).  One step = dq_kll_consume of the whole
column (the slab launch, the tree-merge rounds and the read-back of the one merged sketch; the call
is synchronous, so the step is timed on the host clock) and the export.  The host figure is
dq_diag_kll_sketch (deequ_amd/csrc/dq_kll.cpp, one thread, the same slab-and-tree layout) over the
same values copied to host memory -- over the first --host-rows of them and scaled to --rows when
that option is given.  Prints one JSON line: GPU ms per step (best and median), the host sketch's
single-thread ms, that divided by 16 (ideal scaling on a 16-CPU share), the column's HBM floor
(bytes / 8 TB/s), and whether the GPU state equals the host sketch's."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--host-rows", type=int, default=0, help="rows the host sketch is timed on (0 = all)")
    ap.add_argument("--slab-rows", type=int, default=0, help="0 = the library's constant")
    args = ap.parse_args()
    import torch
    import deequ_amd as d
    from deequ_amd import _lib as L
    from deequ_amd.kll import KLLSketcher
    from deequ_amd.states import DEFAULT_KLL_SLAB_ROWS, KLLState

    d.set_device(0)
    g = torch.Generator(device="cuda").manual_seed(11)
    values = torch.randn(args.rows, device="cuda", dtype=torch.float64, generator=g) * 1e3
    table = d.Table({"x": d.Column("float64", args.rows, values, None, None, 0, device=True)})
    k, c = d.KLLSketch.DEFAULT_SKETCH_SIZE, d.KLLSketch.DEFAULT_SHRINKING_FACTOR
    slab_rows = args.slab_rows or DEFAULT_KLL_SLAB_ROWS

    times, state = [], None
    for step in range(args.warmup + args.steps):
        sk = KLLSketcher(table.schema, [("x", k, c)], args.slab_rows or None)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sk.consume(table)
        state = sk.finish()[0]
        t1 = time.perf_counter()
        sk.close()
        if step >= args.warmup:
            times.append((t1 - t0) * 1e3)

    host_rows = min(args.rows, args.host_rows or args.rows)
    host = values[:host_rows].cpu().numpy()
    need = ctypes.c_int64()
    cap = 8 * (3 + 3 * 64 + 16384)
    buf = ctypes.create_string_buffer(cap)
    t0 = time.perf_counter()
    L.check(L.lib().dq_diag_kll_sketch(host.ctypes.data, None, host_rows, k, c, slab_rows, buf, cap, ctypes.byref(need)))
    host_ms = (time.perf_counter() - t0) * 1e3
    same = None
    if host_rows == args.rows:
        same = KLLState.from_export(buf.raw[:need.value], k, c) == state
    host_ms_scaled = host_ms * (args.rows / host_rows)
    print(json.dumps({
        "rows": args.rows, "sketchSize": k, "shrinkingFactor": c, "slab_rows": slab_rows,
        "gpu_ms_best": round(min(times), 3), "gpu_ms_median": round(statistics.median(times), 3),
        "host_rows": host_rows, "host_single_thread_ms": round(host_ms_scaled, 1),
        "host_div16_ms": round(host_ms_scaled / 16, 1),
        "hbm_floor_ms": round(args.rows * 8 / 8e12 * 1e3, 3),
        "levels": [len(cc.buffer) for cc in state.qSketch.compactors],
        "weight_conserved": state.qSketch.weight() == args.rows,
        "gpu_equals_host_sketch": same}))


if __name__ == "__main__":
    main()
