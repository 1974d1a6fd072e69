"""Distance.categoricalDistance over two device states, next to what it replaces and to a yardstick:

    (a) FrequencyTable.linf_distance(a, b)      dq_freq_linf_distance: totals + two directed probe passes
    (b) dq_freq_merge of a and of b into an empty clone: what one read-and-probe pass over these
        tables costs elsewhere in the library (reported, not gated)
    (c) the host route: export_flat of both tables, then a numpy join of the two key sets and the
        same fp64 arithmetic -- what a caller had before the entry point existed

    python tools/bench_distance.py [--groups 1000000,10000000] [--kinds int64,digits12,str40]
                                   [--steps 10] [--warmup 2] [--limit 540]

Two tables of `groups` groups each with half their keys shared, counts 1..100, of int64 keys,
12-digit string keys (inline, hashed as a packed word) and 40-byte string keys (key heap).  Every
shape runs in a process of its own under --limit seconds; the first failure stops the script.  (a)
and (b) are host clocks around calls that end in a stream synchronise; (c) is a host clock.  The
host result must equal the device result bit for bit.  Prints one JSON line per shape, then one
summary line; the gate: at the largest --groups the device call is faster than the host route.
Exit status 1 if a shape fails or the gate does."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

KEY_BYTES = {"int64": 8, "digits12": 12, "str40": 40}
PREFIX = b"a-forty-byte-grouping-key-::"  # 28 bytes + 12 digits


def make_table(torch, FrequencyTable, kind, first, n, seed):
    """Groups with ids first .. first + n, built and imported on the device."""
    ids = torch.arange(first, first + n, device="cuda", dtype=torch.int64)
    g = torch.Generator(device="cuda").manual_seed(seed)
    counts = torch.randint(1, 101, (n,), device="cuda", generator=g, dtype=torch.int64)
    w = KEY_BYTES[kind]
    if kind == "int64":
        blob = (ids * 1_000_003).view(torch.uint8)
        dtype = "int64"
    else:
        pow10 = torch.tensor([10 ** (11 - j) for j in range(12)], device="cuda", dtype=torch.int64)
        digits = ((ids[:, None] * 7 // pow10[None, :]) % 10 + 48).to(torch.uint8)
        if kind == "str40":
            pre = torch.tensor(list(PREFIX), device="cuda", dtype=torch.uint8)[None, :].expand(n, len(PREFIX))
            digits = torch.cat([pre, digits], dim=1)
        blob = digits.contiguous().view(-1)
        dtype = "string"
    offs = torch.arange(n + 1, device="cuda", dtype=torch.int64) * w
    t = FrequencyTable(["k"], {"k": dtype})
    t.import_flat(counts, offs, blob, int(counts.sum()))
    return t


def host_route(a, b, w):
    """export_flat of both tables + a numpy join: (linf_simple, ms export, ms join)."""
    import numpy as np
    t0 = time.perf_counter()
    ca, _, ba = a.export_flat()
    cb, _, bb = b.export_flat()
    t1 = time.perf_counter()
    key = np.dtype("<i8") if w == 8 else np.dtype("S%d" % w)
    keys = np.concatenate([np.ascontiguousarray(ba).view(key), np.ascontiguousarray(bb).view(key)])
    _, inv = np.unique(keys, return_inverse=True)
    inv = inv.reshape(-1)
    width = int(inv.max()) + 1
    fa = np.bincount(inv[:len(ca)], weights=ca.astype(np.float64), minlength=width)
    fb = np.bincount(inv[len(ca):], weights=cb.astype(np.float64), minlength=width)
    n, m = float(ca.sum()), float(cb.sum())
    linf = float(np.max(np.abs(fa / n - fb / m)))
    t2 = time.perf_counter()
    return linf, (t1 - t0) * 1e3, (t2 - t1) * 1e3


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def run_one(kind, n, steps, warmup):
    import torch
    import deequ_amd as d
    from deequ_amd.frequencies import FrequencyTable
    if not torch.cuda.is_available():
        raise SystemExit("bench_distance.py needs the GPU: there is no CPU path to time")
    d.set_device(0)
    a = make_table(torch, FrequencyTable, kind, 0, n, 1)
    b = make_table(torch, FrequencyTable, kind, n // 2, n, 2)
    torch.cuda.synchronize()
    dist = []
    for step in range(warmup + steps):
        t0 = time.perf_counter()
        r = a.linf_distance(b)
        t1 = time.perf_counter()
        if step >= warmup:
            dist.append((t1 - t0) * 1e3)
    assert (r.groups_a, r.groups_b, r.groups_common) == (n, n, n - n // 2), (r.groups_a, r.groups_b, r.groups_common)
    merge = []
    for step in range(1 + max(1, steps // 3)):
        c = FrequencyTable.like(a)
        c.summary()  # (the clone exists and is idle before the clock starts)
        t0 = time.perf_counter()
        c.merge_from(a)
        c.merge_from(b)
        t1 = time.perf_counter()
        c.close()
        if step >= 1:
            merge.append((t1 - t0) * 1e3)
    host = []
    for step in range(3 if n <= 2_000_000 else 1):
        linf, ms_export, ms_join = host_route(a, b, KEY_BYTES[kind])
        assert linf == r.linf_simple, (linf, r.linf_simple)
        host.append((ms_export + ms_join, ms_export, ms_join))
    host.sort()
    slots_a, slots_b = a.paths()["slots"], b.paths()["slots"]
    # 32-byte slots read: the totals and one directed pass stream each image once, and every group
    # probes at least one slot of the other table (long keys add their heap bytes, not counted)
    slot_bytes = 32 * (2 * slots_a + 2 * slots_b + r.groups_a + r.groups_b)
    ms = median(dist)
    h = host[len(host) // 2]
    return {"kind": kind, "groups": n, "key_bytes": KEY_BYTES[kind], "slots": [slots_a, slots_b],
            "linf_simple": r.linf_simple, "groups_common": r.groups_common,
            "distance_ms": round(ms, 3), "distance_ms_min": round(min(dist), 3), "distance_ms_max": round(max(dist), 3),
            "merge_pair_ms": round(median(merge), 3), "host_route_ms": round(h[0], 1), "host_export_ms": round(h[1], 1),
            "host_join_ms": round(h[2], 1), "host_over_device": round(h[0] / ms, 1),
            "slot_bytes": slot_bytes, "effective_GBps": round(slot_bytes / (ms * 1e-3) / 1e9, 1),
            "steps": steps, "warmup": warmup}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", default="1000000,10000000")
    ap.add_argument("--kinds", default="int64,digits12,str40")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--limit", type=int, default=540, help="seconds allowed to one shape's process")
    ap.add_argument("--one", nargs=2, metavar=("KIND", "GROUPS"), help="(internal) run one shape in this process")
    args = ap.parse_args()
    if args.one:
        print(json.dumps(run_one(args.one[0], int(args.one[1]), args.steps, args.warmup)), flush=True)
        return 0
    sizes = [int(x) for x in args.groups.split(",")]
    kinds = args.kinds.split(",")
    for k in kinds:
        if k not in KEY_BYTES:
            raise SystemExit("unknown kind %r (of %s)" % (k, ", ".join(KEY_BYTES)))
    results = []
    for n in sizes:
        for kind in kinds:
            cmd = [sys.executable, os.path.abspath(__file__), "--one", kind, str(n), "--steps", str(args.steps),
                   "--warmup", str(args.warmup)]
            try:
                p = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=args.limit)
            except subprocess.TimeoutExpired:
                print(json.dumps({"failed": [kind, n], "reason": "time limit of %d s" % args.limit}), flush=True)
                return 1
            if p.returncode != 0:
                print(json.dumps({"failed": [kind, n], "exit_status": p.returncode}), flush=True)
                return 1
            line = p.stdout.decode().strip().splitlines()[-1]
            print(line, flush=True)
            results.append(json.loads(line))
    top = max(sizes)
    gated = [r for r in results if r["groups"] == top]
    ok = all(r["distance_ms"] < r["host_route_ms"] for r in gated)
    print(json.dumps({"gate": "device call faster than the host route at %d groups" % top, "pass": ok,
                      "host_over_device": {r["kind"]: r["host_over_device"] for r in gated}}), flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
