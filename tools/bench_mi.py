"""MutualInformation over a joint frequency table resident in HBM, next to the route it replaces:

    (a) FrequencyTable.mutual_information()   dq_freq_mutual_information: totals, the projection into
        two marginal tables, the exact sum
    (b) the host route of the analyzer before the entry point existed (--host-groups, default 10^6):
        FrequencyTable.export() and MutualInformation.computeMetricFrom's Python loop

    python tools/bench_mi.py [--groups 10000000] [--host-groups 1000000] [--shapes int64,contention,strings]
                             [--steps 5] [--warmup 1] [--limit 540]

Three shapes of `groups` joint groups, counts 1..100:
    int64       (int64, int64), both columns high-cardinality (groups and groups * 2 / 5 values)
    contention  (int64 id, 5 category strings): every group adds to one of 5 marginal slots
    strings     (12-digit string, 40-byte string): heap joint keys, a heap marginal (groups / 10 values)
Every shape runs in a process of its own under --limit seconds; the first failure stops the script.
The clocks are host clocks around calls that end in a stream synchronise.  slot_bytes counts the
32-byte slots the call streams: the joint image three times (totals, projection, sum) and the two
marginal images once (their clearing; probes and heap bytes are not counted).  Prints one JSON line
per shape and size; exit status 1 if a shape fails."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

SHAPES = {"int64": ("int64", "int64"), "contention": ("int64", "string"), "strings": ("string", "string")}
CATEGORY = b"cat-"  # + one digit: 5 categories
PREFIX = b"a-forty-byte-grouping-key-::"  # 28 bytes + 12 digits


def u32(torch, n, value):
    return torch.tensor(list(int(value).to_bytes(4, "little")), device="cuda", dtype=torch.uint8)[None, :].expand(n, 4)


def digits12(torch, v):
    pow10 = torch.tensor([10 ** (11 - j) for j in range(12)], device="cuda", dtype=torch.int64)
    return ((v[:, None] // pow10[None, :]) % 10 + 48).to(torch.uint8)


def make_table(torch, FrequencyTable, shape, n):
    """n joint groups, encoded and imported on the device: (table, marginal sizes)."""
    ids = torch.arange(n, device="cuda", dtype=torch.int64)
    g = torch.Generator(device="cuda").manual_seed(1)
    counts = torch.randint(1, 101, (n,), device="cuda", generator=g, dtype=torch.int64)
    if shape == "int64":
        nb = max(1, n * 2 // 5)
        rows = torch.stack([ids * 1_000_003, ids % nb], dim=1).contiguous().view(torch.uint8).view(n, 16)
        sizes = (n, nb)
    elif shape == "contention":
        cat = torch.tensor(list(CATEGORY), device="cuda", dtype=torch.uint8)[None, :].expand(n, len(CATEGORY))
        rows = torch.cat([(ids * 1_000_003).view(torch.uint8).view(n, 8), u32(torch, n, 5), cat,
                          (ids % 5 + 48).to(torch.uint8)[:, None]], dim=1)
        sizes = (n, 5)
    else:
        nb = max(1, n // 10)
        pre = torch.tensor(list(PREFIX), device="cuda", dtype=torch.uint8)[None, :].expand(n, len(PREFIX))
        rows = torch.cat([u32(torch, n, 12), digits12(torch, ids * 7 + 100_000_000_000), u32(torch, n, 40), pre,
                          digits12(torch, (ids % nb) * 13)], dim=1)
        sizes = (n, nb)
    width = rows.shape[1]
    offs = torch.arange(n + 1, device="cuda", dtype=torch.int64) * width
    t = FrequencyTable(["a", "b"], dict(zip(("a", "b"), SHAPES[shape])))
    t.import_flat(counts, offs, rows.contiguous().view(-1), int(counts.sum()) + 1000)
    return t, sizes, width


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def run_one(shape, n, steps, warmup, host):
    import torch
    import deequ_amd as d
    from deequ_amd import analyzers
    from deequ_amd.frequencies import FrequenciesAndNumRows, FrequencyTable
    if not torch.cuda.is_available():
        raise SystemExit("bench_mi.py needs the GPU: there is no CPU path to time")
    d.set_device(0)
    t, sizes, width = make_table(torch, FrequencyTable, shape, n)
    t.summary()
    torch.cuda.synchronize()
    ms = []
    for step in range(warmup + steps):
        t0 = time.perf_counter()
        r = t.mutual_information()
        t1 = time.perf_counter()
        if step >= warmup:
            ms.append((t1 - t0) * 1e3)
    assert (r.groups, r.groups_a, r.groups_b) == (n, sizes[0], sizes[1]), (r.groups, r.groups_a, r.groups_b)
    slots = t.paths()["slots"]
    m_slots = 2048
    while m_slots < 2 * n:
        m_slots *= 2
    slot_bytes = 32 * (3 * slots + 2 * m_slots)
    out = {"shape": shape, "groups": n, "key_bytes": width, "slots": slots, "marginal_slots": m_slots, "mi": r.mi,
           "groups_a": r.groups_a, "groups_b": r.groups_b, "mi_ms": round(median(ms), 3), "mi_ms_min": round(min(ms), 3),
           "mi_ms_max": round(max(ms), 3), "slot_bytes": slot_bytes,
           "effective_GBps": round(slot_bytes / (median(ms) * 1e-3) / 1e9, 1), "steps": steps, "warmup": warmup}
    if host:  # the route of the analyzer before: export + the Python loop (once: it takes seconds)
        state = FrequenciesAndNumRows(t)
        t0 = time.perf_counter()
        t.export()
        t1 = time.perf_counter()
        bound, analyzers.MI_HOST_MAX_GROUPS = analyzers.MI_HOST_MAX_GROUPS, 1 << 62
        try:
            value = d.MutualInformation("a", "b").computeMetricFrom(state).value.get()
        finally:
            analyzers.MI_HOST_MAX_GROUPS = bound
        t2 = time.perf_counter()
        out.update({"host_export_ms": round((t1 - t0) * 1e3, 1), "host_route_ms": round((t2 - t1) * 1e3, 1),
                    "host_mi": value, "host_minus_device": value - r.mi,
                    "host_over_device": round((t2 - t1) * 1e3 / median(ms), 1)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=10_000_000)
    ap.add_argument("--host-groups", type=int, default=1_000_000, help="size of the host-route comparison (0: none)")
    ap.add_argument("--shapes", default="int64,contention,strings")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--limit", type=int, default=540, help="seconds allowed to one shape's process")
    ap.add_argument("--one", nargs=3, metavar=("SHAPE", "GROUPS", "HOST"), help="(internal) run one shape in this process")
    args = ap.parse_args()
    if args.one:
        print(json.dumps(run_one(args.one[0], int(args.one[1]), args.steps, args.warmup, args.one[2] == "1")), flush=True)
        return 0
    shapes = args.shapes.split(",")
    for s in shapes:
        if s not in SHAPES:
            raise SystemExit("unknown shape %r (of %s)" % (s, ", ".join(SHAPES)))
    runs = [(s, args.groups, "0") for s in shapes] + ([(s, args.host_groups, "1") for s in shapes] if args.host_groups else [])
    for shape, n, host in runs:
        cmd = [sys.executable, os.path.abspath(__file__), "--one", shape, str(n), host, "--steps", str(args.steps),
               "--warmup", str(args.warmup)]
        try:
            p = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=args.limit)
        except subprocess.TimeoutExpired:
            print(json.dumps({"failed": [shape, n], "reason": "time limit of %d s" % args.limit}), flush=True)
            return 1
        if p.returncode != 0:
            print(json.dumps({"failed": [shape, n], "exit_status": p.returncode}), flush=True)
            return 1
        print(p.stdout.decode().strip().splitlines()[-1], flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
