"""The frequency table as a state machine: generated walks (tests/freq_sequences.py) replayed on a
FrequencyTable and on the dict model in lock step.

After every step -- observers included -- the table's export equals the model's dict (every key,
every count, no key twice), summary() gives the model's num_rows / num_groups / num_unique /
grouped_rows exactly and its entropy within 1e-12 relative (test_gpu_frequencies.TOL), and no wait
timed out.  Every observer runs twice with equal results, top / lookup / count_histogram are exact,
linf_distance is held to test_gpu_distance's bar (bit-equal to the restatement) and
mutual_information to test_gpu_mutual_information's (8 ulps of the terms' absolute sum + groups x
2^-96).  Every walk runs under every configuration of CONFIGS; they all compare against the same
model, so they all export the same dict (and the test says so when two differ).

The reach test then asserts that the walks went where they were meant to: the counters of
FrequencyTable.paths(), rollbacks and format changes included, and each template's transition as a
change between two paths() readings of one table.  The record-format counters (packed_runs,
hashed_runs, uuid_runs, raw16_runs, compacted) count aggregations that ran slice by slice on the
partition path, which needs 2^9 slices; tables of these sizes have 2^5, so those counters come from
the DQ_FREQ_PART_MIN=1 configuration with DQ_FREQ_PART_SLOTS=1048576, and the early aggregation is
seen (as a second partition run within one step) with DQ_FREQ_STAGE_BUDGET=700 on top of it.

The replays of one session share the walk being replayed (built once for its 16 configurations: the
parametrisation is seed-major) and leave their paths() readings for the reach test, which replays
what it does not find when it is run alone.  Every configuration is compared with the same model, so
a selection or another order of the cases takes nothing from any case; the cross-configuration
comparison of the final exports is an extra over that, and covers the cases of one session.  A case
takes 0.1 to 0.9 s on an MI355X (the 625 of them 150 s)."""
import hashlib
import math
import random

import numpy as np
import pytest

import deequ_amd as d
import freq_sequences as F
from deequ_amd.frequencies import FrequencyTable, encode_key
from distance_restated import same

pytestmark = pytest.mark.gpu
TOL = 1e-12  # entropy: the bar of test_gpu_frequencies.py

_PART = {"DQ_FREQ_PART_MIN": "1", "DQ_FREQ_PATH": "sorted"}
_SLOTS = dict(_PART, DQ_FREQ_PART_SLOTS="1048576")
CONFIGS = {
    "default": {},
    "part": _PART,
    "slots": _SLOTS,
    "atomic": {"DQ_FREQ_PATH": "atomic"},
    "budget": {"DQ_FREQ_STAGE_BUDGET": "700"},
    "subbatch": {"DQ_FREQ_SUBBATCH_ROWS": "64"},
    "pack0": {"DQ_FREQ_PACK": "0"},
    "hashed0": {"DQ_FREQ_HASHED": "0"},
    "uuid0": {"DQ_FREQ_UUID": "0"},
    "small0": {"DQ_FREQ_SMALL": "0"},
    "compact0": {"DQ_FREQ_COMPACT": "0"},
    # the same knobs where they change something at these sizes: on the region staging
    "slots_budget": dict(_SLOTS, DQ_FREQ_STAGE_BUDGET="700"),
    "part_pack0": dict(_PART, DQ_FREQ_PACK="0"),
    "part_hashed0": dict(_PART, DQ_FREQ_HASHED="0"),
    "part_uuid0": dict(_PART, DQ_FREQ_UUID="0"),
    "slots_compact0": dict(_SLOTS, DQ_FREQ_COMPACT="0"),
}
_KNOBS = sorted({k for env in CONFIGS.values() for k in env})
FORMAT_COUNTERS = ("packed_runs", "hashed_runs", "uuid_runs", "raw16_runs")
REACH_COUNTERS = ("partition_runs", "sort_records", "packed_runs", "small_runs", "hashed_runs", "hashed_inserts",
                  "uuid_runs", "raw16_runs", "compacted", "import_coarse_runs", "import_skipped_runs", "rollbacks",
                  "materialized_for_format")

# what the replays leave for the reach test: per configuration and seed, the main table's paths()
# reading after every step, the largest reading of every counter over all tables, the second
# tables' format signatures, and the final export
_RUNS = {}
_TRIED = set()  # (configuration, seed) of every replay begun: one that is not in _RUNS failed
_WALK = {}  # the one walk being replayed: {"seed", "scenario", "built": {id(batch): host batch}, "groups": {...}}


def _walk(seed):
    if _WALK.get("seed") != seed:
        _WALK.clear()
        _WALK.update(seed=seed, scenario=F.scenario(seed), built={}, groups={})
    return _WALK


def _groups_of(config, batch):
    """group_batch, once per batch of the walk (the model's side is shared by every configuration)."""
    cache = _walk(_WALK["seed"])["groups"]
    if id(batch) not in cache:
        cache[id(batch)] = F.group_batch(config, batch)
    return cache[id(batch)]


def _host_batch(config, batch):
    built = _WALK["built"]
    if id(batch) in built:
        return built[id(batch)]
    schema = config["schema"]
    if batch["source"] == "arrow":
        import pyarrow as pa
        pa_type = {"int64": pa.int64(), "int32": pa.int32(), "float64": pa.float64(), "string": pa.string(),
                   "bool": pa.bool_()}
        lead = batch["lead"]
        full = pa.record_batch({c: pa.array(([v[0]] * lead if v else []) + list(v), pa_type[schema[c]])
                                for c, v in batch["columns"].items()})
        out = full.slice(lead if F.batch_rows(batch) else 0)  # rows [lead, ...) of a longer array: a non-zero offset
    else:
        out = d.Table.from_pydict({c: (schema[c], v) for c, v in batch["columns"].items()})
    built[id(batch)] = out
    return out


def _feed(table, config, batch):
    host = _host_batch(config, batch)
    if batch["source"] == "arrow":
        table.consume(d.ArrowBatch(host))
    elif batch["source"] == "device":
        table.consume(host.to_device(0))
    else:
        table.consume(host)


def _new_table(config):
    return FrequencyTable(config["keys"], config["schema"], histogram=config["histogram"], where=config["where"])


def _export(t):
    counts, keys = t.export()
    out = dict(zip(keys, counts.tolist()))
    assert len(out) == len(keys), "a key was exported twice"
    return out


def _flat_dict(counts, offs, blob):
    counts, offs, raw = np.asarray(counts).tolist(), np.asarray(offs).tolist(), np.asarray(blob).tobytes()
    keys = [raw[offs[i]:offs[i + 1]] for i in range(len(counts))]
    assert len(set(keys)) == len(keys)
    return dict(zip(keys, counts))


def _arrow_dict(t, config):
    tbl = t.to_arrow(strings=False)
    dtypes = [config["schema"][c] for c in config["keys"]]
    cols = [tbl.column(i).to_pylist() for i in range(len(dtypes))]
    counts = tbl.column(len(dtypes)).to_pylist()
    out = {encode_key(list(vals), dtypes, config["histogram"]): c for vals, c in zip(zip(*cols), counts)}
    assert len(out) == len(counts)
    return out


def _summary(t):
    s = t.summary()
    return (s.num_rows, s.num_groups, s.num_unique, s.grouped_rows), s.entropy


def _check_state(t, m, where):
    """The table against the model: paths (first: it reads a compacted table as it stands), summary,
    export."""
    p = t.paths()
    assert p["wait_timeouts"] == 0, (where, p)
    rows, groups, unique, grouped, entropy = m.summary()
    got, got_entropy = _summary(t)
    assert got == (rows, groups, unique, grouped), (where, got, (rows, groups, unique, grouped))
    if entropy is not None:
        print("entropy %s: %.17g against %.17g" % (where, got_entropy, entropy))
        assert F.rel_err(got_entropy, entropy) <= TOL, (where, got_entropy, entropy)
    got = _export(t)
    want = m.export()
    if got != want:
        missing = [k for k in want if k not in got][:3]
        extra = [k for k in got if k not in want][:3]
        wrong = [(k, got[k], want[k]) for k in got if k in want and got[k] != want[k]][:3]
        raise AssertionError("%s: export differs from the model: %d groups against %d; missing %r, extra %r, "
                             "other counts %r" % (where, len(got), len(want), missing, extra, wrong))
    return p


def _observe(t, m, config, step, rng):
    what = step["what"]
    if what == "summary":
        a, b = _summary(t), _summary(t)
        assert a[0] == b[0] == m.summary()[:4] and (a[1] == b[1] or (a[1] != a[1] and b[1] != b[1]))
    elif what == "export":
        assert _export(t) == _export(t) == m.export()
    elif what == "export_flat":
        host = _flat_dict(*t.export_flat())
        dev = _flat_dict(*[x.cpu().numpy() for x in t.export_flat(device=True)])
        assert host == dev == m.export()
    elif what == "to_arrow":
        assert _arrow_dict(t, config) == _arrow_dict(t, config) == m.export()
    elif what == "top":
        got = [list(zip(c.tolist(), k)) for c, k in (t.top(step["n"]), t.top(step["n"]))]
        assert got[0] == got[1] == m.top(step["n"]), (step, got[0][:8], m.top(step["n"])[:8])
    elif what == "lookup":
        for key in m.lookup_keys(rng):
            assert t.lookup(key) == t.lookup(key) == m.lookup(key), key
    elif what == "count_histogram":
        want_hist, want_big = m.count_histogram(step["n_bins"])
        for _ in range(2):
            hist, big = t.count_histogram(step["n_bins"])
            assert hist.tolist() == want_hist and big.tolist() == want_big
    elif what == "paths":
        assert t.paths() == t.paths()
    else:
        raise ValueError(what)


def _second_table(config, steps, run):
    """A second table and its model, built by their own sub-sequence of consume steps."""
    o, om = _new_table(config), F.Model(config)
    for s in steps:
        for b in s["batches"]:
            _feed(o, config, b)
            om.add(*_groups_of(config, b))
    p = _check_state(o, om, "second table")
    _note(run, p)
    run["second_formats"].append(tuple(p[k] > 0 for k in FORMAT_COUNTERS))
    return o, om


def _note(run, paths):
    for k in REACH_COUNTERS:
        run["max"][k] = max(run["max"].get(k, 0), paths[k])


def _partition(t, m, step, config, run):
    import torch
    n_parts = step["parts"]
    pp, pg, pk = t.partition_sizes(n_parts)
    nb = sum(t.part_bytes(p, g) for p, g in zip(pp, pg))
    buf = torch.empty(max(16, nb), dtype=torch.uint8, device="cuda")
    keys = torch.empty(max(8, sum(pk)), dtype=torch.uint8, device="cuda")
    assert t.partition_into(n_parts, buf, keys) == (pp, pg, pk)
    assert sum(pp) + sum(pg) == len(m.groups)
    union = {}
    for p in range(n_parts):  # every part into its own owner table: disjoint, the union is the source
        off = sum(16 * a + 32 * b for a, b in zip(pp[:p], pg[:p]))
        koff = sum(pk[:p])
        o = FrequencyTable.like(t)
        o.import_parts(buf[off:off + 16 * pp[p] + 32 * pg[p]], [pp[p]], [pg[p]], keys[koff:koff + max(1, pk[p])], [pk[p]])
        got = _export(o)
        assert len(got) == pp[p] + pg[p] and not (set(got) & set(union))
        union.update(got)
        _note(run, o.paths())
        o.close()
    assert union == m.export()
    # every part at once into one table: an empty one, or one that already holds other groups
    o, om = FrequencyTable.like(t), F.Model(config)
    if step["preload"] is not None:
        groups, rows = _groups_of(config, step["preload"])
        o.import_groups(list(groups.values()), list(groups.keys()), rows)
        om.add(groups, rows)
        _check_state(o, om, "preloaded receiver")
    o.import_parts(buf, pp, pg, keys, pk, num_rows=m.num_rows)
    om.add(m.groups, m.num_rows)
    _note(run, _check_state(o, om, "receiver of %d parts" % n_parts))
    o.close()


def _replay(seed, name):
    """One walk on a fresh table and on the model; returns the run's record (also kept in _RUNS)."""
    _TRIED.add((name, seed))
    sc = _walk(seed)["scenario"]
    config = sc["config"]
    run = {"seed": seed, "template": sc["template"], "readings": [], "max": {}, "second_formats": [],
           "steps": [{"op": s["op"]} for s in sc["steps"]]}
    t, m = _new_table(config), F.Model(config)
    run["readings"].append(t.paths())
    for i, step in enumerate(sc["steps"]):
        op = step["op"]
        where = "seed %d (%s, %s) step %d %s" % (seed, sc["template"], name, i, op)
        if op == "consume":
            for b in step["batches"]:
                _feed(t, config, b)
                m.add(*_groups_of(config, b))
        elif op == "observe":
            _observe(t, m, config, step, random.Random(seed * 1000 + i))
        elif op == "merge":
            o, om = _second_table(config, step["steps"], run)
            t.merge_from(o)
            m.add(om.groups, om.num_rows)
            assert _export(o) == om.export()  # (the source is as it was)
            o.close()
        elif op == "distance":
            o, om = _second_table(config, step["steps"], run)
            want = m.distance(om)
            for _ in range(2):
                r = t.linf_distance(o)
                assert (r.n, r.m, r.groups_a, r.groups_b, r.groups_common) == want[1:], (where, want)
                assert same(r.linf_simple, want[0]), (where, r.linf_simple, want[0])
            assert _export(o) == om.export()
            o.close()
        elif op == "mi":
            want = m.mutual_information()
            got = [t.mutual_information() for _ in range(2)]
            for r in got:
                assert (r.num_rows, r.groups, r.groups_a, r.groups_b) == (m.num_rows, len(m.groups), want.groups_a,
                                                                         want.groups_b), where
                if math.isnan(want.fsum):
                    assert math.isnan(r.mi)
                else:
                    bound = 8 * 2.0 ** -52 * want.sum_abs + len(m.groups) * 2.0 ** -96
                    print("mi %s: %.17g against %.17g, bound %.3g" % (where, r.mi, want.fsum, bound))
                    assert abs(r.mi - want.fsum) <= bound, (where, r.mi, want.fsum, bound)
            assert same(got[0].mi, got[1].mi)
        elif op == "import":
            groups, rows = _groups_of(config, step["batch"])
            counts, keys = list(groups.values()), list(groups.keys())
            if step["flat"]:
                offs = np.zeros(len(keys) + 1, dtype=np.int64)
                np.cumsum([len(k) for k in keys], out=offs[1:])
                t.import_flat(np.asarray(counts, dtype=np.int64), offs, np.frombuffer(b"".join(keys), dtype=np.uint8), rows)
            else:
                t.import_groups(counts, keys, rows)
            m.add(groups, rows)
        elif op == "partition":
            _partition(t, m, step, config, run)
        elif op == "reserve":
            t.reserve(step["rows"])
        elif op == "expect_groups":
            t.expect_groups(step["groups"])
        elif op == "reset":
            t.reset()
            m.reset()
            assert t.num_rows == 0 and _export(t) == {}
        else:
            raise ValueError(op)
        p = _check_state(t, m, where)
        run["readings"].append(p)
        _note(run, p)
    run["final_table"] = hashlib.sha256(repr(sorted(_export(t).items())).encode()).hexdigest()
    t.close()
    _RUNS[(name, seed)] = run
    return run


def _set_env(monkeypatch, name):
    for k in _KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in CONFIGS[name].items():
        monkeypatch.setenv(k, v)


# seed-major: the walk and the model's grouping of its batches are built once for all configurations
@pytest.mark.parametrize("seed,name", [(s, n) for s in F.SEEDS for n in CONFIGS],
                         ids=["%d-%s" % (s, n) for s in F.SEEDS for n in CONFIGS])
def test_walk_matches_model(gpu, monkeypatch, seed, name):
    _set_env(monkeypatch, name)
    run = _replay(seed, name)
    for (other, s), r in _RUNS.items():  # every configuration exports the identical dict
        if s == seed:
            assert r["final_table"] == run["final_table"], (other, name)


# ---------------------------------------------------------------- reach
def _runs_of(monkeypatch, name):
    out = {}
    for seed in F.SEEDS:
        if (name, seed) not in _TRIED:  # (this test run alone: replay what is missing)
            _set_env(monkeypatch, name)
            _replay(seed, name)
        assert (name, seed) in _RUNS, "the walk of seed %d failed under %s: see its own test" % (seed, name)
        out[seed] = _RUNS[(name, seed)]
    return out


def _deltas(run):
    """Per step: (step, reading before, reading after, {counter: increase})."""
    r = run["readings"]
    return [(s, a, b, {k: b[k] - a[k] for k in REACH_COUNTERS}) for s, a, b in zip(run["steps"], r, r[1:])]


def _seen(run, cond):
    return any(cond(s, a, b, dl) for s, a, b, dl in _deltas(run))


def _pad8(key):
    return (len(key.encode()) + 7) & ~7


def _main_batches(seed):
    """Per step of the walk: the batches the main table consumes."""
    return [s["batches"] if s["op"] == "consume" else [] for s in _walk(seed)["scenario"]["steps"]]


def _tiny_rollbacks(seed):
    """The rollbacks a walk of a single string key owes to small batches alone.  The string staging
    kernels read keys 16 bytes at a time and hand a batch whose key column holds fewer than 16 bytes
    (Arrow: up to its last row, the rows sliced off the front included) to the general path, by a
    rollback -- as long as the table stages packed or 16-byte records, that is: no batch since the
    last reset held a key over 15 bytes."""
    out, long_keys = 0, False
    sc = _walk(seed)["scenario"]
    for step in sc["steps"]:
        if step["op"] == "reset":
            long_keys = False
        for b in step["batches"] if step["op"] == "consume" else []:
            keys = [k for k in b["columns"]["k"] if k is not None]
            held = sum(len(k.encode()) for k in keys) + (b["lead"] * len((b["columns"]["k"][0] or "").encode()) if keys else 0)
            if keys and not long_keys and held < 16:
                out += 1
            long_keys = long_keys or any(len(k.encode()) > 15 for k in keys)
    return out


def _hot_key_heap(seed):
    """The key heap's cursor after the hot-key step: the hashed stage copied every row's key (8-byte
    aligned) of the batch it kept, the rolled-back batch's bytes are given back, and the general
    path adds each new group's key once."""
    first, second = next(b for b in _main_batches(seed) if len(b) == 2)
    kept = [k for k in first["columns"]["k"] if k is not None]
    new = {k for k in second["columns"]["k"] if k is not None} - set(kept)
    return sum(_pad8(k) for k in kept) + sum(_pad8(k) for k in new)


def _brief(run):
    keys = ("slots", "heap_used") + REACH_COUNTERS
    return [{k: p[k] for k in keys if p[k]} for p in run["readings"]]


def test_reach(gpu, monkeypatch):
    """Over the seed list under the DQ_FREQ_PART_MIN=1 configurations: every counter of paths() is
    non-zero at least once, and every template's transition shows within one table as a change
    between two paths() readings."""
    part, slots, budget = (_runs_of(monkeypatch, n) for n in ("part", "slots", "slots_budget"))
    top = {k: max(max(r["max"].get(k, 0) for r in runs.values()) for runs in (part, slots)) for k in REACH_COUNTERS}
    print("reach:", {n: {k: max(r["max"].get(k, 0) for r in runs.values()) for k in REACH_COUNTERS}
                     for n, runs in (("part", part), ("slots", slots), ("slots_budget", budget))})
    misses = []

    def need(ok, what, run=None):
        if not ok:
            misses.append((what, _brief(run) if run else None))

    by = lambda runs, template: [r for r in runs.values() if r["template"] == template]  # noqa: E731
    consume = lambda s: s["op"] == "consume"  # noqa: E731
    for k in REACH_COUNTERS:
        need(top[k] > 0, "counter %s never moved" % k)

    # a rollback and a format change in one consume step, and the record formats on both sides of it
    # (packed -> 16-byte: the packed regions, then the 16-byte ones, each in a partition run of its own;
    # into hashed: hashed records go one by one into a table that already holds groups)
    for template, before, after in (("packed_to_rec16_rollback", "packed_runs", "partition_runs"),
                                    ("rec16_to_hashed", "partition_runs", "hashed_inserts"),
                                    ("uuid_to_hashed_late", "uuid_runs", "hashed_inserts"),
                                    ("raw16_to_hashed", "raw16_runs", "hashed_inserts")):
        for runs in (part, slots):
            for r in by(runs, template):
                need(_seen(r, lambda s, a, b, dl: consume(s) and dl["rollbacks"] >= 1 and
                           dl["materialized_for_format"] >= 1), template + ": rollback and format change", r)
        for r in by(slots, template):
            need(_seen(r, lambda s, a, b, dl: consume(s) and dl["rollbacks"] >= 1 and dl[before] >= 1 and
                       dl[after] >= (2 if after == "partition_runs" else 1)), "%s: %s then %s" % (template, before, after), r)
    rolled = by(part, "packed_to_hashed_unsampled")
    for r in rolled:
        need(_seen(r, lambda s, a, b, dl: consume(s) and dl["rollbacks"] >= 1), "packed_to_hashed_unsampled: rollback", r)
    need(any(_seen(r, lambda s, a, b, dl: dl["materialized_for_format"] >= 1) for r in rolled),
         "packed_to_hashed_unsampled: format change")
    need(any(_seen(r, lambda s, a, b, dl: dl["rollbacks"] >= 1 and dl["packed_runs"] >= 1 and dl["hashed_inserts"] >= 1)
             for r in by(slots, "packed_to_hashed_unsampled")), "packed_to_hashed_unsampled: packed_runs then hashed_inserts")
    # the rolled-back batch of 28000 new ids: the 38000 records staged before it hold 1500 ids, so a
    # table sized from the restored sketch keeps its 2^16 slots through the step (1.15 x 1500 + 4096 <
    # 2^15 for the UUID regions; (1500 + 28000) x 10 < 2^16 x 6 for the hashed records after them),
    # and one sized from a sketch that kept the rolled-back hashes has 2^17 (1.15 x 29500 + 4096 > 2^15)
    for r in by(part, "uuid_to_hashed_late"):
        need(_seen(r, lambda s, a, b, dl: consume(s) and dl["rollbacks"] >= 1 and b["slots"] == 1 << 16),
             "uuid_to_hashed_late: 2^16 slots after the rollback", r)
    # the hot key: rolled back, nothing of the batch inserted as hashed records, and the key heap's
    # cursor back where the batch found it (then the general path's new groups)
    for runs in (part, slots):
        for r in by(runs, "hashed_rollback_hot_key"):
            want = _hot_key_heap(r["seed"])
            need(_seen(r, lambda s, a, b, dl: consume(s) and dl["rollbacks"] >= 1 and a["heap_used"] == 0 and
                       b["heap_used"] == want), "hashed_rollback_hot_key: heap cursor %d" % want, r)
    for r in by(part, "hashed_rollback_hot_key"):
        need(_seen(r, lambda s, a, b, dl: consume(s) and dl["rollbacks"] >= 1 and dl["materialized_for_format"] == 0 and
                   0 < dl["hashed_inserts"] < 40000), "hashed_rollback_hot_key: rollback to the general path", r)
    for r in by(slots, "hashed_rollback_hot_key"):
        need(_seen(r, lambda s, a, b, dl: consume(s) and dl["rollbacks"] >= 1 and dl["hashed_runs"] >= 1),
             "hashed_rollback_hot_key: hashed_runs", r)
    # reset: the next batch is probed like a table's first, so no batch is rolled back for its keys
    # in the whole walk; the only rollbacks are those of batches under 16 key bytes (_tiny_rollbacks:
    # one each in the walks of seeds 110 and 123, whose last batch is one 12-digit key), and such a
    # batch turns no table to hashed records
    for r in by(part, "reset_to_other_format"):
        tiny = _tiny_rollbacks(r["seed"])
        need(r["readings"][-1]["rollbacks"] == tiny, "reset_to_other_format: %d rollbacks expected" % tiny, r)
        need(not _seen(r, lambda s, a, b, dl: dl["rollbacks"] >= 1 and dl["hashed_inserts"] >= 1),
             "reset_to_other_format: a small batch as hashed records", r)
    for r in by(slots, "reset_to_other_format"):
        cut = [s["op"] for s in r["steps"]].index("reset")
        fmt = lambda a, b: tuple(b[k] - a[k] > 0 for k in FORMAT_COUNTERS)  # noqa: E731
        need(fmt(r["readings"][0], r["readings"][cut]) != fmt(r["readings"][cut], r["readings"][-1]),
             "reset_to_other_format: another format", r)
    # merge: the second table took another record format than the first
    for r in by(slots, "merge_two_formats"):
        cut = [s["op"] for s in r["steps"]].index("merge")
        first = tuple(r["readings"][cut][k] > 0 for k in FORMAT_COUNTERS)
        need(any(f != first and any(f) for f in r["second_formats"]), "merge_two_formats: %r %r" % (first, r["second_formats"]), r)
    # early aggregation: within one consume step two partition runs, or (hashed records) one run
    # into the empty table and then inserts into the table that holds groups -- without the budget
    # the step's batches are aggregated in one run
    early = lambda s, a, b, dl: consume(s) and (dl["partition_runs"] >= 2 or (  # noqa: E731
        dl["hashed_runs"] >= 1 and dl["hashed_inserts"] >= 1))
    for r in by(budget, "early_aggregation"):
        need(_seen(r, early), "early_aggregation: with the budget", r)
    for r in by(slots, "early_aggregation"):
        need(not _seen(r, early), "early_aggregation: without the budget", r)
    # growth across batches past the initial 2^16 slots
    for r in by(part, "growth_70k"):
        slots_seen = [p["slots"] for p in r["readings"]]
        need(slots_seen[1] == 1 << 16 and max(slots_seen) > 1 << 16, "growth_70k: %r" % slots_seen)
    for r in by(part, "few_groups_partition"):
        need(r["max"]["small_runs"] >= 1, "few_groups_partition: small_runs", r)
    need(any(r["max"]["import_coarse_runs"] >= 1 for r in by(part, "few_groups_partition")), "import_coarse_runs")
    need(any(r["max"]["import_skipped_runs"] >= 1 for r in by(slots, "few_groups_partition")), "import_skipped_runs")
    need(any(r["max"]["raw16_runs"] >= 1 for r in by(slots, "pair_walk")), "pair_walk: raw16_runs")
    for what, readings in misses:
        print("reach miss:", what, readings)
    assert not misses, [what for what, _ in misses]


# ---------------------------------------------------------------- regressions the walks found
def _fields_of(t):
    s = t.summary()
    return s.num_rows, s.num_groups, s.num_unique, s.grouped_rows


def test_rolled_back_batch_on_the_general_path_is_in_the_summary(gpu, monkeypatch):
    """Reduced from the walks of seeds 118 and 131 under DQ_FREQ_PART_MIN=1 with DQ_FREQ_HASHED=0: a
    staged batch of digit keys, then a batch with one 17-byte key.  The second batch is rolled back
    and grouped on the general path; dq_freq_consume aggregated the first one on the way (into an
    empty table, on the partition path, which marks the count-of-counts it fused as valid) and the
    summary then described the table without the second batch: 523 grouped rows for 11318."""
    _set_env(monkeypatch, "part_hashed0")
    a = ["%09d" % (i % 400) for i in range(1000)]
    b = ["%09d" % (i % 700) for i in range(1000)]
    b[-1] = "x" * 17
    t = FrequencyTable(["k"], {"k": "string"})
    t.reserve(2000)
    t.consume(d.Table.from_pydict({"k": ("string", a)}))
    t.consume(d.Table.from_pydict({"k": ("string", b)}))
    assert t.paths()["rollbacks"] == 1
    assert _fields_of(t) == (2000, 701, 301, 2000)
    c, k = t.top(1)  # (the slice maxima are as stale as the count-of-counts)
    assert list(zip(c.tolist(), k)) == [(5, b"%09d" % i) for i in range(200)]
    assert len(_export(t)) == 701
    t.close()


def test_hot_key_rolled_back_from_hashed_regions_is_in_the_summary(gpu, monkeypatch):
    """Reduced from the walks of seeds 109, 122 and 135 under DQ_FREQ_PART_SLOTS=1048576: hashed
    regions of long keys, then 78000 rows of which 96 % hold one key, more than its region and the
    overflow list take.  The batch is rolled back to the general path, and the key heap's cursor
    with it (paths()["heap_used"]); the summary counted 1500 groups and 17963 grouped rows for 2691
    and 95963."""
    _set_env(monkeypatch, "slots")
    a = ["a-long-grouping-key-%06d" % (i % 1500) for i in range(18000)]
    b = ["a-long-grouping-key-%06d" % (424242 if i % 25 else 1000 + i % 2000) for i in range(78000)]
    t = FrequencyTable(["k"], {"k": "string"})
    t.reserve(96000)
    t.consume(d.Table.from_pydict({"k": ("string", a)}))
    t.consume(d.Table.from_pydict({"k": ("string", b)}))
    p = t.paths()
    assert p["rollbacks"] == 1 and p["hashed_runs"] == 1, p
    want = {}
    for key in a + b:
        want[key.encode()] = want.get(key.encode(), 0) + 1
    # the heap cursor: the 18000 keys the hashed stage kept (26 bytes, 8-aligned: 32), the rolled-back
    # batch's 78000 x 32 bytes given back, then one key per group the general path added
    assert p["heap_used"] == 32 * 18000 + 32 * (len(want) - 1500), p
    assert _fields_of(t) == (96000, len(want), sum(1 for c in want.values() if c == 1), 96000)
    c, k = t.top(1)
    assert list(zip(c.tolist(), k)) == [(74880, b"a-long-grouping-key-424242")]
    assert _export(t) == want
    t.close()


def test_batch_under_16_key_bytes_keeps_the_record_format(gpu, monkeypatch):
    """Reduced from the walks of seeds 110 and 123 (reset, digit keys, then a batch of one 12-digit
    key): the string staging kernels cannot read a key column of fewer than 16 bytes and hand the
    batch to the general path by a rollback.  They reported it as a 16-byte key, which also turned
    the table to hashed records for good: the one row, and every batch after it, went in as hashed
    records with their keys in the heap."""
    _set_env(monkeypatch, "part")
    t = FrequencyTable(["k"], {"k": "string"})
    t.consume(d.Table.from_pydict({"k": ("string", ["000000004192"])}))
    p = t.paths()
    assert (p["rollbacks"], p["hashed_inserts"], p["heap_used"]) == (1, 0, 0), p
    more = ["%012d" % (i % 400) for i in range(1000)]
    t.consume(d.Table.from_pydict({"k": ("string", more)}))
    p = t.paths()
    assert (p["rollbacks"], p["hashed_inserts"], p["heap_used"]) == (1, 0, 0), p
    want = {b"%012d" % i: (3 if i < 200 else 2) for i in range(400)}
    want[b"000000004192"] = 1
    assert _fields_of(t) == (1001, 401, 1, 1001) and _export(t) == want
    t.close()


def test_format_change_inside_one_consume_is_in_the_summary(gpu, monkeypatch):
    """The walk of packed_to_rec16_rollback by hand, under DQ_FREQ_PART_SLOTS=1048576: packed regions,
    then 78000 keys that do not pack.  The second batch is rolled back and staged again as 16-byte
    records; on the way begin_region_stage aggregates the packed regions into the empty table, which
    marks the fused count-of-counts and slice maxima valid, and the 16-byte regions are later
    aggregated into the table that holds groups: the partition path drops those views there."""
    _set_env(monkeypatch, "slots")
    a = ["%012d" % (i % 3000) for i in range(17000)]
    b = ["k%x-%d" % (i % 2500 * 40503 % 65536, i % 2500) for i in range(78000)]
    t = FrequencyTable(["k"], {"k": "string"})
    t.reserve(95000)
    t.consume(d.Table.from_pydict({"k": ("string", a)}))
    t.consume(d.Table.from_pydict({"k": ("string", b)}))
    p = t.paths()
    assert (p["rollbacks"], p["materialized_for_format"]) == (1, 1) and p["packed_runs"] >= 1 and p["partition_runs"] >= 2, p
    want = {}
    for key in a + b:
        want[key.encode()] = want.get(key.encode(), 0) + 1
    assert _fields_of(t) == (95000, len(want), sum(1 for c in want.values() if c == 1), 95000)
    c, k = t.top(3)
    cut = sorted(want.values(), reverse=True)[2]
    assert list(zip(c.tolist(), k)) == sorted(((n, key) for key, n in want.items() if n >= cut), key=lambda x: (-x[0], x[1]))
    assert _export(t) == want
    t.close()


@pytest.mark.parametrize("how", ["import_groups", "merge_from", "import_parts"])
def test_staged_batch_then_import_is_in_the_summary(gpu, monkeypatch, how):
    """The same stale views by the other door: a staged batch that an import aggregates on its way
    in (the importers dropped the derived views before that aggregation, not after it; import_groups
    and merge_from showed it, import_parts is held to the same)."""
    import torch
    _set_env(monkeypatch, "part")
    a = ["%09d" % (i % 400) for i in range(1000)]
    more = {b"%09d" % i: 3 for i in range(300, 900)}
    t = FrequencyTable(["k"], {"k": "string"})
    t.consume(d.Table.from_pydict({"k": ("string", a)}))
    if how == "import_groups":
        t.import_groups(list(more.values()), list(more.keys()), 1800)
    else:
        o = FrequencyTable(["k"], {"k": "string"})
        o.import_groups(list(more.values()), list(more.keys()), 1800)
        if how == "merge_from":
            t.merge_from(o)
        else:
            pp, pg, pk = o.partition_sizes(2)
            buf = torch.empty(max(16, sum(o.part_bytes(x, y) for x, y in zip(pp, pg))), dtype=torch.uint8, device="cuda")
            keys = torch.empty(max(8, sum(pk)), dtype=torch.uint8, device="cuda")
            o.partition_into(2, buf, keys)
            t.import_parts(buf, pp, pg, keys, pk, num_rows=1800)
        o.close()
    want = {b"%09d" % i: (3 if i < 200 else 2) for i in range(400)}
    for key, c in more.items():
        want[key] = want.get(key, 0) + c
    assert _fields_of(t) == (2800, 900, 0, 2800)
    c, k = t.top(1)
    assert list(zip(c.tolist(), k)) == [(5, b"%09d" % i) for i in range(300, 400)]
    assert _export(t) == want
    t.close()


def test_composite_key_past_64_bytes_is_rolled_back_then_declined(gpu, monkeypatch):
    """What no walk holds, because the table is unusable afterwards: an (int64, string) key whose
    encoding passes 64 bytes.  The hashed staging rolls the batch back (rollbacks moves) and the
    general path declines it: DQ_ERR_UNSUPPORTED."""
    from deequ_amd import _lib as L
    _set_env(monkeypatch, "part")
    cfg = F.make_config("i64_s")
    t = _new_table(cfg)
    t.reserve(3000)
    names = ["mid-key-%d-yyyyyyy" % (i % 300) for i in range(1000)]
    t.consume(d.Table.from_pydict({"a": ("int64", list(range(1000))), "k": ("string", names)}))
    bad = list(names)
    bad[-1] = "x" * 70
    with pytest.raises(L.DeequAmdError) as e:
        t.consume(d.Table.from_pydict({"a": ("int64", list(range(1000))), "k": ("string", bad)}))
    assert e.value.status == L.DQ_ERR_UNSUPPORTED
    assert t.paths()["rollbacks"] == 1
    t.close()
