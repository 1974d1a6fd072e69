"""The generated frequency-table walks (tests/freq_sequences.py) without a GPU: the generator is
deterministic, the seed list of tests/test_gpu_freq_sequences.py holds every template, every table
configuration, every batch shape, size class, placement and source, the model replays every walk
(none is skipped: the GPU test replays the same list), and nothing is drawn that the library
declines."""
import collections
import math

import pytest

import freq_sequences as F
from deequ_amd.frequencies import encode_key


@pytest.fixture(scope="module")
def walks():
    return {seed: F.scenario(seed) for seed in F.SEEDS}


def test_same_seed_same_scenario_byte_for_byte(walks):
    for seed in F.SEEDS:
        assert F.fingerprint(F.scenario(seed)) == F.fingerprint(walks[seed])
    assert F.fingerprint(F.scenario(F.SEEDS[0])) != F.fingerprint(F.scenario(F.SEEDS[0] + len(F.TEMPLATES)))


def test_probe_rows_restate_the_kernels():
    """Every row up to 16384 rows; beyond, 16384 draws of (i * 11400714819323198485 mod 2^64) mod n."""
    assert F.probe_rows(0) == set() and F.probe_rows(65) == set(range(65))
    assert F.probe_rows(16384) == set(range(16384))
    s = F.probe_rows(17000)
    assert 0 in s and (11400714819323198485 % 17000) in s and ((2 * 11400714819323198485) % 2 ** 64) % 17000 in s
    assert 9000 < len(s) <= 16384 and max(s) < 17000
    assert len(set(range(17000)) - s) > 600  # rows that no probe sees


def test_seed_list_holds_every_template_and_configuration(walks):
    assert 30 <= len(F.SEEDS) <= 40
    assert collections.Counter(w["template"] for w in walks.values()) == {t: 3 for t in F.TEMPLATES}
    assert {w["config"]["kind"] for w in walks.values()} == set(F.KINDS)
    assert any(w["config"]["histogram"] for w in walks.values())
    assert any(w["config"]["where"] for w in walks.values())
    ops = {s["op"] for w in walks.values() for s in w["steps"]}
    assert ops == {"consume", "observe", "merge", "distance", "mi", "import", "partition", "reserve", "expect_groups",
                   "reset"}
    seen = {(s["what"], s.get("n")) for w in walks.values() for s in w["steps"] if s["op"] == "observe"}
    assert {w for w, _ in seen} == {"summary", "export", "export_flat", "to_arrow", "top", "lookup", "count_histogram",
                                    "paths"}
    assert {n for w, n in seen if w == "top"} == {1, 5, 1 << 20}
    assert {s["parts"] for w in walks.values() for s in w["steps"] if s["op"] == "partition"} == {2, 3}
    assert {s["flat"] for w in walks.values() for s in w["steps"] if s["op"] == "import"} == {False, True}


def test_batches_cover_the_shapes_sizes_placements_and_sources(walks):
    rows, sources, placements, lengths = set(), set(), set(), set()
    floats, uuid_forms, over_local = set(), set(), 0
    for w in walks.values():
        cfg = w["config"]
        batches = list(F.all_batches(w["steps"]))
        assert sum(1 for s in w["steps"] if s["op"] == "consume" for _ in s["batches"]) <= 8
        for b in batches:
            n = F.batch_rows(b)
            rows.add(n)
            sources.add(b["source"])
            assert b["lead"] > 0 if b["source"] == "arrow" else b["lead"] == 0
            if b["breaker"]:
                placements.add((b["breaker"]["placement"], b["breaker"]["sampled"]))
            for c, vals in b["columns"].items():
                t = cfg["schema"][c]
                for v in vals:
                    if v is None:
                        continue
                    if t == "string":
                        lengths.add(len(v.encode()))
                        if len(v) == 36 and v.count("-") == 4:
                            uuid_forms.add(v == v.lower())
                    elif t == "float64":
                        floats.add("nan" if v != v else "-0" if v == 0 and math.copysign(1, v) < 0 else v)
            if len(cfg["keys"]) > 1:  # the library declines an encoding past kMaxLocalKey: never drawn
                for r in range(n):
                    vals = [b["columns"][c][r] for c in cfg["keys"]]
                    if None not in vals:
                        assert len(encode_key(vals, [cfg["schema"][c] for c in cfg["keys"]])) <= F.MAX_LOCAL_KEY
            else:
                over_local += any(v is not None and len(v.encode()) > 64 for v in b["columns"][cfg["keys"][0]]) \
                    if cfg["schema"][cfg["keys"][0]] == "string" else 0
    assert {0, 1, 63, 64, 65} <= rows and any(900 <= n <= 1100 for n in rows) and any(17000 <= n <= 40000 for n in rows)
    # one batch shape needs more rows than 40000 (the packed stage's overflow list: the module's docstring)
    assert {n for n in rows if n > 40000} == {78000}
    assert sources == {"host", "device", "arrow"}
    assert {("sampled", True), ("unsampled", False)} <= placements and any(p == "last" for p, _ in placements)
    assert {0, 15, 16, 17, 36} <= lengths and any(18 <= n <= 64 for n in lengths) and any(n > 64 for n in lengths)
    assert uuid_forms == {True, False}
    assert {0.0, "-0", "nan", math.inf, -math.inf} <= floats
    assert over_local >= 3


def test_nothing_the_library_declines_is_drawn(walks):
    for w in walks.values():
        cfg = w["config"]
        assert not any(t.startswith("decimal") for t in cfg["schema"].values())
        assert not (cfg["histogram"] and cfg["where"])
        assert not (cfg["histogram"] and len(cfg["keys"]) > 1)
        for s in w["steps"]:
            if s["op"] == "mi":
                assert len(cfg["keys"]) == 2
            if s["op"] == "expect_groups":  # a hint; the table is not a few-groups-only one
                assert s["groups"] > 0


def test_model_replays_every_walk(walks):
    """Every walk of the seed list, on the model alone: none is skipped, every step has a state, the
    observers' expected values exist, and the named transition is in the walk."""
    for seed, w in walks.items():
        states = F.replay_model(w)
        assert len(states) == len(w["steps"]) > 0
        assert any(groups for groups, _ in states), seed
        m = F.Model(w["config"])
        for step, (groups, num_rows) in zip(w["steps"], states):
            F.apply_to_model(m, step)
            assert (m.export(), m.num_rows) == (groups, num_rows)
            if step["op"] == "reset":
                assert (groups, num_rows) == ({}, 0)
        rows, n_groups, unique, grouped, entropy = m.summary()
        assert n_groups == len(m.groups) and unique <= n_groups and grouped == sum(m.groups.values())
        assert (entropy is None) == (not m.groups)
        top = m.top(5)
        assert [c for c, _ in top] == sorted((c for c, _ in top), reverse=True) and len(top) >= min(5, n_groups)
        assert m.top(1 << 20) == sorted(((c, k) for k, c in m.groups.items()), key=lambda ck: (-ck[0], ck[1]))
        hist, big = m.count_histogram(8)
        assert sum(hist) + len(big) == n_groups and hist[0] == 0
        assert len(states[-1][0]) <= 110_000  # (a table stays small: at most ~100000 distinct keys)


def test_model_top_keeps_ties_at_the_cut():
    m = F.Model(F.make_config("s"))
    m.add({b"a": 3, b"b": 2, b"c": 2, b"d": 1}, 9)
    assert m.top(1) == [(3, b"a")]
    assert m.top(2) == [(3, b"a"), (2, b"b"), (2, b"c")]
    assert m.top(9) == [(3, b"a"), (2, b"b"), (2, b"c"), (1, b"d")]
    assert m.count_histogram(3) == ([0, 1, 2], [3])
    assert m.lookup(b"b") == 2 and m.lookup(b"zz") == 0


def test_model_groups_like_the_oracle():
    """The model's batch grouping on hand-checked rows: NULL keys drop out (or are Histogram's
    "NullValue" / empty key), a filter keeps the rows it is TRUE on, floats group by their bits."""
    cfg = F.make_config("s", where="w > 0")
    b = {"columns": {"k": ["7", None, "7", "x", "7"], "w": [1, 1, None, 2, -1]}}
    assert F.group_batch(cfg, b) == ({b"7": 1, b"x": 1}, 3)
    cfg = F.make_config("s", histogram=True)
    assert F.group_batch(cfg, {"columns": {"k": ["7", None, "NullValue"]}}) == ({b"7": 1, b"NullValue": 2}, 3)
    cfg = F.make_config("f64", histogram=True)
    got, rows = F.group_batch(cfg, {"columns": {"f": [0.0, -0.0, None, float("nan"), float("nan")]}})
    assert rows == 5 and got == {encode_key([0.0], ["float64"]): 1, encode_key([-0.0], ["float64"]): 1, b"": 1,
                                 encode_key([float("nan")], ["float64"], True): 2}
    cfg = F.make_config("i64_f64")
    got, rows = F.group_batch(cfg, {"columns": {"a": [1, 1, None], "f": [0.0, -0.0, 1.0]}})
    assert rows == 3 and got == {encode_key([1, 0.0], ["int64", "float64"]): 1,
                                 encode_key([1, -0.0], ["int64", "float64"]): 1}
    assert F.split_fields(encode_key([5, "ab"], ["int64", "string"]), ["int64", "string"]) == \
        ((5).to_bytes(8, "little"), b"ab")
