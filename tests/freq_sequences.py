"""Generated step sequences for the frequency table, and the dict model they are replayed against.

The group-by behind Uniqueness, Distinctness, Entropy, Histogram, MutualInformation and Distance is
a state machine: a table latches a record format from the first batch's sampled keys, rolls a batch
back when a key does not fit that format, aggregates the staged regions when the format changes, and
takes merges, imports, partitions and resets in between.  The hand-built tests each check one such
transition; this module generates whole walks.  It is pure Python, deterministic from a seed, and
shared by tests/test_freq_sequences.py (CPU: the generator and the model alone) and
tests/test_gpu_freq_sequences.py (GPU: every walk replayed on a FrequencyTable and on the model in
lock step).  It imports nothing of the library but the host key codec (encode_key), and nothing of
tests/fake_freq.py.

A scenario = {"seed", "template", "config", "steps"}:

  config  {"kind", "keys": [column], "schema": {column: dtype}, "histogram": bool, "where": text | None}
  step    {"op": "consume", "batches": [batch, ...]}   consumed back to back: nothing reads the table
                                                        in between, so the staged regions of one batch
                                                        meet the next batch (what a format change needs)
          {"op": "observe", "what": ..., ...}          summary / export / export_flat / to_arrow / top /
                                                        lookup / count_histogram / paths
          {"op": "merge", "steps": [...]}              merge_from a second table built by the sub-steps
          {"op": "distance", "steps": [...]}           linf_distance against such a table (read only)
          {"op": "mi"}                                 mutual_information (two key columns, read only)
          {"op": "import", "flat": bool, "batch": b}   import_groups / import_flat of the batch's groups
          {"op": "partition", "parts": 2 | 3, "preload": batch | None}
          {"op": "reserve", "rows": n} {"op": "expect_groups", "groups": n} {"op": "reset"}
  batch   {"source": "host" | "device" | "arrow", "lead": rows sliced off the Arrow array's front,
           "columns": {column: [value | None]}, "breaker": None | {"row", "placement", "shape"}}

Which rows the probes sample (deequ_amd/csrc/dq_freq.hip).  The pack probe (launch_freq_pack_probe),
the key-length probe (launch_freq_len_probe), the UUID probe (launch_freq_uuid_probe) and the 16-byte
probe (launch_freq_len16_probe) all sample the same rows of the table's first staged batch: every row
when the batch has at most 16384 rows, else the 16384 rows (i * 11400714819323198485 mod 2^64) mod
n_rows for i in [0, 16384) -- scattered, not strided.  A row whose first key column is NULL (or that
the table's filter dropped) counts for no probe.  probe_rows() restates that; a "breaker" -- the
first key that does not fit the table's record format -- is placed on a sampled row, on a row outside
the sample (batches of 17000+ rows), or on the very last row.

What the generator never draws, because the library declines it: decimal key columns
(reject_decimal), a filter on a Histogram table (dq_freq_set_filter), few_only tables (a batch past
the few-groups kernel is DQ_ERR_SPACE), and a multi-column key whose encoding passes 64 bytes
(kMaxLocalKey: the hashed staging rolls such a batch back and the general path then answers
DQ_ERR_UNSUPPORTED, "combined grouping key longer than 64 bytes", which leaves the table unusable;
the GPU test has a hand-written case for it).  A single string key may be longer than 64 bytes: it
is a hashed record like any other long key, and is drawn.  The hashed rollback that does go on to
the general path is the hot key's: template hashed_rollback_hot_key.

Two batch shapes are larger than the others, both because a region staging's overflow list holds
rows / 16 + 65536 records and only a batch that fills it rolls back: the 78000 non-digit keys that
turn a packed table to 16-byte records, and the 78000 rows of one hot key that send a hashed table's
batch to the general path.  Every other batch has at most 40000 rows.
"""
import json
import math
import random
import struct
from collections import Counter

import pyoracle as O
from deequ_amd.frequencies import encode_key

import distance_restated
import mi_restated

PROBE_ROWS = 16384
_GOLDEN = 11400714819323198485
MAX_LOCAL_KEY = 64

KINDS = {
    "s": (["k"], {"k": "string"}),
    "i64": (["a"], {"a": "int64"}),
    "i32": (["a"], {"a": "int32"}),
    "f64": (["f"], {"f": "float64"}),
    "b": (["b"], {"b": "bool"}),
    "i64_s": (["a", "k"], {"a": "int64", "k": "string"}),
    "i64_f64": (["a", "f"], {"a": "int64", "f": "float64"}),
    "s_s": (["k", "k2"], {"k": "string", "k2": "string"}),
    "three": (["a", "k", "b"], {"a": "int64", "k": "string", "b": "bool"}),
}
WHERE_COLUMN = "w"
WHERES = ("w > 0", "w IS NOT NULL AND w < 6", "w >= 2 OR w < -2")

TEMPLATES = (
    "packed_to_rec16_rollback", "packed_to_hashed_unsampled", "rec16_to_hashed", "uuid_to_hashed_late",
    "raw16_to_hashed", "hashed_rollback_hot_key", "reset_to_other_format", "merge_two_formats",
    "early_aggregation", "growth_70k", "few_groups_partition", "fixed_width_walk", "pair_walk",
)
# the walks the GPU test replays (and the CPU test checks): every template three times
SEEDS = tuple(range(101, 101 + 3 * len(TEMPLATES)))

SPECIAL_FLOATS = (0.0, -0.0, float("nan"), float("inf"), -float("inf"))
STRING_SHAPES = ("digits", "digits12", "alnum", "short3", "len15", "len16", "len17", "s16", "uuid", "uuid_upper",
                 "mid", "long", "over64")


def probe_rows(n_rows):
    """The rows of a first batch that the pack, key-length, UUID and 16-byte probes sample."""
    if n_rows <= PROBE_ROWS:
        return set(range(n_rows))
    return {((i * _GOLDEN) & 0xFFFFFFFFFFFFFFFF) % n_rows for i in range(PROBE_ROWS)}


def _uuid(v):
    x = (v * 0x9E3779B97F4A7C15 + 0x632BE59BD9B4E019) % 2 ** 64
    y = ((v ^ 0x5DEECE66D) * 0xC2B2AE3D27D4EB4F) % 2 ** 64
    h = "%016x%016x" % (x, y)
    return "%s-%s-%s-%s-%s" % (h[:8], h[8:12], h[12:16], h[16:20], h[20:32])


def value_of(shape, v):
    """The v-th value of a shape (v >= 0)."""
    if shape == "digits":  # 1 to 15 digits, leading zeros kept; the empty string among them
        if v % 97 == 0:
            return ""
        n = 1 + v % 15
        return str(v * 2654435761 % 10 ** n).zfill(n)
    if shape == "digits12":
        return "%012d" % v
    if shape == "alnum":  # at most 15 bytes, never a digit string; the empty string among them
        return "" if v % 89 == 0 else ("k%x-%d" % (v * 40503 % 65536, v))[:15]
    if shape == "short3":  # 1 to 3 bytes: a composite key that stays within a 16-byte record
        return "%x" % (v % 4096)
    if shape == "len15":
        return "x%014x" % v
    if shape == "len16":
        return "x%015x" % v
    if shape == "len17":
        return "x%016x" % v
    if shape == "s16":  # 16 bytes, hex: not a canonical UUID
        return "%016x" % (v * 0x9E3779B97F4A7C15 % 2 ** 64)
    if shape == "uuid":
        return _uuid(v)
    if shape == "uuid_upper":
        return _uuid(v).upper()
    if shape == "long":  # 18 to 64 bytes
        s = "long-key-%d-" % v
        return s + "z" * (18 + v % 47 - len(s))
    if shape == "mid":  # 18 to 26 bytes: two of them with their length prefixes stay within 64
        s = "mid-key-%d-" % v
        return s + "y" * (18 + v % 9 - len(s))
    if shape == "over64":  # 65 to 100 bytes (a single string key only)
        s = "over-64-%d-" % v
        return s + "w" * (65 + v % 36 - len(s))
    if shape == "int":
        return v - 500
    if shape == "bigint":
        return v * 1000003 * 4099 - 2 ** 45
    if shape == "bool":
        return bool(v & 1)
    if shape == "float":
        return SPECIAL_FLOATS[(v // 11) % len(SPECIAL_FLOATS)] if v % 11 == 0 else v * 0.25 - 40.0
    raise ValueError(shape)


def make_config(kind, histogram=False, where=None):
    keys, schema = KINDS[kind]
    schema = dict(schema)
    if where is not None:
        schema[WHERE_COLUMN] = "int64"
    return {"kind": kind, "keys": list(keys), "schema": schema, "histogram": histogram, "where": where}


def make_batch(rng, config, n, shapes, distinct, base=0, null_frac=0.03, hot=None, source=None, mods=None,
               breaker=None):
    """A batch of n rows.  shapes: {key column: shape}; row r draws one v in [base, base + distinct)
    (`hot` = (v, fraction): that v more often) and column c holds value_of(shape, v % mods[c]) or NULL.
    breaker = (column, shape, placement): one row, chosen by the placement, holds a key of that other
    shape (and is neither NULL nor filtered out)."""
    cols = {c: [] for c in config["schema"]}
    keys = config["keys"]
    mods = mods or {}
    for _ in range(n):
        v = hot[0] if hot and rng.random() < hot[1] else base + rng.randrange(distinct)
        for c in keys:
            if rng.random() < null_frac:
                cols[c].append(None)
            else:
                cols[c].append(value_of(shapes[c], v % mods[c] if c in mods else v))
        if config["where"] is not None:
            cols[WHERE_COLUMN].append(None if rng.random() < 0.05 else rng.randrange(-5, 10))
    info = None
    if breaker is not None and n > 0:
        column, shape, placement = breaker
        sampled = probe_rows(n)
        if placement == "unsampled" and n > PROBE_ROWS:
            outside = [r for r in range(n - 1) if r not in sampled]
            row = outside[rng.randrange(len(outside))]
        elif placement == "last":
            row = n - 1
        else:
            placement = "sampled"
            row = sorted(sampled)[rng.randrange(len(sampled))]
        for c in keys:
            if cols[c][row] is None:
                cols[c][row] = value_of(shapes[c], base)
        cols[column][row] = value_of(shape, base + distinct + 7)
        if config["where"] is not None:
            cols[WHERE_COLUMN][row] = 3  # (every filter of WHERES keeps w = 3)
        info = {"row": row, "placement": placement, "shape": shape, "sampled": row in sampled}
    source = source or rng.choice(("host", "host", "device", "arrow"))
    return {"source": source, "lead": rng.choice((1, 3, 8, 13)) if source == "arrow" else 0, "columns": cols,
            "breaker": info}


def batch_rows(batch):
    return len(next(iter(batch["columns"].values())))


# ---------------------------------------------------------------- the model
def _hist_value(text, dtype):
    """Histogram's cast-to-string key back to the column's value (None: the NULL group)."""
    if dtype == "string":
        return text
    if text == "NullValue":
        return None
    if dtype == "bool":
        return text == "true"
    if dtype == "float64":
        return float({"Infinity": "inf", "-Infinity": "-inf", "NaN": "nan"}.get(text, text))
    return int(text)


def _plain(key, dtypes):
    """The oracle keys floats by their bits: back to the float of those bits."""
    return [struct.unpack("<d", struct.pack("<Q", v[1]))[0] if t == "float64" else v for v, t in zip(key, dtypes)]


def group_batch(config, batch):
    """(Counter {encoded key: count}, numRows) of one batch: the oracle's grouping of the rows the
    filter keeps (O._where_mask is TRUE), keys through encode_key."""
    keys = config["keys"]
    dtypes = [config["schema"][c] for c in keys]
    table = {c: O.OColumn(config["schema"][c], list(v)) for c, v in batch["columns"].items()}
    if config["where"] is not None:
        keep = [m is True for m in O._where_mask(table, config["where"])]
        table = {c: O.OColumn(col.dtype, [v for v, kp in zip(col.values, keep) if kp]) for c, col in table.items()}
    if config["histogram"]:
        st = O.histogram_state(table, keys[0])
        out = Counter()
        for (text,), c in st.frequencies.items():
            out[encode_key([_hist_value(text, dtypes[0])], dtypes, True)] += c
        return out, st.num_rows
    st = O.frequencies_state(table, keys)
    return Counter({encode_key(_plain(k, dtypes), dtypes): c for k, c in st.frequencies.items()}), st.num_rows


def split_fields(key, dtypes):
    """An encoded multi-column key -> its fields' bytes (a string without its length prefix)."""
    width = {"bool": 1, "int32": 4, "int64": 8, "float64": 8}
    out, pos = [], 0
    for t in dtypes:
        if t == "string":
            n = struct.unpack_from("<I", key, pos)[0]
            pos += 4
        else:
            n = width[t]
        out.append(key[pos:pos + n])
        pos += n
    assert pos == len(key)
    return tuple(out)


class Model:
    """dict {encoded key: count} + num_rows, with Counter arithmetic; the expected value of every
    observer, written without the code under test."""

    def __init__(self, config):
        self.config = config
        self.dtypes = [config["schema"][c] for c in config["keys"]]
        self.groups = Counter()
        self.num_rows = 0

    def add(self, groups, num_rows):
        self.groups.update(groups)
        self.num_rows += num_rows

    def consume(self, batch):
        self.add(*group_batch(self.config, batch))

    def reset(self):
        self.groups = Counter()
        self.num_rows = 0

    def export(self):
        return dict(self.groups)

    def summary(self):
        """(num_rows, num_groups, num_unique, grouped_rows, entropy or None)."""
        counts = self.groups.values()
        st = O.FrequenciesAndNumRows(dict(self.groups), self.num_rows)
        return (self.num_rows, len(self.groups), sum(1 for c in counts if c == 1), sum(counts), O.entropy_exact(st))

    def top(self, n):
        """FrequencyTable.top's contract: the groups whose count is at least the n-th largest count
        (ties at the cut kept), count descending then encoded key ascending."""
        if not self.groups or n < 1:
            return []
        ordered = sorted(self.groups.items(), key=lambda kv: (-kv[1], kv[0]))
        cut = ordered[min(n, len(ordered)) - 1][1]
        return [(c, k) for k, c in ordered if c >= cut]

    def lookup(self, key):
        return self.groups.get(key, 0)

    def count_histogram(self, n_bins):
        hist = [0] * n_bins
        big = []
        for c in self.groups.values():
            if c < n_bins:
                hist[c] += 1
            else:
                big.append(c)
        return hist, sorted(big)

    def distance(self, other):
        """(linf_simple, n, m, groups_a, groups_b, groups_common) per tests/distance_restated.py."""
        linf, n, m = distance_restated.linf_simple(self.groups, other.groups)
        return linf, int(n), int(m), len(self.groups), len(other.groups), len(set(self.groups) & set(other.groups))

    def mutual_information(self):
        """mi_restated.restate over the joint groups keyed by their fields' bytes."""
        joint = {split_fields(k, self.dtypes): c for k, c in self.groups.items()}
        return mi_restated.restate(joint, self.num_rows)

    def lookup_keys(self, rng):
        """Present, absent and longer-than-16-byte keys to look up."""
        present = sorted(self.groups)
        picks = [present[rng.randrange(len(present))] for _ in range(min(3, len(present)))]
        longer = [k for k in present if len(k) > 16][:1]
        absent = [b"absent-key-no-table-holds-it", b"\xff" * 7, b"never-" + b"x" * 70]
        return picks + longer + absent


def sub_table_model(config, steps):
    m = Model(config)
    for s in steps:
        for b in s["batches"]:
            m.consume(b)
    return m


def replay_model(scenario):
    """The model after every step: [(groups dict, num_rows)]; needs no GPU."""
    m = Model(scenario["config"])
    out = []
    for step in scenario["steps"]:
        apply_to_model(m, step)
        out.append((m.export(), m.num_rows))
    return out


def apply_to_model(m, step):
    op = step["op"]
    if op == "consume":
        for b in step["batches"]:
            m.consume(b)
    elif op == "merge":
        other = sub_table_model(m.config, step["steps"])
        m.add(other.groups, other.num_rows)
    elif op == "import":
        groups, rows = group_batch(m.config, step["batch"])
        m.add(groups, rows)
    elif op == "reset":
        m.reset()
    elif op not in ("observe", "distance", "mi", "partition", "reserve", "expect_groups"):
        raise ValueError(op)


# ---------------------------------------------------------------- templates
def _observers(rng, k=3):
    """k observer steps in random order."""
    pool = [{"op": "observe", "what": "summary"}, {"op": "observe", "what": "export"},
            {"op": "observe", "what": "export_flat"}, {"op": "observe", "what": "to_arrow"},
            {"op": "observe", "what": "top", "n": 1}, {"op": "observe", "what": "top", "n": 5},
            {"op": "observe", "what": "top", "n": 1 << 20}, {"op": "observe", "what": "lookup"},
            {"op": "observe", "what": "count_histogram", "n_bins": 1 << 16},
            {"op": "observe", "what": "count_histogram", "n_bins": 8}, {"op": "observe", "what": "paths"}]
    return rng.sample(pool, k)


def _big(rng):
    return rng.randrange(17000, 21000)


def _small(rng):
    return rng.choice((0, 1, 63, 64, 65, rng.randrange(900, 1100)))


def _consume(*batches):
    return {"op": "consume", "batches": list(batches)}


def _tail(rng, config, shapes, distinct, steps, mods=None):
    """Random rest of a walk: small batches of the same columns, observers, sometimes an import."""
    for _ in range(rng.randrange(1, 3)):
        steps.append(_consume(make_batch(rng, config, _small(rng), shapes, distinct, null_frac=rng.choice((0.0, 0.05, 0.3)),
                                         mods=mods)))
        steps.extend(_observers(rng, rng.randrange(1, 4)))
    if rng.random() < 0.5:
        steps.append({"op": "import", "flat": rng.random() < 0.5,
                      "batch": make_batch(rng, config, rng.randrange(50, 400), shapes, distinct, mods=mods)})
        steps.extend(_observers(rng, 2))


def _t_packed_to_rec16_rollback(rng, variant):
    cfg = make_config("s", histogram=rng.random() < 0.3)
    n1 = _big(rng)
    steps = [{"op": "reserve", "rows": n1 + 78000}]
    first = make_batch(rng, cfg, n1, {"k": "digits12"}, 3000, null_frac=0.02, hot=(17, 0.05))
    # more keys that do not pack than the packed stage's overflow list holds (rows / 16 + 65536)
    other = make_batch(rng, cfg, 78000, {"k": "alnum"}, 2500, null_frac=0.005)
    steps.append(_consume(first, other))
    steps.extend(_observers(rng, 3))
    steps.append(_consume(make_batch(rng, cfg, _small(rng), {"k": "digits"}, 500)))
    _tail(rng, cfg, {"k": "alnum"}, 2500, steps)
    return cfg, steps


def _t_packed_to_hashed_unsampled(rng, variant):
    cfg = make_config("s", where=rng.choice((None, None, WHERES[0])))
    n = _big(rng)
    steps = [{"op": "reserve", "rows": n + 1100}]
    first = make_batch(rng, cfg, rng.randrange(900, 1100), {"k": "digits"}, 4000)
    second = make_batch(rng, cfg, n, {"k": "digits"}, 4000, null_frac=0.04,
                        breaker=("k", rng.choice(("len17", "long", "len16")), "unsampled"))
    # (every third walk: the long key hides in the table's first batch, which the pack probe samples)
    steps.append(_consume(second) if variant % 3 == 2 else _consume(first, second))
    steps.extend(_observers(rng, 3))
    steps.append(_consume(make_batch(rng, cfg, _small(rng), {"k": "long"}, 300)))
    _tail(rng, cfg, {"k": "digits"}, 4000, steps)
    return cfg, steps


def _t_rec16_to_hashed(rng, variant):
    cfg = make_config("i64_s")
    n = _big(rng)
    mods = {"a": 700}
    steps = [{"op": "reserve", "rows": 2 * n}]
    first = make_batch(rng, cfg, n, {"a": "int", "k": "short3"}, 5000, mods=mods)
    second = make_batch(rng, cfg, rng.randrange(900, 1100), {"a": "int", "k": "short3"}, 5000, mods=mods,
                        breaker=("k", "mid", ("sampled", "last")[variant % 2]))
    steps.append(_consume(first, second))
    steps.extend(_observers(rng, 2))
    steps.append({"op": "mi"})
    steps.append(_consume(make_batch(rng, cfg, _small(rng), {"a": "bigint", "k": "mid"}, 900, mods=mods)))
    _tail(rng, cfg, {"a": "int", "k": "short3"}, 5000, steps, mods=mods)
    return cfg, steps


def _t_uuid_to_hashed_late(rng, variant):
    cfg = make_config("s")
    # 38000 staged rows of 1500 ids, then 28000 distinct ids with one that is not canonical: the
    # rolled-back batch's hashes must leave the sizing sketch before the UUID regions are aggregated
    # (see the GPU test's reach check)
    steps = [{"op": "reserve", "rows": 66000}]
    first = make_batch(rng, cfg, 38000, {"k": "uuid"}, 1500, null_frac=0.01)
    second = make_batch(rng, cfg, 28000, {"k": "uuid"}, 10 ** 7, base=10 ** 5, null_frac=0.0,
                        breaker=("k", "uuid_upper", ("unsampled", "last")[variant % 2]))
    steps.append(_consume(first, second))
    steps.extend(_observers(rng, 3))
    steps.append(_consume(make_batch(rng, cfg, _small(rng), {"k": "uuid_upper"}, 400)))
    _tail(rng, cfg, {"k": "uuid"}, 6000, steps)
    return cfg, steps


def _t_raw16_to_hashed(rng, variant):
    cfg = make_config("s")
    n = _big(rng)
    steps = [{"op": "reserve", "rows": 2 * n}]
    first = make_batch(rng, cfg, n, {"k": rng.choice(("s16", "len16"))}, 7000)
    second = make_batch(rng, cfg, rng.randrange(900, 1100), {"k": "s16"}, 7000,
                        breaker=("k", rng.choice(("len17", "len15", "uuid")), ("last", "sampled")[variant % 2]))
    steps.append(_consume(first, second))
    steps.extend(_observers(rng, 3))
    _tail(rng, cfg, {"k": "s16"}, 7000, steps)
    return cfg, steps


def _t_hashed_rollback_hot_key(rng, variant):
    cfg = make_config("s")
    n1 = _big(rng)
    steps = [{"op": "reserve", "rows": n1 + 78000}]
    first = make_batch(rng, cfg, n1, {"k": "long"}, 1500, null_frac=0.01, source="device")
    # one key on 96 % of 78000 rows: more records than its region and the overflow list
    # (rows / 16 + 65536 records) hold, so the hashed staging rolls back, heap cursor included, and the
    # batch is grouped on the general path
    second = make_batch(rng, cfg, 78000, {"k": "long"}, 2000, base=1000, null_frac=0.0, hot=(424242, 0.96))
    steps.append(_consume(first, second))
    steps.extend(_observers(rng, 3))
    steps.append(_consume(make_batch(rng, cfg, _small(rng), {"k": "over64"}, 50)))  # (single strings past 64 bytes)
    steps.extend(_observers(rng, 2))
    return cfg, steps


def _t_reset_to_other_format(rng, variant):
    cfg = make_config("s", histogram=rng.random() < 0.3)
    n = _big(rng)
    a, b = rng.choice((("digits12", "uuid"), ("uuid", "digits12"), ("digits", "long"), ("s16", "digits")))
    steps = [_consume(make_batch(rng, cfg, n, {"k": a}, 5000))]
    steps.extend(_observers(rng, 2))
    steps.append({"op": "reset"})
    steps.extend(_observers(rng, 2))
    steps.append(_consume(make_batch(rng, cfg, n, {"k": b}, 5000)))
    steps.extend(_observers(rng, 2))
    _tail(rng, cfg, {"k": b}, 5000, steps)
    return cfg, steps


def _t_merge_two_formats(rng, variant):
    cfg = make_config("s", where=rng.choice((None, WHERES[1])))
    a, b = rng.choice((("digits12", "uuid"), ("uuid", "alnum"), ("s16", "long"), ("digits", "uuid_upper")))
    n = _big(rng)
    steps = [_consume(make_batch(rng, cfg, n, {"k": a}, 4000))]
    steps.append({"op": "observe", "what": "top", "n": 5})
    steps.append({"op": "merge", "steps": [_consume(make_batch(rng, cfg, n, {"k": b}, 4000)),
                                           _consume(make_batch(rng, cfg, _small(rng), {"k": a}, 4000))]})
    steps.append({"op": "observe", "what": "top", "n": 5})
    steps.append({"op": "merge", "steps": [_consume(make_batch(rng, cfg, 0, {"k": b}, 10))]})  # no groups, no rows
    steps.append({"op": "observe", "what": "top", "n": 5})
    # a source whose every key is NULL: numRows moves, no group does
    steps.append({"op": "merge", "steps": [_consume(make_batch(rng, cfg, 65, {"k": b}, 10, null_frac=1.0))]})
    steps.extend(_observers(rng, 3))
    steps.append({"op": "distance", "steps": [_consume(make_batch(rng, cfg, 1000, {"k": b}, 4000))]})
    _tail(rng, cfg, {"k": a}, 4000, steps)
    return cfg, steps


def _t_early_aggregation(rng, variant):
    kind = ("s", "i64", "i64_s")[variant % 3]
    cfg = make_config(kind)
    shapes = {"s": {"k": "digits12"}, "i64": {"a": "bigint"}, "i64_s": {"a": "int", "k": "mid"}}[kind]
    steps = [{"op": "reserve", "rows": 60000}]
    # one step, three batches: under a small staging budget the first is aggregated before the second
    steps.append(_consume(make_batch(rng, cfg, _big(rng), shapes, 9000), make_batch(rng, cfg, 1000, shapes, 9000),
                          make_batch(rng, cfg, _big(rng), shapes, 9000, base=4000)))
    steps.extend(_observers(rng, 3))
    if kind == "i64_s":
        steps.append({"op": "mi"})
    _tail(rng, cfg, shapes, 9000, steps)
    return cfg, steps


def _t_growth_70k(rng, variant):
    kind = ("s", "i64", "s")[variant % 3]
    cfg = make_config(kind)
    shapes = {"s": {"k": rng.choice(("digits12", "len15", "uuid"))}, "i64": {"a": "bigint"}}[kind]
    steps = []
    for i in range(3):  # ~71000 distinct keys in all: past the initial 2^16 slots
        steps.append(_consume(make_batch(rng, cfg, 24000, shapes, 10 ** 7, base=i * 10 ** 7, null_frac=0.01)))
        steps.extend(_observers(rng, 1))
    steps.append({"op": "partition", "parts": 2, "preload": None})
    steps.append({"op": "distance", "steps": [_consume(make_batch(rng, cfg, 1000, shapes, 10 ** 7))]})
    return cfg, steps


def _t_few_groups_partition(rng, variant):
    kind = ("s", "i32", "b")[variant % 3]
    cfg = make_config(kind, histogram=rng.random() < 0.5)
    shapes = {"s": {"k": rng.choice(("digits", "alnum"))}, "i32": {"a": "int"}, "b": {"b": "bool"}}[kind]
    steps = [{"op": "expect_groups", "groups": 200}]
    steps.append(_consume(make_batch(rng, cfg, _big(rng), shapes, 150, null_frac=0.1, hot=(3, 0.4))))
    steps.extend(_observers(rng, 2))
    steps.append(_consume(make_batch(rng, cfg, _small(rng), shapes, 150)))
    # the parts of this small table into a table that already holds 40000 other groups
    pre_shapes = {"s": {"k": "len15"}, "i32": {"a": "int"}, "b": {"b": "bool"}}[kind]
    steps.append({"op": "partition", "parts": 3,
                  "preload": make_batch(rng, cfg, 40000, pre_shapes, 10 ** 7, base=1000, null_frac=0.0)})
    steps.append({"op": "partition", "parts": 2, "preload": None})
    steps.extend(_observers(rng, 2))
    return cfg, steps


def _t_fixed_width_walk(rng, variant):
    kind = ("f64", "i32", "b")[variant % 3]
    cfg = make_config(kind, histogram=rng.random() < 0.5, where=None)
    if not cfg["histogram"] and rng.random() < 0.5:
        cfg = make_config(kind, where=rng.choice(WHERES))
    shapes = {"f64": {"f": "float"}, "i64": {"a": "bigint"}, "i32": {"a": "int"}, "b": {"b": "bool"}}[kind]
    steps = []
    for n in (_small(rng), _big(rng), _small(rng)):
        steps.append(_consume(make_batch(rng, cfg, n, shapes, 800, null_frac=rng.choice((0.0, 0.1)))))
        steps.extend(_observers(rng, 2))
    steps.append({"op": "distance", "steps": [_consume(make_batch(rng, cfg, 500, shapes, 800))]})
    steps.append({"op": "reset"})
    steps.append(_consume(make_batch(rng, cfg, 65, shapes, 30)))
    steps.extend(_observers(rng, 2))
    return cfg, steps


def _t_pair_walk(rng, variant):
    kind = ("i64_f64", "s_s", "three")[variant % 3]
    cfg = make_config(kind)
    shapes = {"i64_f64": {"a": "int", "f": "float"}, "s_s": {"k": "mid", "k2": "alnum"},
              "three": {"a": "bigint", "k": "alnum", "b": "bool"}}[kind]
    mods = {"i64_f64": {"a": 300}, "s_s": {"k2": 40}, "three": {"k": 60}}[kind]
    n = _big(rng)
    steps = [{"op": "reserve", "rows": 2 * n}]
    steps.append(_consume(make_batch(rng, cfg, n, shapes, 6000, mods=mods),
                          make_batch(rng, cfg, _small(rng), shapes, 6000, mods=mods)))
    steps.extend(_observers(rng, 2))
    if len(cfg["keys"]) == 2:
        steps.append({"op": "mi"})
    if kind == "s_s":  # 26 + 15 bytes and two length prefixes: 49; the longest pair the shapes give is 4 + 26 + 4 + 15
        steps.append(_consume(make_batch(rng, cfg, 1000, {"k": "mid", "k2": "len15"}, 500)))
    steps.append({"op": "merge", "steps": [_consume(make_batch(rng, cfg, 1000, shapes, 6000, mods=mods))]})
    _tail(rng, cfg, shapes, 6000, steps, mods=mods)
    return cfg, steps


_BUILDERS = {name: globals()["_t_" + name] for name in TEMPLATES}


def scenario(seed):
    """The walk of a seed: its template is TEMPLATES[seed % len(TEMPLATES)] and the key columns of
    the templates that vary them rotate with seed // len(TEMPLATES); the rest is drawn."""
    rng = random.Random(seed)
    template = TEMPLATES[seed % len(TEMPLATES)]
    config, steps = _BUILDERS[template](rng, seed // len(TEMPLATES))
    return {"seed": seed, "template": template, "config": config, "steps": steps}


def all_batches(steps):
    for s in steps:
        if s["op"] == "consume":
            yield from s["batches"]
        elif s["op"] in ("merge", "distance"):
            yield from all_batches(s["steps"])
        elif s["op"] == "import":
            yield s["batch"]
        elif s["op"] == "partition" and s["preload"] is not None:
            yield s["preload"]


def fingerprint(sc):
    """The scenario as bytes (NaN and -0.0 keep their spelling): equal seeds give equal bytes."""
    return json.dumps(sc, sort_keys=True).encode()


def rel_err(a, b):
    if a == b or (math.isnan(a) and math.isnan(b)):
        return 0.0
    return abs(a - b) / max(abs(b), 1e-300)
