"""The group-by and KLL entry points over sliced key columns in hostile buffers (tests/hostile.py).

dq_freq_consume stages each key with one 16-byte load and packs digit keys and UUIDs into
records: a key followed by a NULL slot holding more digits, more hex, or 0xFF bytes must stay the
key it is.  Every path of test_gpu_heap_tail.PATHS (the partition path includes the hashed and
UUID records), keys of digits, 'k' + digits, 15 / 16 / 17 bytes and 36-character UUIDs,
composites whose NULL slots hold garbage, numeric keys of every dtype, and Histogram, where a NULL
is the "NullValue" group whatever its span holds.  Exact against O.frequencies_state /
O.histogram_state; no wait ever times out.  One KLL case: hostile float64 / int64 columns against
kll_sketch_slabs."""
import struct

import numpy as np
import pytest

import deequ_amd as d
import hostile as H
import pyoracle as O
from deequ_amd import kll
from deequ_amd.frequencies import FrequencyTable, encode_key
from deequ_amd.states import kll_sketch_slabs
from helpers import oracle_table
from test_gpu_freq_hashed import _uuid
from test_gpu_heap_tail import PATHS

pytestmark = pytest.mark.gpu

N = 2049
residency = pytest.mark.parametrize("device", [True, False], ids=["device", "host"])


def _nulls(rng, vals, frac=0.3):
    return [None if rng.random() < frac else v for v in vals]


def _string_keys(kind):
    rng = np.random.default_rng(len(kind) + 50)
    ids = rng.integers(0, 300, N)
    if kind == "digits":      # lengths 1..15: packed records; "9.e-" would lengthen the key
        keys = [str(int(v) * 10 ** int(v % 13)) for v in ids]
    elif kind == "kdigits":
        keys = ["k%d" % v for v in ids]
    elif kind == "len15_16_17":
        keys = ["%0*d" % (15 + int(v) % 3, int(v)) for v in ids]
    elif kind == "uuid":
        keys = [_uuid(int(v)) for v in ids]
    else:
        raise KeyError(kind)
    return _nulls(rng, keys)


KINDS = {"digits": "digits", "kdigits": "text", "len15_16_17": "digits", "uuid": "high"}


def _plain(key, dtypes):
    """The oracle keys floats by their bits: back to the float of those bits."""
    out = []
    for v, t in zip(key, dtypes):
        if t == "float64":
            v = struct.unpack("<d", struct.pack("<Q", v[1]))[0]
        elif t == "float32":
            v = struct.unpack("<f", struct.pack("<I", v[1]))[0]
        out.append(v)
    return out


def _want(spec, cols, hist=False):
    ot = oracle_table(spec)
    dtypes = [spec[c][0] for c in cols]
    if hist:  # (string columns: the histogram's keys are the strings, NULL -> "NullValue")
        return {k[0].encode(): c for k, c in O.histogram_state(ot, cols[0]).frequencies.items()}
    return {encode_key(_plain(k, dtypes), dtypes): c for k, c in O.frequencies_state(ot, cols).frequencies.items()}


def _group(table, cols, hist=False, few=None):
    t = FrequencyTable(cols, dict(table.schema), histogram=hist)
    try:
        if few is not None:
            t.expect_groups(few)
        t.reserve(table.num_rows)
        t.consume(table)
        counts, keys = t.export()
        paths = t.paths()
        print(cols, "hist" if hist else "", {k: v for k, v in paths.items() if v})
        assert paths["wait_timeouts"] == 0
        assert t.summary().num_rows == table.num_rows
        return dict(zip(keys, counts.tolist())), paths
    finally:
        t.close()


@residency
@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("kind", list(KINDS))
def test_string_keys_on_every_path(gpu, monkeypatch, kind, path, device):
    for k, v in PATHS[path].items():
        monkeypatch.setenv(k, v)
    spec = {"key": ["string", _string_keys(kind)]}
    for hist in (False, True):
        want = _want(spec, ["key"], hist)
        assert (b"NullValue" in want) == hist
        for off in (24, 61):
            table = H.hostile_table(spec, offset=off, flavour=KINDS[kind], device=device)
            got, paths = _group(table, ["key"], hist, few=min(len(want) + 1, 900) if path == "small" else None)
            assert got == want, (kind, path, hist, off)


RECORDS = [("digits", "packed_runs"), ("kdigits", "partition_runs"), ("len15_16_17", "hashed_runs"),
           ("uuid", "uuid_runs")]


@residency
@pytest.mark.parametrize("kind,counter", RECORDS, ids=[r[0] for r in RECORDS])
def test_region_records_aggregated_in_lds(gpu, monkeypatch, kind, counter, device):
    """test_gpu_freq_hashed's `part` environment with a table of 2^20 slots (one slice per
    level-1 region): the staged records -- packed digits, 16-byte, hashed, UUID -- are aggregated
    by the LDS slice kernels rather than inserted one by one."""
    for k, v in PATHS["partition"].items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("DQ_FREQ_PART_SLOTS", str(1 << 20))
    spec = {"key": ["string", _string_keys(kind)]}
    want = _want(spec, ["key"])
    for off in (8, 7):
        table = H.hostile_table(spec, offset=off, flavour=KINDS[kind], device=device)
        got, paths = _group(table, ["key"])
        assert got == want, (kind, off)
        assert paths[counter] >= 1 and paths["hashed_inserts"] == 0, paths
    if kind == "uuid":  # Histogram keeps NULL as a key: hashed records instead of UUID records
        got, paths = _group(H.hostile_table(spec, offset=61, flavour="high", device=device), ["key"], hist=True)
        assert got == _want(spec, ["key"], True)


@residency
def test_composite_region_records(gpu, monkeypatch, device):
    """(int64, utf8) -> hashed records, (int64, float64) -> 16-byte raw records, LDS aggregated."""
    for k, v in PATHS["partition"].items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("DQ_FREQ_PART_SLOTS", str(1 << 20))
    rng = np.random.default_rng(67)
    a = rng.integers(0, 40, N)
    spec = {"id": ["int64", _nulls(rng, [int(v) for v in a], 0.2)],
            "name": ["string", _nulls(rng, ["name-%05d" % (v % 7) for v in a], 0.2)],
            "x": ["float64", _nulls(rng, [float(v % 5) * 0.5 for v in a], 0.2)]}
    table = H.hostile_table(spec, offset={"id": 1, "name": 24, "x": 61}, flavour="digits", device=device)
    for cols, counter in ((["id", "name"], "hashed_runs"), (["id", "x"], "raw16_runs")):
        got, paths = _group(table, cols)
        assert got == _want(spec, cols), cols
        assert paths[counter] >= 1 and paths["hashed_inserts"] == 0, paths


@residency
def test_composite_keys_with_garbage_under_nulls(gpu, monkeypatch, device):
    """(int64, utf8) and (int64, float64): a NULL in either column drops the row, whatever
    INT64_MIN / NaN / "9.e-" its slot holds; on the partition path (hashed / 16-byte records) and
    the default one."""
    rng = np.random.default_rng(61)
    a = rng.integers(0, 40, N)
    spec = {"id": ["int64", _nulls(rng, [int(v) for v in a], 0.2)],
            "name": ["string", _nulls(rng, ["name-%05d" % (v % 7) for v in a], 0.2)],
            "x": ["float64", _nulls(rng, [float(v % 5) * 0.5 for v in a], 0.2)]}
    offsets = {"id": 1, "name": 24, "x": 61}
    for env in ({}, PATHS["partition"]):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        table = H.hostile_table(spec, offset=offsets, flavour="digits", device=device)
        for cols in (["id", "name"], ["id", "x"], ["name", "x"]):
            got, _ = _group(table, cols)
            assert got == _want(spec, cols), (cols, env)


@residency
@pytest.mark.parametrize("dtype", list(H.NUMERIC) + ["bool"])
def test_numeric_keys_of_every_dtype(gpu, monkeypatch, dtype, device):
    rng = np.random.default_rng(71)
    if dtype == "bool":
        vals = [bool(v) for v in rng.integers(0, 2, N)]
    elif dtype.startswith("float"):
        vals = [float(v) * 0.25 for v in rng.integers(-60, 60, N)]
    else:
        vals = [int(v) for v in rng.integers(-100, 100, N)]
    spec = {"key": [dtype, _nulls(rng, vals)]}
    want = _want(spec, ["key"])
    for env in ({}, PATHS["partition"]):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        for index, off in enumerate(H.OFFSETS[1:]):
            table = H.hostile_table(spec, offset=off, device=device)
            got, _ = _group(table, ["key"], few=300 if index % 2 else None)
            assert got == want, (dtype, off, env)


def test_kll_over_hostile_columns(gpu):
    """The KLL slab kernel over a float64 column at offsets 3 and 69 and an int64 column: NaN /
    Inf / INT64_MIN under the NULLs and around the window never reach the sketch."""
    rng = np.random.default_rng(81)
    n = 6151
    f = _nulls(rng, [float(v) for v in rng.normal(0.0, 1e4, n)], 0.1)
    i = _nulls(rng, [int(v) for v in rng.integers(-2 ** 40, 2 ** 40, n)], 0.1)
    for device in (True, False):
        for off_f, off_i in ((3, 8), (69, 1)):
            table = d.Table({"f": H.hostile_column("float64", f, offset=off_f, device=device),
                             "i": H.hostile_column("int64", i, offset=off_i, device=device)})
            for k, slab_rows in ((2, 37), (2048, 1000)):
                sk = kll.KLLSketcher(table.schema, [("f", k, 0.64), ("i", k, 0.64)], slab_rows)
                try:
                    sk.consume(table)
                    got_f, got_i = sk.finish()
                finally:
                    sk.close()
                assert got_f == kll_sketch_slabs(f, k, 0.64, slab_rows), (device, off_f, k)
                assert got_i == kll_sketch_slabs([None if v is None else float(v) for v in i], k, 0.64, slab_rows), \
                    (device, off_i, k)
