"""The fused scan over sliced columns in hostile buffers (tests/hostile.py) against the oracle.

Every branch of prepare_column with a non-zero Arrow offset -- device validity in place at a byte
address that is no multiple of 4 (offsets 8, 24, 64), realigned by the kernel (1, 7, 61, 2051),
fixed-width values in place or copied device to device depending on (width, offset), bool
bitmaps in place or realigned, and the host staging of the same bytes -- feeds
dq_scan_fast_kernel, dq_scan_values_kernel (the other widths, and DQ_SCAN_FAST=0), the where / mask
kernels, dq_scan_bits_kernel and dq_corr_kernel.  NULL slots hold NaN / +-Inf / +-1e300 /
INT_MIN / INT_MAX, rows outside the window are valid and hold the same, bitmap padding is set.

Bar (test_gpu_parity._check_state): bit-exact counts, Compliance, Min / Max, integral Sum, HLL
words; fp64 Sum / Mean / StdDev / Correlation within 1e-12 of the exact rational value.  States
that are exact also equal those of the same values in a benign product_table."""
import numpy as np
import pytest

import deequ_amd as d
import hostile as H
from helpers import oracle_table, product_table, random_table
from test_gpu_fast_scan import _suite
from test_gpu_parity import _check_state

pytestmark = pytest.mark.gpu

COLS = ["c_" + t for t in H.NUMERIC]
CORR = [("c_int64", "c_float64"), ("c_int32", "c_float32"), ("c_float64", "c_int8")]
WHERE = "w > 0"
_SPECS = {}


def _spec(n, null_frac):
    """{column: [dtype, values]}: one column per numeric dtype and a bool at `null_frac`, plus the
    filter column `w` (int32, 30 % NULL).  Made once per (n, null_frac), never modified."""
    key = (n, null_frac)
    if key not in _SPECS:
        rng = np.random.default_rng(4000 + n + int(null_frac * 10))
        spec = random_table(rng, n, null_frac, list(H.NUMERIC) + ["bool"])
        w = rng.integers(-5, 6, n).tolist()
        spec["w"] = ["int32", [None if rng.random() < 0.3 else v for v in w]]
        _SPECS[key] = (spec, oracle_table(spec))
    return _SPECS[key]


def _offsets(spec, index):
    return {name: H.OFFSETS[(index + j) % len(H.OFFSETS)] for j, name in enumerate(spec)}


def _analyzers(where=None):
    """test_gpu_fast_scan._suite of every numeric column (with `where`: the same analyzers,
    filtered), the bool column's bit tasks and the correlations."""
    out = []
    for c in COLS:
        if where is None:
            out += _suite(c, ["%s > 3" % c])
        else:
            out += [d.Size(where), d.Completeness(c, where), d.Sum(c, where), d.Mean(c, where),
                    d.StandardDeviation(c, where), d.Minimum(c, where), d.Maximum(c, where),
                    d.ApproxCountDistinct(c, where), d.Compliance("p0", "%s > 3" % c, where)]
    out += [d.Completeness("c_bool", where), d.Compliance("b", "c_bool", where),
            d.Compliance("nb", "NOT c_bool", where), d.ApproxCountDistinct("c_bool", where)]
    out += [d.Correlation(x, y, where) for x, y in CORR]
    return list(dict.fromkeys(out))


_INEXACT = (d.Sum, d.Mean, d.StandardDeviation, d.Correlation)


def _run_and_check(an, table, ot, benign=None):
    got = d.run_scan(an, table)
    for a in an:
        _check_state(a, got[a], ot)
        if benign is not None and not isinstance(a, _INEXACT):
            assert got[a] == benign[a], a
    return got


@pytest.mark.parametrize("device", [True, False], ids=["device", "host"])
@pytest.mark.parametrize("null_frac", [0.0, 0.3, 1.0])
@pytest.mark.parametrize("n,index", H.PAIRS)
def test_scan_suite_fast_general_and_where(gpu, monkeypatch, n, index, null_frac, device):
    spec, ot = _spec(n, null_frac)
    offsets = _offsets(spec, index)
    assert len(set(offsets.values())) == len(offsets)  # every column sliced differently
    table = H.hostile_table(spec, offset=offsets, device=device)
    for name in spec:
        assert table.columns[name].offset == offsets[name] and table.columns[name].validity is not None
    plain, filtered = _analyzers(), _analyzers(WHERE)
    benign = d.run_scan(plain, product_table(spec))
    _run_and_check(plain, table, ot, benign)          # int64 / fp64 tasks: dq_scan_fast_kernel
    _run_and_check(filtered, table, ot)                # `where` on a column sliced elsewhere
    monkeypatch.setenv("DQ_SCAN_FAST", "0")            # every task through dq_scan_values_kernel
    monkeypatch.setenv("DEEQU_AMD_PLAN_CACHE", "0")    # (a pooled plan keeps its kernels)
    _run_and_check(plain, table, ot, benign)


@pytest.mark.parametrize("device", [True, False], ids=["device", "host"])
@pytest.mark.parametrize("dtype", ["int64", "float64"])
def test_fast_scan_alone_with_one_predicate(gpu, dtype, device):
    """The headline shape (one 8-byte column, one inline predicate, no other task) at every
    (n, offset) pair: NULL rows take the wave's stand-in value, never the NaN / INT_MIN under them."""
    col = "c_" + dtype
    for n, index in H.PAIRS:
        for null_frac in (0.3, 1.0):
            spec, ot = _spec(n, null_frac)
            offset = H.OFFSETS[index]
            table = H.hostile_table({col: spec[col]}, offset=offset, device=device)
            an = _suite(col, ["%s >= 0" % col])
            _run_and_check(an, table, oracle_table({col: spec[col]}))


@pytest.mark.parametrize("device", [True, False], ids=["device", "host"])
def test_two_hostile_batches(gpu, device):
    """PartitionedTable of two hostile batches sliced differently: the states of the union."""
    (a, _), (b, _) = _spec(2049, 0.3), _spec(65, 0.3)
    union = {k: [a[k][0], a[k][1] + b[k][1]] for k in a}
    parts = d.PartitionedTable([H.hostile_table(a, offset=_offsets(a, 2), device=device),
                                H.hostile_table(b, offset=_offsets(b, 7), device=device)])
    ot = oracle_table(union)
    benign = d.run_scan(_analyzers(), product_table(union))
    _run_and_check(_analyzers(), parts, ot, benign)
    _run_and_check(_analyzers(WHERE), parts, ot)
