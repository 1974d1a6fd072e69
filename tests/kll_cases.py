"""Shared by test_kll.py and test_gpu_kll.py: the reference's known answers
(tests/golden/kll_known_answers.json), seeded inputs, and the two CPU implementations of the
library's KLL layout -- the Python mirror (deequ_amd.states) and the C++ host sketch
(dq_diag_kll_sketch)."""
import ctypes
import json
import os

import numpy as np

import deequ_amd as d
from deequ_amd import _lib as L
from deequ_amd.states import KLLState, kll_sketch_slabs

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kll_known_answers.json")))
PROFILES = GOLDEN["profiles"]

_INPUTS = {}


def seeded(n=300_000, seed=20240607, null_frac=0.05):
    """(float64 values, validity) with ~5 % NULLs: computed once, shared, never modified."""
    key = (n, seed, null_frac)
    if key not in _INPUTS:
        rng = np.random.default_rng(seed)
        vals = rng.normal(0.0, 1e4, n)
        valid = rng.random(n) >= null_frac
        vals.setflags(write=False)
        valid.setflags(write=False)
        _INPUTS[key] = (vals, valid)
    return _INPUTS[key]


def pylist(vals, valid=None):
    """Rows as Python floats, None for NULL (the mirror's input)."""
    vals = np.asarray(vals)
    out = vals.astype(np.float64).tolist()
    if valid is not None:
        out = [v if ok else None for v, ok in zip(out, np.asarray(valid).tolist())]
    return out


def host_sketch(vals, valid, k, c, slab_rows) -> KLLState:
    """dq_diag_kll_sketch: the C++ host sketch over the slab-and-tree layout."""
    vals = np.ascontiguousarray(vals, dtype=np.float64)
    v = None if valid is None else np.ascontiguousarray(valid, dtype=np.uint8)
    need = ctypes.c_int64()
    lib = L.lib()
    st = lib.dq_diag_kll_sketch(vals.ctypes.data, None if v is None else v.ctypes.data, len(vals), k, c, slab_rows,
                                None, 0, ctypes.byref(need))
    assert st == L.DQ_ERR_SPACE, lib.dq_last_error()
    buf = ctypes.create_string_buffer(need.value)
    L.check(lib.dq_diag_kll_sketch(vals.ctypes.data, None if v is None else v.ctypes.data, len(vals), k, c, slab_rows,
                                   buf, need.value, ctypes.byref(need)))
    return KLLState.from_export(buf.raw[:need.value], k, c)


def mirror_sketch(vals, valid, k, c, slab_rows) -> KLLState:
    return kll_sketch_slabs(pylist(vals, valid), k, c, slab_rows)


def buckets_of(metric):
    return [[b.lowValue, b.highValue, b.count] for b in metric.value.get().buckets]


def dist_bits(metric):
    """A BucketDistribution bit for bit (NaN bounds, which `==` never equates, included)."""
    import struct
    dist = metric.value.get()
    return ([(struct.pack("<dd", b.lowValue, b.highValue), b.count) for b in dist.buckets], dist.parameters,
            [struct.pack("<%dd" % len(level), *level) for level in dist.data])


def known_table(case):
    return d.Table.from_pydict({case["column"]: (case["dtype"], case["values"])})
