"""Distance (analyzers/Distance.scala:19-87): the L-infinity drift between two profiles.

* `categoricalDistance` -- the largest difference of two `{value: count}` maps' relative
  frequencies.  Two dicts are evaluated on the host, as the reference does; two device states
  (`FrequenciesAndNumRows`) through `dq_freq_linf_distance` (deequ_amd/csrc/dq_freq.hip,
  "Distance"): one table's slots probe the other in HBM and the host never sees a group.
* `numericalDistance` -- the largest difference of two KLL sketches' CDFs (host code: a sketch
  holds a few thousand items at most).

Both end in `select_metrics`, the reference's `selectMetrics` with its inverted flag name:
`correctForLowNumberOfSamples=True` returns the plain maximum, the default subtracts the
two-sample Kolmogorov-Smirnov term.
"""
from __future__ import annotations

import math
from typing import Dict, Tuple

from . import _lib as L
from .frequencies import FrequenciesAndNumRows, FrequencyTable
from .states import KLLState, QuantileNonSample

_NAN = float("nan")


def _java_math_max(a: float, b: float) -> float:
    """java.lang.Math.max for the values met here (no -0.0): a NaN on either side stays."""
    if a != a or b != b:
        return _NAN
    return a if a >= b else b


def _div(a: float, b: float) -> float:
    """Java's double division (a Long numerator is converted first): x / 0.0 is NaN or an
    infinity where Python raises."""
    a = float(a)
    if b == 0.0:
        return _NAN if a == 0.0 or a != a else math.copysign(float("inf"), a) * math.copysign(1.0, b)
    return a / b


def select_metrics(linfSimple: float, n: float, m: float, correctForLowNumberOfSamples: bool = False) -> float:
    """Distance.selectMetrics (Distance.scala:72-86), in fp64 in the reference's operation order."""
    if correctForLowNumberOfSamples:
        return linfSimple
    ratio = _div(n + m, n * m)
    root = math.sqrt(ratio) if ratio == ratio and ratio >= 0.0 else _NAN
    return _java_math_max(0.0, linfSimple - 1.8 * root)


def categorical_linf(sample1: Dict, sample2: Dict) -> Tuple[float, float, float]:
    """(linfSimple, n, m) of two {key: count} maps (Distance.scala:50-66)."""
    n = 0.0
    for c in sample1.values():
        n += c
    m = 0.0
    for c in sample2.values():
        m += c
    linf = 0.0
    for key in set(sample1) | set(sample2):
        diff = abs(_div(sample1.get(key, 0), n) - _div(sample2.get(key, 0), m))
        linf = _java_math_max(linf, diff)
    return linf, n, m


class Distance:
    """The reference's `Distance` object: static methods only."""

    @staticmethod
    def categoricalDistance(sample1, sample2, correctForLowNumberOfSamples: bool = False) -> float:
        s1, s2 = _is_state(sample1), _is_state(sample2)
        if s1 and s2:
            r = _state_distance(sample1, sample2)
            return select_metrics(r.linf_simple, float(r.n), float(r.m), correctForLowNumberOfSamples)
        if s1 or s2 or not isinstance(sample1, dict) or not isinstance(sample2, dict):
            raise TypeError("categoricalDistance takes two dicts or two FrequenciesAndNumRows, not %s and %s"
                            % (type(sample1).__name__, type(sample2).__name__))
        linf, n, m = categorical_linf(sample1, sample2)
        return select_metrics(linf, n, m, correctForLowNumberOfSamples)

    @staticmethod
    def numericalDistance(sample1, sample2, correctForLowNumberOfSamples: bool = False) -> float:
        if isinstance(sample1, KLLState) and isinstance(sample2, KLLState):
            sample1, sample2 = sample1.qSketch, sample2.qSketch
        if not isinstance(sample1, QuantileNonSample) or not isinstance(sample2, QuantileNonSample):
            raise TypeError("numericalDistance takes two QuantileNonSample or two KLLState, not %s and %s"
                            % (type(sample1).__name__, type(sample2).__name__))
        rankMap1, rankMap2 = sample1.getRankMap(), sample2.getRankMap()
        if not rankMap1 or not rankMap2:
            raise ValueError("numericalDistance of an empty sketch (the reference's max of an empty iterator throws)")
        n = float(max(rankMap1.values()))
        m = float(max(rankMap2.values()))
        linf = 0.0
        for key in list(rankMap1) + [k for k in rankMap2 if k not in rankMap1]:
            diff = abs(_div(sample1.getRank(key, rankMap1), n) - _div(sample2.getRank(key, rankMap2), m))
            linf = _java_math_max(linf, diff)
        return select_metrics(linf, n, m, correctForLowNumberOfSamples)


def _is_state(x) -> bool:
    return isinstance(x, FrequenciesAndNumRows) or (hasattr(x, "table") and hasattr(x, "numRows")
                                                    and not isinstance(x, dict))


def _state_distance(a, b) -> L.DqFreqDistance:
    for s in (a, b):
        if not isinstance(s, FrequenciesAndNumRows) or not isinstance(s.table, FrequencyTable):
            raise L.UnsupportedOnGpu(L.DQ_ERR_UNSUPPORTED,
                                     "categoricalDistance needs each state in one single-device FrequencyTable; "
                                     "%s holds a sharded run's per-owner tables" % type(s).__name__)
    if a.table.histogram and b.table.histogram and a.table.dtypes != b.table.dtypes:
        # (as FrequenciesAndNumRows.sum: a persisted Histogram state is keyed by strings)
        a, b = a.as_string_keys(), b.as_string_keys()
    if b.table.dtypes != a.table.dtypes or b.table.histogram != a.table.histogram:
        raise ValueError("frequency states over different key columns cannot be compared")
    return a.table.linf_distance(b.table)
