"""MutualInformation restated from MutualInformation.scala:38-81, independent of oracle/ and of
deequ_amd/analyzers.py: plain Python floats in the reference's operation order, the terms summed
exactly (math.fsum).  Used by the CPU and GPU tests of dq_freq_mutual_information."""
import math
from collections import namedtuple

Restated = namedtuple("Restated", "terms fsum sum_abs groups_a groups_b")


def _log(x: float) -> float:
    """java.lang.Math.log on what the terms can hand it: log(0.0) = -inf, log(NaN) = NaN."""
    if x != x:
        return float("nan")
    if x == 0.0:
        return float("-inf")
    return math.log(x)


def _div(a: float, b: float) -> float:
    """IEEE division (Python raises on a zero divisor)."""
    if b == 0.0:
        return float("nan") if a == 0.0 or a != a else math.copysign(float("inf"), a)
    return a / b


def restate(joint, num_rows: int) -> Restated:
    """joint = {(a, b): count}, a and b any hashable group identities (the tests use the encoded
    field bytes, the exact identity of a group).  A term that is not finite makes fsum NaN."""
    total = float(num_rows)
    ma, mb = {}, {}
    for (a, b), c in joint.items():
        ma[a] = ma.get(a, 0) + c
        mb[b] = mb.get(b, 0) + c
    terms = []
    for (a, b), c in joint.items():
        px, py, pxy = float(ma[a]), float(mb[b]), float(c)
        p = _div(pxy, total)
        terms.append(p * _log(_div(p, _div(px, total) * _div(py, total))))
    if all(math.isfinite(t) for t in terms):
        return Restated(terms, math.fsum(terms), math.fsum(abs(t) for t in terms), len(ma), len(mb))
    return Restated(terms, float("nan"), float("nan"), len(ma), len(mb))
