"""Distance.scala:43-87 restated with Python floats in the reference's operation order: the
oracle of tests/test_distance.py and tests/test_gpu_distance.py (independent of
deequ_amd/distance.py: it shares no code with it)."""
import math


def jdiv(a, b):
    """a / b as the JVM divides doubles (a Long numerator is converted first)."""
    try:
        return a / b
    except ZeroDivisionError:
        return math.nan if a == 0 or a != a else math.copysign(math.inf, a)


def jmax(a, b):
    """Math.max: a NaN stays."""
    if a != a or b != b:
        return math.nan
    return max(a, b)


def linf_simple(sample1, sample2):
    """(linfSimple, n, m) of two {key: count} maps (:50-66)."""
    n = 0.0
    for key in sample1:
        n += sample1[key]
    m = 0.0
    for key in sample2:
        m += sample2[key]
    linf = 0.0
    for key in set(sample1).union(sample2):
        cdf1 = jdiv(sample1.get(key, 0), n)
        cdf2 = jdiv(sample2.get(key, 0), m)
        linf = jmax(linf, abs(cdf1 - cdf2))
    return linf, n, m


def select(linf, n, m, correct_for_low_number_of_samples=False):
    """selectMetrics (:72-86), the inverted flag name included."""
    if correct_for_low_number_of_samples:
        return linf
    return jmax(0.0, linf - 1.8 * math.sqrt(jdiv(n + m, n * m)))


def categorical(sample1, sample2, correct_for_low_number_of_samples=False):
    return select(*linf_simple(sample1, sample2), correct_for_low_number_of_samples)


def same(a, b):
    """Bit-equal doubles, every NaN equal to every NaN."""
    return (a != a and b != b) or (a == b and math.copysign(1.0, a) == math.copysign(1.0, b))
