"""CPU tests of MutualInformation's shared source (deequ_amd/csrc/dq_mi.h, the code the kernels
behind dq_freq_mutual_information run on the device), through its host build dq_diag_mi_*:

  * the split of a joint key into its two fields against the Python key codec (encode_key /
    decode_key), over every pair of key types and the inline / heap boundary lengths, and the
    refusal of every malformed key without a read past its length;
  * the fixed-point conversions against Python's exact integers and rationals: to_fixed is
    round-half-even(|t| 2^96) with t's sign, from_fixed the nearest double of v / 2^96, and a sum of
    fixed-point terms converted back is the correctly rounded exact sum.
No GPU is touched."""
import ctypes
import itertools
import math
import random
import struct
from fractions import Fraction

import pytest

from deequ_amd import _lib as L
from deequ_amd.frequencies import decode_key, encode_key

import mi_restated

TYPES = ["bool", "int8", "int16", "int32", "int64", "float32", "float64", "string"]
STRING_LENGTHS = [0, 1, 15, 16, 17, 40]
SAMPLE = {"bool": [True, False], "int8": [-128, 7], "int16": [-2, 32767], "int32": [-(2 ** 31), 65536],
          "int64": [-(2 ** 63), 0x0102030405060708], "float32": [1.5, -0.0], "float64": [-2.5e300, 0.0]}
ONE = 1 << 96


def _values(t):
    if t == "string":
        return ["".join(chr(ord("a") + (i * 7 + n) % 26) for i in range(n)) for n in STRING_LENGTHS]
    return SAMPLE[t]


def _split(key: bytes, ta: str, tb: str, pad: bytes = b""):
    """dq_diag_mi_split on key (followed in memory by `pad`, which it must not read)."""
    out = (ctypes.c_int32 * 4)(-1, -1, -1, -1)
    st = L.lib().dq_diag_mi_split(key + pad, len(key), L.TYPE_CODES[ta], L.TYPE_CODES[tb], out)
    return st, tuple(out)


def _single(v, t) -> bytes:
    return encode_key((v,), (t,))


def test_struct_layout_and_symbols():
    assert ctypes.sizeof(L.DqFreqMi) == 40
    assert [f[0] for f in L.DqFreqMi._fields_] == ["mi", "num_rows", "groups", "groups_a", "groups_b"]
    assert L.DqFreqMi.mi.offset == 0 and L.DqFreqMi.groups_b.offset == 32
    lib = L.lib()
    for name in ("dq_freq_mutual_information", "dq_diag_mi_split", "dq_diag_mi_to_fixed", "dq_diag_mi_from_fixed"):
        assert hasattr(lib, name), name


@pytest.mark.parametrize("ta,tb", list(itertools.product(TYPES, TYPES)))
def test_split_agrees_with_the_key_codec(ta, tb):
    """Each field's bytes are the single-column encoding of the value decode_key gives."""
    joint_lengths = set()
    for va, vb in itertools.product(_values(ta), _values(tb)):
        key = encode_key((va, vb), (ta, tb))
        joint_lengths.add(len(key))
        st, (oa, la, ob, lb) = _split(key, ta, tb, pad=b"\xff" * 8)
        assert st == L.DQ_OK, (ta, tb, va, vb)
        da, db = decode_key(key, (ta, tb))
        assert key[oa:oa + la] == _single(da, ta) == _single(va, ta)
        assert key[ob:ob + lb] == _single(db, tb) == _single(vb, tb)
        assert oa == (4 if ta == "string" else 0) and ob == oa + la + (4 if tb == "string" else 0)
        assert ob + lb == len(key)
    if ta == "string" and tb == "string":
        assert {8, 9, 23, 24, 25}.issubset(joint_lengths)


def test_split_joint_keys_of_16_and_17_bytes():
    """The joint key's own inline / heap boundary, reached from both sides."""
    cases = [(("int64", "int64"), (1, -1), 16), (("int64", "string"), (5, "abcd"), 16), (("int64", "string"), (5, "abcde"), 17),
             (("string", "string"), ("abcd", "efgh"), 16), (("string", "string"), ("abcd", "efghi"), 17),
             (("string", "int8"), ("elevenbytes", 3), 16), (("string", "int8"), ("twelve-bytes", 3), 17),
             (("float64", "float64"), (float("nan"), -0.0), 16), (("int8", "string"), (-1, "elevenbytes"), 16),
             (("int8", "string"), (-1, "twelve-bytes"), 17)]
    for dtypes, values, size in cases:
        key = encode_key(values, dtypes)
        assert len(key) == size
        st, (oa, la, ob, lb) = _split(key, *dtypes)
        assert st == L.DQ_OK
        assert key[oa:oa + la] == _single(values[0], dtypes[0]) and key[ob:ob + lb] == _single(values[1], dtypes[1])


def test_split_refuses_malformed_keys_without_reading_past_them():
    """A length prefix running past the key, a truncated prefix or fixed field, bytes left over, a
    type that is no key type: DQ_ERR_INVALID.  The bytes after the key hold a length that would
    make the key well formed if they were read."""
    good = encode_key(("abc", 7), ("string", "int32"))
    assert _split(good, "string", "int32")[0] == L.DQ_OK
    for cut in range(len(good)):  # every proper prefix, followed in memory by the rest of the key
        st, out = _split(good[:cut], "string", "int32", pad=good[cut:])
        assert st == L.DQ_ERR_INVALID and out == (-1, -1, -1, -1), cut
    assert _split(good + b"\x00", "string", "int32")[0] == L.DQ_ERR_INVALID  # a byte left over
    long_len = struct.pack("<I", 0xFFFFFFFF) + b"abc" + struct.pack("<i", 7)
    assert _split(long_len, "string", "int32")[0] == L.DQ_ERR_INVALID  # no u32 wrap-around
    two = encode_key(("ab", "cd"), ("string", "string"))
    for cut in range(len(two)):
        assert _split(two[:cut], "string", "string", pad=two[cut:])[0] == L.DQ_ERR_INVALID, cut
    bad_second = struct.pack("<I", 2) + b"ab" + struct.pack("<I", 3) + b"cd"
    assert _split(bad_second, "string", "string", pad=b"e")[0] == L.DQ_ERR_INVALID
    for t in ("int64", "float64", "int16", "bool"):
        key = encode_key((1, 1), (t, t))
        assert _split(key[:-1], t, t, pad=key[-1:])[0] == L.DQ_ERR_INVALID
        assert _split(key + b"\x01", t, t)[0] == L.DQ_ERR_INVALID
    assert _split(b"", "int8", "int8")[0] == L.DQ_ERR_INVALID
    out = (ctypes.c_int32 * 4)()
    for code in (0, 9, 99, -1):  # decimal128 and unknown types are no group key types
        assert L.lib().dq_diag_mi_split(b"\x00" * 16, 16, code, L.TYPE_CODES["int64"], out) == L.DQ_ERR_INVALID
    assert L.lib().dq_diag_mi_split(None, 4, 4, 4, out) == L.DQ_ERR_INVALID
    assert L.lib().dq_diag_mi_split(b"", 0, 8, 8, out) == L.DQ_ERR_INVALID
    st, got = _split(struct.pack("<II", 0, 0), "string", "string")  # two empty strings
    assert st == L.DQ_OK and got == (4, 0, 8, 0)


# ---------------------------------------------------------------- fixed point
def _to_fixed(t: float):
    lo, hi = ctypes.c_uint64(), ctypes.c_int64()
    st = L.lib().dq_diag_mi_to_fixed(t, ctypes.byref(lo), ctypes.byref(hi))
    return st, (hi.value << 64) | lo.value  # hi is signed: the two's-complement value


def _from_fixed(v: int) -> float:
    w = v & ((1 << 128) - 1)
    hi = w >> 64
    out = ctypes.c_double()
    L.check(L.lib().dq_diag_mi_from_fixed(w & 0xFFFFFFFFFFFFFFFF, hi - (1 << 64) if hi >> 63 else hi, ctypes.byref(out)))
    return out.value


def _exact_fixed(t: float) -> int:
    """round-half-even(|t| 2^96) with t's sign (Python's round on a Fraction is half-even)."""
    mag = round(abs(Fraction(t)) * ONE)
    return -mag if t < 0 else mag


def _bits(x: float) -> int:
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def _terms():
    rng = random.Random(20261020)
    edge = [0.0, -0.0, 2.0 ** -97, -2.0 ** -97, 2.0 ** -96, -2.0 ** -96, 1.0, -1.0, math.log(2.0 ** 63), -math.log(2.0 ** 63),
            3 * 2.0 ** -97, -3 * 2.0 ** -97, 2.0 ** -98, 2.0 ** -97 * (1 + 2.0 ** -52), 2.0 ** -96 * (1.5), 2.0 ** -96 * 2.5,
            5e-324, -5e-324, 2.2250738585072014e-308, 2.2250738585072009e-308, math.nextafter(64.0, 0.0),
            -math.nextafter(64.0, 0.0), 2.0 ** -44 + 2.0 ** -96, 2.0 ** -45 + 2.0 ** -97, 2.0 ** -45 + 3 * 2.0 ** -97]
    rand = [rng.uniform(-44.0, 44.0) for _ in range(10_000)]
    small = [rng.uniform(-1.0, 1.0) * 2.0 ** -rng.randrange(30, 110) for _ in range(2_000)]
    return edge, rand, small


def test_to_fixed_is_exact():
    edge, rand, small = _terms()
    assert abs(math.log(2.0 ** 63) - 43.66827237527655) < 1e-12
    for t in edge + rand + small:
        st, v = _to_fixed(t)
        assert st == L.DQ_OK and v == _exact_fixed(t), (t, v, _exact_fixed(t))
    assert _to_fixed(2.0 ** -97)[1] == 0 and _to_fixed(3 * 2.0 ** -97)[1] == 2  # ties go to even
    assert _to_fixed(-(2.0 ** -96))[1] == -1 and _to_fixed(1.0)[1] == ONE and _to_fixed(-1.0)[1] == -ONE
    assert _to_fixed(5e-324)[1] == 0 and _to_fixed(-0.0)[1] == 0
    for t in (64.0, -64.0, 1e300, float("inf"), float("-inf"), float("nan")):
        assert _to_fixed(t)[0] == L.DQ_ERR_INVALID


def test_from_fixed_is_correctly_rounded():
    rng = random.Random(7)
    values = [0, 1, -1, ONE, -ONE, (1 << 53) + 1, (1 << 54) + 2, (1 << 54) + 6, -((1 << 54) + 2), (1 << 127) - 1,
              -(1 << 127), (1 << 102) - 1, ((1 << 53) - 1) << 40 | (1 << 39), (1 << 100) + (1 << 47), (1 << 100) + 3 * (1 << 47)]
    values += [rng.randrange(-(1 << 127), 1 << 127) >> rng.randrange(0, 127) for _ in range(10_000)]
    for v in values:
        got, want = _from_fixed(v), float(Fraction(v, ONE))
        assert _bits(got) == _bits(want), (v, got, want)
    edge, rand, small = _terms()
    for t in edge + rand:  # what to_fixed keeps comes back: exact down to 2^-96
        st, v = _to_fixed(t)
        assert _from_fixed(v) == float(Fraction(_exact_fixed(t), ONE))
        if abs(t) >= 2.0 ** -44:
            assert _from_fixed(v) == t


def test_sum_of_fixed_terms_is_the_rounded_exact_sum():
    """10^4 terms: the integer sum of their fixed-point values, converted once, is the correctly
    rounded sum of the rounded terms -- and within groups * 2^-97 of fsum of the terms."""
    _, rand, _ = _terms()
    rng = random.Random(11)
    terms = [t / 10_000 * rng.choice([1.0, 2.0 ** -20, 2.0 ** -50]) for t in rand]
    fixed = [_to_fixed(t)[1] for t in terms]
    total = sum(fixed)
    assert _bits(_from_fixed(total)) == _bits(float(Fraction(total, ONE)))
    shuffled = fixed[:]
    rng.shuffle(shuffled)
    assert sum(shuffled) == total
    exact = sum(Fraction(t) for t in terms)
    assert abs(Fraction(total, ONE) - exact) <= Fraction(len(terms), 1 << 97)


def test_restatement_known_answers():
    """The restatement itself on cases with closed forms."""
    indep = {(a, b): ca * cb for a, ca in zip("xyz", [1, 3, 4]) for b, cb in zip("uvw", [2, 6, 8])}
    r = mi_restated.restate(indep, 128)
    assert r.fsum == 0.0 and r.terms == [0.0] * 9 and (r.groups_a, r.groups_b) == (3, 3)
    same = {(i, i): 1 for i in range(4)}
    r = mi_restated.restate(same, 4)
    assert abs(r.fsum - math.log(4.0)) < 1e-15 and (r.groups_a, r.groups_b) == (4, 4)
    r = mi_restated.restate({(0, 0): 0, (1, 1): 2}, 2)
    assert math.isnan(r.fsum)
