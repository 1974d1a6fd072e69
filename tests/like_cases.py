"""Shared by the LIKE / RLIKE tests (test_like.py, test_gpu_like.py): independent references, the
fixed case tables and the seeded generator.

References (oracle/pyoracle.py knows no pattern operator, so they are restated here):
* LIKE: `like_match`, a two-pointer wildcard matcher over Python code points.  No regex.
* RLIKE: `re.search(p, s, re.ASCII) is not None` -- Matcher.find(0): any match, an empty one
  included -- under pattern_cases.py's input discipline: random inputs hold no \\r, U+0085, U+2028
  or U+2029 (Java's other line terminators), which RLIKE_CASES covers by hand.
* a combined predicate: Kleene logic (`k_and`, `k_or`, `k_not`) over the matcher's verdict and the
  oracle's verdict of the other side."""
import json
import os
import re

import numpy as np

import pattern_cases as C

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# ---------------------------------------------------------------------------- references
def like_match(pattern, s):
    """SQL LIKE without escapes: `_` one code point, `%` any run of code points; the whole of s."""
    p, n, m = 0, len(pattern), len(s)
    i = 0
    star_p, star_i = -1, 0
    while i < m:
        if p < n and pattern[p] == "%":
            star_p, star_i = p, i
            p += 1
        elif p < n and (pattern[p] == "_" or pattern[p] == s[i]):
            p += 1
            i += 1
        elif star_p >= 0:  # let the last % take one more code point
            star_i += 1
            p, i = star_p + 1, star_i
        else:
            return False
    while p < n and pattern[p] == "%":
        p += 1
    return p == n


def rlike_match(pattern, s):
    return re.search(pattern, s, re.ASCII) is not None


def verdict(kind, pattern, s):
    """True / False / None (NULL value) of `s LIKE pattern` or `s RLIKE pattern`."""
    if s is None:
        return None
    return like_match(pattern, s) if kind == "like" else rlike_match(pattern, s)


def k_not(a):
    return None if a is None else not a


def k_and(a, b):
    if a is False or b is False:
        return False
    return None if a is None or b is None else True


def k_or(a, b):
    if a is True or b is True:
        return True
    return None if a is None or b is None else False


def sql_quote(pattern):
    """The pattern as a SQL literal in the only form the front end accepts: `\\` doubled, a quote
    through an adjacent literal of the other quote character."""
    assert "'" not in pattern
    return "'" + pattern.replace("\\", "\\\\") + "'"


# ---------------------------------------------------------------------------- fixed cases
# (pattern, text, expected): written out by hand, checked against like_match by test_like.py
LIKE_CASES = [
    ("", "", 1), ("", "a", 0), ("", "\n", 0),
    ("%", "", 1), ("%", "abc", 1), ("%", "a\nb\r\u2028", 1), ("%%", "", 1), ("%%", "é例😀", 1),
    ("_", "", 0), ("_", "a", 1), ("_", "é", 1), ("_", "例", 1), ("_", "😀", 1), ("_", "ab", 0), ("_", "\n", 1), ("_", "\r", 1),
    ("_", "éé", 0), ("__", "é例", 1), ("__", "😀", 0), ("___", "a😀例", 1),
    ("a%", "a", 1), ("a%", "abc", 1), ("a%", "ba", 0), ("a%", "", 0), ("a%", "a\n\n", 1), ("a%", "A", 0),
    ("%a", "a", 1), ("%a", "bca", 1), ("%a", "ab", 0), ("%a", "\r\na", 1), ("%a", "a\n", 0),
    ("%a%", "xay", 1), ("%a%", "xyz", 0), ("%a%", "\na\n", 1), ("%é%", "xéy", 1), ("%é%", "xèy", 0),
    ("a_c", "abc", 1), ("a_c", "a例c", 1), ("a_c", "a😀c", 1), ("a_c", "a\nc", 1), ("a_c", "a\rc", 1), ("a_c", "ac", 0),
    ("a_c", "abbc", 0), ("a_c", "abc\n", 0),
    ("a%b%c", "abc", 1), ("a%b%c", "aXbYc", 1), ("a%b%c", "a\nb\r\nc", 1), ("a%b%c", "acb", 0), ("a%b%c", "abcb", 0),
    ("a%b%c", "abcbc", 1),
    ("_%_", "", 0), ("_%_", "a", 0), ("_%_", "ab", 1), ("_%_", "é例", 1), ("_%_", "😀", 0), ("_%_", "a\n\nb", 1),
    ("abc", "abc", 1), ("abc", "abc\n", 0), ("abc", "abc\r\n", 0), ("abc", "xabc", 0), ("abc", "ab", 0),
    ("例%", "例子", 1), ("例%", "子例", 0), ("%😀", "a😀", 1), ("%😀", "😀a", 0), ("é_", "é例", 1), ("é_", "e例", 0),
    ("%ab%ab%", "abab", 1), ("%ab%ab%", "aba", 0), ("%aab", "aaab", 1), ("%aab", "aabaab", 1), ("%aab", "aaba", 0),
    ("a.c", "a.c", 1), ("a.c", "abc", 0), ("a*", "a*", 1), ("a*", "aaa", 0), ("(a|b)", "(a|b)", 1), ("^a$", "a", 0),
]

NULLABLE_REGEXES = [r"a*", r"\d*", r"(|a)", r"^$", r"^\d*$", r"x*$"]
# (regex, text, Java's Matcher.find(0)): the issue's examples, then `$` and `.` around Java's line
# terminators (Pattern.Dollar / Pattern.Dot of JDK 8, by hand)
RLIKE_CASES = [
    (r"a*", "", 1), (r"a*", "xyz", 1), (r"a*", "\r\u2028", 1), (r"\d*", "abc", 1), (r"(|a)", "q", 1),
    (r"^$", "", 1), (r"^$", "\n", 1), (r"^$", "a", 0), (r"^$", "\n\n", 0), (r"^$", "\r\n", 1), (r"^$", "\r", 1),
    (r"^$", "\u2028", 1), (r"^$", "\u0085", 1), (r"^$", "\n\r", 0),
    (r"^\d*$", "", 1), (r"^\d*$", "123", 1), (r"^\d*$", "123\n", 1), (r"^\d*$", "12a", 0), (r"^\d*$", "123\r\n", 1),
    (r"^\d*$", "123\n\n", 0), (r"^\d*$", "\n", 1),
    (r"x*$", "", 1), (r"x*$", "abc", 1), (r"x*$", "abc\n", 1),
    (r"a?", "b", 1), (r"(a|b*)", "zzz", 1), (r"x{0,3}", "", 1), (r"", "", 1), (r"", "abc", 1),
    (r"^a*$", "aaa", 1), (r"^a*$", "aab", 0), (r"^a*$", "aaa\u2029", 1), (r"^a*$", "aaa\u2027", 0),
    (r"^.*$", "ab", 1), (r"^.*$", "a\nb", 0), (r"^.*$", "a\rb", 0), (r"^.*$", "a\u2028b", 0), (r"^.*$", "ab\n", 1),
    (r"^.?$", "\r", 1), (r"^.$", "\r", 0), (r"^.$", "\u0085", 0), (r"^.$", "\u0084", 1), (r"^.$", "😀", 1),
    (r"keyword", "a keyword here", 1), (r"keyword", "keywor", 0),
] + [(p, s, w) for p, s, w in C.JAVA_LINE_CASES]

# regexes RLIKE must still decline (pattern_cases.MUST_REJECT minus the nullable ones)
RLIKE_MUST_REJECT = [p for p in C.MUST_REJECT if p not in
                     (r"a*", r"\d*", r"(|a)", r"^$", r"^\d*$", r"a?", r"(a|b*)", r"x{0,3}", r"")]


# ---------------------------------------------------------------------------- generator
_LITERALS = list("abcab01 .-") + ["é", "例", "😀", "\n", "\t", "A", "z", "q"]
_INSERTS = list("abc01 .-qZ") + ["é", "例", "😀", "➡", "\n", "\t"]


# six `_` after a `%`, 24 code points, several such segments: the largest DFAs the generator's
# rules allow
EXTREME_LIKE = ["%a______", "%a______%b______%c_____", "______%é______%", "%a_b_c_d_e_f_g%hijklmnop", "%ab_ab__ab___ab%ab_ab__a"]


def gen_like_pattern(rng):
    """A LIKE pattern of 1..24 code points: segments of literals and `_` joined by `%`, at most 6
    `_` in the segment after any `%`, no backslash, no quote."""
    n_seg = int(rng.integers(1, 5))
    budget = 24
    parts = []
    lead = rng.random() < 0.6
    trail = rng.random() < 0.6
    for k in range(n_seg):
        seg_len = int(rng.integers(0 if n_seg > 1 else 1, 7))
        seg, under = [], 0
        for _ in range(seg_len):
            if rng.random() < 0.3 and under < 6:
                seg.append("_")
                under += 1
            else:
                seg.append(_LITERALS[int(rng.integers(len(_LITERALS)))])
        parts.append("".join(seg))
    pattern = ("%" if lead else "") + "%".join(parts) + ("%" if trail else "")
    pattern = "".join(list(pattern)[:budget])
    return pattern or "%"


def like_instance(pattern, rng):
    """A string the pattern matches: `_` and `%` filled from the insert alphabet."""
    out = []
    for ch in pattern:
        if ch == "_":
            out.append(_INSERTS[int(rng.integers(len(_INSERTS)))])
        elif ch == "%":
            out += [_INSERTS[int(i)] for i in rng.integers(len(_INSERTS), size=int(rng.integers(0, 6)))]
        else:
            out.append(ch)
    return "".join(out)


def like_inputs(pattern, n, rng):
    """n strings: instances of the pattern under pattern_cases.make_strings' mutations."""
    seeds = [like_instance(pattern, rng) for _ in range(4)]
    return C.make_strings(seeds, n, rng)


def generated_like(seed, n_patterns, n_strings):
    """[(pattern, strings)], deterministic in the seed."""
    rng = np.random.default_rng(seed)
    out, seen = [], set()
    fixed = list(EXTREME_LIKE)  # the limits of the construction first
    while len(out) < n_patterns:
        p = fixed.pop(0) if fixed else gen_like_pattern(rng)
        if p in seen:
            continue
        seen.add(p)
        out.append((p, like_inputs(p, n_strings, rng)))
    return out


# the `other` side of the combined predicates, over the columns of combined_table()
OTHERS = ["n > 3", "n IS NULL", "n IN (1, 2, 5)", "x < 0.5", "COALESCE(n, 0) = 0", "t = 'abc'", "t IS NOT NULL",
          "n BETWEEN 2 AND 6", "NOT (x >= 0.25)", "n <=> 4"]


def combined_table(strings, seed):
    """{"s": strings with ~8 % NULLs, "n": int64, "x": float64, "t": string}, NULLs in each."""
    rng = np.random.default_rng(seed)
    n = len(strings)
    s = [None if rng.random() < 0.08 else v for v in strings]
    nn = [None if rng.random() < 0.15 else int(v) for v in rng.integers(0, 8, n)]
    x = [None if rng.random() < 0.15 else float(v) for v in rng.random(n)]
    t = [None if rng.random() < 0.15 else ("abc", "abd", "")[int(v)] for v in rng.integers(0, 3, n)]
    return {"s": ("string", s), "n": ("int64", nn), "x": ("float64", x), "t": ("string", t)}


def combine(form, left, right):
    """(SQL text, Kleene function) of form 0..3 over the pattern predicate `left` and `right`."""
    if form == 0:
        return "(%s) AND (%s)" % (left, right), k_and
    if form == 1:
        return "(%s) OR (%s)" % (left, right), k_or
    if form == 2:
        return "NOT (%s) OR (%s)" % (left, right), lambda a, b: k_or(k_not(a), b)
    return "NOT ((%s) AND (%s))" % (left, right), lambda a, b: k_not(k_and(a, b))


def known_answers():
    with open(os.path.join(GOLDEN, "like_known_answers.json"), encoding="utf-8") as f:
        return json.load(f)


def image_digests():
    with open(os.path.join(GOLDEN, "regex_image_digests.json"), encoding="utf-8") as f:
        return json.load(f)
