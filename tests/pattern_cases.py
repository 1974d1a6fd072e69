"""Shared by the PatternMatch tests (test_pattern_match.py, test_gpu_pattern_match.py): the fixed
pattern list, seeded inputs made by mutating strings that match, and the independent oracle.

The oracle is Python's `re.search(p, s, re.ASCII)` with a non-empty group 0.  For the supported
subset it answers as java.util.regex does, except around \\r, U+0085, U+2028 and U+2029 (Java's
line terminators for `.` and `$`): those characters stay out of the random inputs and are covered
by JAVA_LINE_CASES, whose expected values follow JDK 8's Pattern.Dollar / Pattern.Dot by hand."""
import json
import os
import re

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def known_answers():
    with open(os.path.join(GOLDEN, "pattern_match_known_answers.json"), encoding="utf-8") as f:
        return json.load(f)


def _fixture_pattern(case_id):
    return next(c["pattern"] for c in known_answers()["cases"] if c["id"] == case_id)


EMAIL = _fixture_pattern("pattern_email")
URL = _fixture_pattern("pattern_url")
CREDITCARD = _fixture_pattern("pattern_creditcard")
SSN = _fixture_pattern("pattern_ssn")
UUID = r"[0-9a-f]{8}-[0-9a-f]{4}-[0-9a-f]{4}-[0-9a-f]{4}-[0-9a-f]{12}"

# (pattern, strings that match it): every construct of the supported subset
PATTERNS = [
    (r"foo", ["xfoox", "foo"]),
    (r"a\.b\*c\\d", ["a.b*c\\d", "zza.b*c\\dzz"]),
    (r"x\ty|u\nv|p\fq", ["x\ty", "u\nv", "p\fq"]),
    (r"\x41é\x7e", ["Aé~", "..Aé~"]),
    (r"\u00e9[\u4e00-\u9fff]+|\u0041\u007a", ["é例子", "xé测试y", "Az"]),   # \uhhhh outside and inside a class
    (r"a\r?b|x[\r\n]y|[^\r]\t", ["ab", "x\ny", "q\t"]),                        # the \r escape (inputs hold no \r)
    (r"a.c", ["abc", "a例c", "a\U0001F600c"]),
    (r"[abc]x[^a-c]z", ["axdz", "cxéz", "bx例z"]),
    (r"[a-f0-9]{4}-[^\s-]", ["beef-x", "12ab-➡"]),
    (r"\d+\.\d+", ["3.14", "x10.5y"]),
    (r"\D\d\s\S", ["a1 b", "é7\tq"]),
    (r"\w+@\W", ["ab_1@!", "x@é"]),
    (r"[\d\s]{3}[^\w]", ["1 2!", "  7é"]),
    (r"[\W\d]q[+*?.$^(|){-]", ["!q+", "7q{", "éq-", "1q$"]),
    (r"(ab)+c", ["abc", "ababababc"]),
    (r"(?:ab|cd)e(f|g(h|i))", ["abef", "cdegh", "xcdegi"]),
    (r"cat|dog|bird", ["cat", "hotdog", "birds"]),
    (r"ab?c", ["ac", "abc"]),
    (r"ab*c", ["ac", "abbbbc"]),
    (r"ab+c", ["abc", "abbbc"]),
    (r"a{3}b", ["aaab", "xaaaab"]),
    (r"a{2,}b", ["aab", "aaaaaab"]),
    (r"a{2,4}b", ["aab", "aaaab"]),
    (r"a+?b|c*?d|e??f|g{2,3}?h", ["aab", "ccd", "ef", "f", "ggh"]),
    (r"^abc", ["abc", "abcdef"]),
    (r"abc$", ["abc", "xxabc", "abc\n"]),
    (r"^\d+$", ["12345", "7", "42\n"]),
    (r"^ab|cd$", ["abx", "xcd", "cd\n"]),
    (r"é+x|例子", ["ééx", "例子.测试"]),
    (r"[^\s]例|[à-ÿ]{2}", ["q例", "éè"]),
    (r"\d{3}-\d{2}-\d{4}", ["111-05-1130", "id 078-05-1120."]),
    (UUID, ["123e4567-e89b-12d3-a456-426614174000"]),
    (r"^" + UUID + r"$", ["123e4567-e89b-12d3-a456-426614174000", "00000000-0000-0000-0000-000000000000\n"]),
    (EMAIL, ["someone@somewhere.org", "a.b-c+d@x-y.example.co", "\"quoted.name\"@host.io", "u@[192.168.0.1]"]),
    (URL, ["http://foo.com/blah_blah", "https://foo_bar.example.com/", "ftp://➡.ws/䨹",
           "http://例子.测试"]),
]

# patterns the compiler must decline (DQ_ERR_UNSUPPORTED), by what they use
MUST_REJECT = [
    r"(a)\1", r"(?<n>a)\k<n>",                          # back-references
    r"(?=a)b", r"(?!a)b", r"(?<=a)b", r"(?<!a)b",       # look-around
    r"\bx", r"x\B", r"\Ax", r"x\z", r"x\Z", r"\Gx",     # boundary matchers
    r"a*+b", r"a++b", r"a?+b", r"a{2}+b",               # possessive quantifiers
    r"(?>a)b",                                          # atomic group
    r"(?i)a", r"(?s:a)", r"(?x) a",                     # inline flags
    r"(?<name>a)",                                      # named group
    r"\p{L}", r"\P{Lu}x", r"\p{Alpha}",                 # property classes
    r"\hx", r"\vx", r"\R", r"\X",
    r"[a-z&&[^b]]", r"[a[b]]",                          # class intersection / nesting
    r"a*", r"\d*", r"(|a)", r"^$", r"^\d*$", r"a?", r"(a|b*)", r"x{0,3}", r"",  # can match ""
    r"a^b", r"a$b", r"(^a)", r"(a$)",                   # anchors off the pattern's edges
    CREDITCARD, SSN,
]
STATE_CAP_PATTERN = r"(a|b)*a(a|b){14}"  # >= 32768 DFA states

# (pattern, input, Java's answer): the line-terminator rules Python's re does not share
JAVA_LINE_CASES = [
    (r"b\r$", "b\r\n", 0),       # $ never holds between \r and \n
    (r"b$", "b\r\n", 1),         # ... but before a final \r\n
    (r"b$", "b\n", 1), (r"b$", "b\r", 1), (r"b$", "b\u0085", 1), (r"b$", "b\u2028", 1), (r"b$", "b\u2029", 1),
    (r"b$", "b", 1), (r"b$", "b\n\n", 0), (r"b$", "b\n\r", 0), (r"b$", "b\r\r", 0), (r"b$", "b\u2028\n", 0),
    (r"b$", "b\u2027", 0), (r"b$", "b\u0084", 0), (r"b$", "bx", 0), (r"b$", "b\u202a", 0),
    (r"b\n$", "b\n\n", 1), (r"b\r?$", "b\r\n", 1), (r"\r$", "\r\n", 0), (r"\r$", "\r\r", 1), (r"a\r$", "a\r", 1),
    (r"^b$", "b\u2029", 1), (r"^b$|^c", "b\r\n", 1), (r"^b$", "b\r\nx", 0),
    (r"a.c", "a\rc", 0), (r"a.c", "a\nc", 0), (r"a.c", "a\u0085c", 0), (r"a.c", "a\u2028c", 0),
    (r"a.c", "a\u2029c", 0), (r"a.c", "a\u2027c", 1), (r"a.c", "a\u0084c", 1), (r"a.c", "a\u0086c", 1),
    (r"a.c", "a\u202ac", 1), (r"a.c", "a\U0001F600c", 1), (r"a..c", "a\U0001F600c", 0),
    (r"a[^x]c", "a\rc", 1), (r"a[^x]c", "a\u2028c", 1), (r"a\sc", "a\rc", 1), (r"a\Sc", "a\u0085c", 1),
]

_EXTRA = ["é", "例", "\U0001F600", "➡", " ", "\n", "\t", "-", ".", "@", "/", ":", "_", "a", "b", "0", "9", "Z"]


def oracle(pattern, s):
    m = re.search(pattern, s, re.ASCII)
    return 1 if (m is not None and m.group(0) != "") else 0


def make_strings(seeds, n, rng):
    """n strings of 0..70 characters: the seeds under 0..5 random edits (substitute, delete, insert,
    duplicate a slice, truncate), with multi-byte characters among the inserted ones."""
    alphabet = sorted(set("".join(seeds))) + _EXTRA
    out = []
    for k in range(n):
        s = list(seeds[int(rng.integers(len(seeds)))])
        if rng.random() < 0.35:  # padded with unrelated text
            pad = [alphabet[int(i)] for i in rng.integers(len(alphabet), size=int(rng.integers(0, 20)))]
            s = pad + s if rng.random() < 0.5 else s + pad
        for _ in range(int(rng.integers(0, 6))):
            op = int(rng.integers(5))
            i = int(rng.integers(len(s) + 1))
            c = alphabet[int(rng.integers(len(alphabet)))]
            if op == 0 and s:
                s[min(i, len(s) - 1)] = c
            elif op == 1 and s:
                del s[min(i, len(s) - 1)]
            elif op == 2:
                s.insert(i, c)
            elif op == 3 and s:
                j = int(rng.integers(i, len(s) + 1))
                s[i:i] = s[i:j]
            elif op == 4 and rng.random() < 0.3:
                s = s[:i]
        out.append("".join(s)[:70])
    out[0] = ""  # lengths 0 .. 70
    out[1] = (seeds[0] * 70)[:70]
    return out


def pattern_inputs(index, n=3000):
    pattern, seeds = PATTERNS[index]
    return pattern, make_strings(seeds, n, np.random.default_rng(1000 + index))
