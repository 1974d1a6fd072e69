"""Generated regular expressions, host engine against oracle (no GPU).

Every pattern of regex_gen.generate over SEEDS is compiled and walked by the host build of the
engine (dq_diag_regex_match: the compiler plan creation runs, the walker the kernels run) on the
strings regex_gen.strings samples from the pattern's own AST, and compared with
pattern_cases.oracle string by string.  The compiler may decline a pattern only for a construction
bound; the caps below keep the test from passing by leaving cases out.  The metamorphic test needs
no oracle: three rewrites that keep a pattern's language must answer every string as the pattern
does.  test_gpu_regex_generated.py runs a subset of these cases through both kernels.
"""
import functools

import pytest

from deequ_amd import _lib as L

import pattern_cases as C
import regex_gen as G
from test_pattern_match import regex_match

SEEDS = [3101, 3102, 3103, 3104, 3105, 3106, 3107, 3108]
PER_SEED = 250
MAX_DECLINED = 0.15          # share of the patterns a construction bound may decline
MIN_BALANCED = 0.85          # share of the accepted patterns whose oracle match rate is in [0.1, 0.9]
MIN_ABOVE_16K, MIN_ABOVE_40K = 50, 1
BOUNDS = ("more than 2048 states", "LDS budget", "NFA nodes")   # the declines the compiler may give
REWRITES = {"lazy<->greedy": {"flip_lazy": True}, "(?:..)": {"noncapturing": True}, "\\uhhhh classes": {"uclass": True}}


class Case:
    """One generated pattern: its AST, text, strings, the oracle's answers and the compiler's verdict."""

    def __init__(self, seed, index, pattern):
        self.seed, self.index, self.pattern = seed, index, pattern
        self.text = pattern.text()
        self.status, _, n_states, n_cols, self.message = regex_match(self.text, "")
        self.table_bytes = 2 * n_states * n_cols if self.status == L.DQ_OK else 0

    @functools.cached_property
    def strings(self):
        return G.strings(self.pattern, self.seed * 100000 + self.index)

    @functools.cached_property
    def want(self):
        return [C.oracle(self.text, s) for s in self.strings]

    @property
    def accepted(self):
        return self.status == L.DQ_OK

    @property
    def rate(self):
        return sum(self.want) / len(self.want)


@functools.lru_cache(maxsize=None)
def cases(seed):
    """The seed's cases, computed once per session and shared (the GPU tests read them too)."""
    return tuple(Case(seed, k, p) for k, p in enumerate(G.generate(seed, PER_SEED)))


def all_cases():
    return [c for seed in SEEDS for c in cases(seed)]


def test_generator_is_deterministic_and_keeps_its_rules():
    a, b = G.generate(SEEDS[0], 40), G.generate(SEEDS[0], 40)
    assert [p.text() for p in a] == [p.text() for p in b]
    assert [G.strings(p, 7) for p in a] == [G.strings(p, 7) for p in b]
    assert [p.text() for p in a] != [p.text() for p in G.generate(SEEDS[1], 40)]
    seen = set()
    for c in all_cases():
        assert G.paths(c.pattern) <= G.MAX_PATHS
        assert all(len(s) <= G.MAX_CHARS for s in c.strings) and 35 <= len(c.strings) <= 45
        assert not any(ch in c.text or any(ch in s for s in c.strings) for ch in G.BANNED), c.text
        assert "" in c.strings and "\n" in c.strings
        seen.update(len(ch.encode("utf-8")) for s in c.strings for ch in s)
    assert seen == {1, 2, 3, 4}   # multi-byte characters of every length
    texts = [c.text for c in all_cases()]
    assert len(texts) >= 2000 and len(set(texts)) > 0.95 * len(texts)
    # every construct of the subset occurs somewhere
    joined = "\n".join(texts)
    for piece in ("\\t", "\\n", "\\f", "\\x", "\\u", "\\.", ".", "\\d", "\\s", "\\w", "\\D", "\\S", "\\W", "[^", "à-ÿ", "一-鿿",
                  "\\-", "(?:", "((", "|", "?", "*", "+", "{2}", "{2,}", "{2,3}", "??", "*?", "+?", "}?", "^", "$"):
        assert piece in joined, piece


@pytest.mark.parametrize("seed", SEEDS)
def test_engine_equals_oracle(seed):
    bad, wrongly_declined = [], []
    for c in cases(seed):
        if not c.accepted:
            if c.status != L.DQ_ERR_UNSUPPORTED or not any(b in c.message for b in BOUNDS):
                wrongly_declined.append((c.text, c.status, c.message))
            continue
        for s, w in zip(c.strings, c.want):
            st, got, _, _, msg = regex_match(c.text, s)
            assert st == L.DQ_OK, (c.text, msg)
            if got != w:
                bad.append("pattern %r on %r: engine %d, oracle %d" % (c.text, s, got, w))
    # the generator emits supported syntax only: a decline names a construction bound
    assert not wrongly_declined, wrongly_declined[:5]
    assert not bad, "%d disagreements:\n%s" % (len(bad), "\n".join(bad[:10]))


@pytest.mark.parametrize("seed", SEEDS)
def test_rewrites_keep_every_answer(seed):
    bad = []
    for c in cases(seed):
        if not c.accepted:
            continue
        got = None
        for name, how in REWRITES.items():
            text = c.pattern.text(**how)
            if text == c.text:
                continue
            if got is None:
                got = [regex_match(c.text, s)[1] for s in c.strings]
            for s, g in zip(c.strings, got):
                st, other, _, _, msg = regex_match(text, s)
                if st != L.DQ_OK:
                    bad.append("%s of %r: %r is declined: %s" % (name, c.text, text, msg))
                    break
                if other != g:
                    bad.append("%s of %r: %r answers %d on %r, the pattern %d" % (name, c.text, text, other, s, g))
    assert not bad, "%d differences:\n%s" % (len(bad), "\n".join(bad[:10]))


def test_rewrites_rewrite():
    p = next(c.pattern for c in all_cases() if "(" in c.text.replace("(?:", "").replace("\\(", "") and "[" in c.text)
    assert "(" not in p.text(noncapturing=True).replace("(?:", "").replace("\\(", "")
    some = [c for c in all_cases() if any(isinstance(a, G.Cls) for a in G.atoms(c.pattern))]
    assert sum("\\u" in c.pattern.text(uclass=True) for c in some) > 0.9 * len(some)
    lazy = [c for c in all_cases() if any(q in c.text for q in ("+?", "*?", "??", "}?"))]
    assert lazy and all(c.pattern.text(flip_lazy=True) != c.text for c in lazy)


def test_caps():
    """The tallies, and the caps that the generator alone must satisfy."""
    every = all_cases()
    accepted = [c for c in every if c.accepted]
    declined = [c for c in every if not c.accepted]
    empty = sum(C.oracle(c.text, "") for c in every)
    balanced = sum(0.1 <= c.rate <= 0.9 for c in accepted)
    above_16k = sum(c.table_bytes > 16 * 1024 for c in accepted)
    above_40k = sum(c.table_bytes > 40 * 1024 for c in accepted)
    sizes = sorted(c.table_bytes for c in accepted)
    print("patterns %d: accepted %d, declined by a bound %d (%.1f %%), matching \"\" %d" % (
        len(every), len(accepted), len(declined), 100.0 * len(declined) / len(every), empty))
    print("oracle match rate within [0.1, 0.9]: %d of %d accepted (%.1f %%); over all strings %.3f" % (
        balanced, len(accepted), 100.0 * balanced / len(accepted),
        sum(sum(c.want) for c in accepted) / sum(len(c.want) for c in accepted)))
    print("table bytes: median %d, above 16 KiB %d, above 40 KiB %d, largest %s" % (
        sizes[len(sizes) // 2], above_16k, above_40k, sizes[-8:]))
    assert len(every) >= 2000
    assert empty == 0
    assert len(declined) <= MAX_DECLINED * len(every)
    assert balanced >= MIN_BALANCED * len(accepted)
    assert above_16k >= MIN_ABOVE_16K and above_40k >= MIN_ABOVE_40K
