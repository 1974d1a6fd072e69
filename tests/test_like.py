"""LIKE / RLIKE in predicates, on the host: the front end (every accepted spelling, every decline
with its message, the syntax errors), the regex compiler's three matching modes through
dq_diag_regex_match_mode, generated LIKE patterns row by row through dq_diag_eval_predicate (the
host build of the interpreter, which walks the same DFA images the match-mask kernel walks), and
the reference's own LIKE fixture through Compliance states.  References: like_cases.py."""
import ctypes
import hashlib
import time

import numpy as np
import pytest

import like_cases as K
import pattern_cases as C
from deequ_amd import _lib as L
from deequ_amd.predicates import PredicateSyntaxError, UnsupportedPredicate, compile_predicate
from deequ_amd.table import Table
from test_pred_casts import _eval_lib, _otable

from oracle import pyoracle as O

SCHEMA = {"s": (0, "string"), "n": (1, "int64"), "Two Words": (2, "string"), "x": (3, "float64")}
COL, LIT, LIKE, RLIKE, NOT = L.DQ_P_COLUMN, L.DQ_P_LIT_STRING, L.DQ_P_LIKE, L.DQ_P_RLIKE, L.DQ_P_NOT


def triple(col, pattern, op, at=0):
    b = pattern.encode("utf-8")
    return [(COL, col, 0, 0.0), (LIT, len(b), at, 0.0), (op, 0, 0, 0.0)]


# ---------------------------------------------------------------------------- 1. front end
def test_like_compiles_to_the_triple():
    """Fails before LIKE existed: `s LIKE 'a%'` raised PredicateSyntaxError("unexpected 'LIKE'")."""
    prog = compile_predicate("s LIKE 'a%'", SCHEMA)
    assert list(prog) == triple(0, "a%", LIKE) and prog.pool == b"a%"


@pytest.mark.parametrize("text,code,pool", [
    ("s like 'a%'", triple(0, "a%", LIKE), b"a%"),
    ("S LiKe 'a%'", triple(0, "a%", LIKE), b"a%"),
    ("s NOT LIKE 'x'", triple(0, "x", LIKE) + [(NOT, 0, 0, 0.0)], b"x"),
    ("s not like 'x'", triple(0, "x", LIKE) + [(NOT, 0, 0, 0.0)], b"x"),
    ("NOT s LIKE 'x'", triple(0, "x", LIKE) + [(NOT, 0, 0, 0.0)], b"x"),
    ("s RLIKE '^a+$'", triple(0, "^a+$", RLIKE), b"^a+$"),
    ("s rlike 'a'", triple(0, "a", RLIKE), b"a"),
    ("s REGEXP 'a'", triple(0, "a", RLIKE), b"a"),
    ("s NOT REGEXP 'a'", triple(0, "a", RLIKE) + [(NOT, 0, 0, 0.0)], b"a"),
    ("s not rlike 'a'", triple(0, "a", RLIKE) + [(NOT, 0, 0, 0.0)], b"a"),
    ("`s` LIKE 'a'", triple(0, "a", LIKE), b"a"),
    ("`Two Words` LIKE '%é_'", triple(2, "%é_", LIKE), "%é_".encode()),
    ("`two words` RLIKE 'x'", triple(2, "x", RLIKE), b"x"),
    ("s LIKE 'a' 'b%'", triple(0, "ab%", LIKE), b"ab%"),
    ("s LIKE 'it' \"'\" 's%'", triple(0, "it's%", LIKE), b"it's%"),
    ("s LIKE \"a%\"", triple(0, "a%", LIKE), b"a%"),
    ("s LIKE ''", triple(0, "", LIKE), b""),
    ("s RLIKE '^\\\\d{5}$'", triple(0, "^\\d{5}$", RLIKE), b"^\\d{5}$"),
    ("s RLIKE 'a\\\\\\\\b'", triple(0, "a\\\\b", RLIKE), b"a\\\\b"),
    ("s RLIKE '\\\\.' '\\\\w'", triple(0, "\\.\\w", RLIKE), b"\\.\\w"),
    ("s RLIKE 'a*'", triple(0, "a*", RLIKE), b"a*"),
    ("(s LIKE 'a%')", triple(0, "a%", LIKE), b"a%"),
])
def test_accepted_spellings(text, code, pool):
    prog = compile_predicate(text, SCHEMA)
    assert list(prog) == code and prog.pool == pool


def test_combinations_compile():
    prog = compile_predicate("s LIKE 'a%' OR s LIKE '%b'", SCHEMA)
    assert list(prog) == triple(0, "a%", LIKE) + triple(0, "%b", LIKE, at=2) + [(L.DQ_P_OR, 0, 0, 0.0)]
    prog = compile_predicate("n > 3 AND NOT (s RLIKE 'k' OR `Two Words` LIKE '_')", SCHEMA)
    assert [c[0] for c in prog].count(RLIKE) == 1 and [c[0] for c in prog].count(LIKE) == 1


@pytest.mark.parametrize("text,message", [
    # the left side
    ("n LIKE '1%'", "LIKE of the int64 column n: Spark casts it to string"),
    ("x RLIKE '1'", "RLIKE of the float64 column x: Spark casts it to string"),
    ("COALESCE(s, 'x') LIKE 'a'", "LIKE of COALESCE(...): the left side must be a string column"),
    ("'abc' LIKE 'a%'", "LIKE of a literal: the left side must be a string column"),
    ("CAST(n AS DOUBLE) RLIKE '1'", "RLIKE of CAST(...): the left side must be a string column"),
    ("3 REGEXP '3'", "RLIKE of a literal: the left side must be a string column"),
    # the right side
    ("s LIKE `Two Words`", "LIKE pattern is a column: the right side must be one string literal"),
    ("s RLIKE s", "RLIKE pattern is a column"),
    ("s LIKE NULL", "LIKE pattern is NULL"),
    ("s LIKE 3", "LIKE pattern is not a string literal"),
    ("s RLIKE COALESCE(s, 'a')", "RLIKE pattern is not a string literal"),
    ("s LIKE ('a')", "LIKE pattern is not a string literal"),
    # backslashes in the literal's source text
    ("s RLIKE '\\d'", "RLIKE pattern literal holds the backslash sequence \\d"),
    ("s RLIKE 'a\\nb'", "backslash sequence \\n"),
    ("s LIKE 'a\\%'", "LIKE pattern literal holds the backslash sequence \\%"),
    ("s LIKE 'a\\_'", "backslash sequence \\_"),
    ("s RLIKE '\\u0041'", "backslash sequence \\u"),
    ("s RLIKE 'a\\\\\\d'", "backslash sequence \\d"),
    ("s LIKE 'a\\'b'", "backslash sequence \\'"),
    ("s LIKE 'a' 'b\\%'", "backslash sequence \\%"),
    # a LIKE pattern that still holds a backslash
    ("s LIKE 'a\\\\b'", "LIKE pattern holds a backslash: Spark's LIKE escapes are not evaluated"),
    ("s LIKE '\\\\%'", "LIKE pattern holds a backslash"),
    # the compiler's declines, with the construct and its offset
    ("s RLIKE '(a)\\\\1'", "regex: a back-reference at offset 3"),
    ("s RLIKE '(?i)a'", "regex: an inline flag group at offset 0"),
    ("s RLIKE 'a(?=b)'", "regex: a look-around group at offset 1"),
    ("s RLIKE 'a++'", "regex: a possessive quantifier at offset 1"),
    ("s RLIKE '[a'", "regex: an unclosed character class at offset 0"),
    ("s RLIKE 'a{1001}'", "regex: a repetition count above 1000 at offset 1"),
    ("s RLIKE '(a|b)*a(a|b){14}'", "search DFA has more than 2048 states"),
    ("s LIKE '%a______________'", "LIKE: the pattern's DFA has more than 2048 states"),
])
def test_declines_name_their_cause(text, message):
    with pytest.raises(UnsupportedPredicate) as e:
        compile_predicate(text, SCHEMA)
    assert message in str(e.value), str(e.value)


@pytest.mark.parametrize("text", ["s LIKE", "s LIKE LIKE 'a'", "s NOT 'a'", "s RLIKE AND n > 1", "s NOT LIKE"])
def test_malformed_text_stays_a_syntax_error(text):
    with pytest.raises(PredicateSyntaxError):
        compile_predicate(text, SCHEMA)


def test_string_literals_elsewhere_are_unescaped_as_before():
    prog = compile_predicate("s = 'a\\%b' OR s = 'c\\\\d' OR s = 'it\\'s'", SCHEMA)
    assert prog.pool == b"a%bc\\dit's"


def test_over_the_bound_declines_in_milliseconds():
    """'%a' and 14 `_`: 2^15 subsets; the construction stops at kMaxStates of them."""
    pattern = ("%a" + "_" * 14).encode()
    t0 = time.perf_counter()
    with pytest.raises(L.UnsupportedOnGpu) as e:
        L.diag_regex_match(pattern + b"_", b"", "full")   # (a pattern no earlier test has compiled)
    dt = time.perf_counter() - t0
    assert "more than 2048 states" in str(e.value)
    assert dt < 0.25, "declined after %.0f ms" % (dt * 1e3)


# ---------------------------------------------------------------------------- the library's validator
def _validate(code, pool, types=("string", "int64")):
    data = {"s": (types[0], ["a"] if types[0] == "string" else [1]), "n": (types[1], [1])}
    return _eval_lib(code, pool, Table.from_pydict(data), ["s", "n"])


def test_validator_takes_only_the_triple():
    assert _validate(triple(0, "a%", LIKE), b"a%") == [True]
    assert _validate(triple(0, "b", RLIKE), b"b") == [False]
    # an empty pattern travels without a string pool: LIKE '' is FALSE for "a", RLIKE '' TRUE
    assert _validate(triple(0, "", LIKE), b"") == [False] and _validate(triple(0, "", RLIKE), None) == [True]
    for bad in ([(COL, 1, 0, 0.0), (LIT, 1, 0, 0.0), (LIKE, 0, 0, 0.0)],               # a numeric column
                [(LIT, 1, 0, 0.0), (LIT, 1, 0, 0.0), (LIKE, 0, 0, 0.0)],               # a literal on the left
                [(COL, 0, 0, 0.0), (COL, 0, 0, 0.0), (RLIKE, 0, 0, 0.0)],              # a column as the pattern
                [(COL, 0, 0, 0.0), (L.DQ_P_LIT_NULL, 0, 0, 0.0), (LIKE, 0, 0, 0.0)],   # NULL as the pattern
                [(COL, 0, 0, 0.0), (COL, 0, 0, 0.0), (L.DQ_P_COALESCE, 0, 0, 0.0), (LIT, 1, 0, 0.0), (LIKE, 0, 0, 0.0)]):
        st, msg = _validate(bad, b"a")
        assert st == L.DQ_ERR_UNSUPPORTED and "takes a string column on the left and one string literal" in msg, msg
    st, msg = _validate([(LIT, 1, 0, 0.0), (LIKE, 0, 0, 0.0)], b"a")
    assert st == L.DQ_ERR_INVALID and "underflow" in msg
    st, msg = _validate([(COL, 0, 0, 0.0), (LIT, 5, 0, 0.0), (LIKE, 0, 0, 0.0)], b"a")
    assert st == L.DQ_ERR_INVALID
    st, msg = _validate(triple(0, "a\\%", LIKE), b"a\\%")
    assert st == L.DQ_ERR_UNSUPPORTED and "LIKE: a backslash in the pattern at offset 1" in msg
    st, msg = _validate(triple(0, "(a)\\1", RLIKE), b"(a)\\1")
    assert st == L.DQ_ERR_UNSUPPORTED and "a back-reference at offset 3" in msg
    assert L.lib().dq_abi_version() == 4


# ---------------------------------------------------------------------------- 2. compiler modes
def _match(pattern, text, mode):
    return L.diag_regex_match(pattern.encode("utf-8"), text.encode("utf-8"), mode)[0]


def test_like_table_agrees_with_the_hand_matcher():
    for p, s, want in K.LIKE_CASES:
        assert int(K.like_match(p, s)) == want, (p, s)


@pytest.mark.parametrize("pattern", sorted({p for p, _, _ in K.LIKE_CASES}), ids=repr)
def test_full_mode_like_cases(pattern):
    for p, s, want in K.LIKE_CASES:
        if p == pattern:
            assert _match(p, s, "full") == want, (p, s)


def test_full_mode_early_accept_and_shapes():
    """A trailing % enters the accept row as soon as the prefix is read; `%` alone starts there."""
    assert L.diag_regex_match(b"%", b"", "full")[1] == 1 and L.diag_regex_match(b"%%", b"x", "full")[1] == 1
    # 'a%' on a text whose tail is not UTF-8 at all: accepted before the tail is read
    assert L.diag_regex_match(b"a%", b"a\xff\xfe", "full")[0] == 1
    # '%a__%b__' is about the sum of its halves, not their product
    _, whole, _ = L.diag_regex_match(b"%a______%b______", b"", "full")
    _, half, _ = L.diag_regex_match(b"%a______", b"", "full")
    assert whole <= 2 * half + 8, (whole, half)


@pytest.mark.parametrize("regex", sorted({p for p, _, _ in K.RLIKE_CASES}), ids=repr)
def test_find_mode_hand_cases(regex):
    for p, s, want in K.RLIKE_CASES:
        if p == regex:
            assert _match(p, s, "find") == want, (p, s)


@pytest.mark.parametrize("index", range(len(C.PATTERNS)))
def test_find_mode_pattern_list(index):
    """pattern_cases.PATTERNS with the non-empty condition dropped (none of them is nullable, so the
    answer is PatternMatch's), 600 mutated strings each."""
    pattern, strings = C.pattern_inputs(index, 600)
    hits = 0
    for s in strings:
        want = int(K.rlike_match(pattern, s))
        assert _match(pattern, s, "find") == want, (pattern, s)
        assert want == C.oracle(pattern, s)
        hits += want
    assert 0 < hits < len(strings)


@pytest.mark.parametrize("regex", K.NULLABLE_REGEXES, ids=repr)
def test_find_mode_nullable_list(regex):
    rng = np.random.default_rng(len(regex))
    strings = C.make_strings(["", "123", "aaa", "12a", "x", "123\n", "\n"], 400, rng)
    for s in strings:
        assert _match(regex, s, "find") == int(K.rlike_match(regex, s)), (regex, s)
    with pytest.raises(L.UnsupportedOnGpu, match="can match the empty string"):
        L.diag_regex_match(regex.encode(), b"", "find_non_empty")
    if regex != r"x*$":  # (declined by PatternMatch too, and by the old entry point still)
        assert regex in C.MUST_REJECT


@pytest.mark.parametrize("regex", K.RLIKE_MUST_REJECT, ids=repr)
def test_find_mode_keeps_every_other_decline(regex):
    with pytest.raises(L.UnsupportedOnGpu):
        L.diag_regex_match(regex.encode("utf-8"), b"", "find")


def test_find_non_empty_images_are_byte_identical_to_the_parent_build():
    doc = K.image_digests()
    assert [e["pattern"] for e in doc["images"]] == [p for p, _ in C.PATTERNS]
    for e in doc["images"]:
        p = e["pattern"].encode("utf-8")
        image = L.diag_regex_match(p, b"", "find_non_empty", want_image=True)[3]
        assert len(image) == e["bytes"] and hashlib.sha256(image).hexdigest() == e["sha256"], e["pattern"]
        # the old entry point is that mode
        m, ns, nc = L.c_int32(0), L.c_int32(0), L.c_int32(0)
        L.check(L.lib().dq_diag_regex_match(p, len(p), b"", 0, ctypes.byref(m), ctypes.byref(ns), ctypes.byref(nc)))
        assert (ns.value, nc.value) == L.diag_regex_match(p, b"", "find_non_empty")[1:3]


# ---------------------------------------------------------------------------- 3. generated
GEN_SEEDS = [11, 12, 13, 14]
PER_SEED = 40
STRINGS = 160


@pytest.mark.parametrize("seed", GEN_SEEDS)
def test_generated_like_row_by_row(seed):
    """Generated patterns over mutated matching strings, row by row; then NOT LIKE and four combined
    forms against Kleene logic over the hand matcher and the oracle's verdict of the other side."""
    cases = K.generated_like(seed, PER_SEED, STRINGS)
    rng = np.random.default_rng(seed)
    both = declined_other = combined = 0
    for k, (pattern, strings) in enumerate(cases):
        assert len(pattern) <= 24 and "\\" not in pattern
        data = K.combined_table(strings, seed * 1000 + k)
        names = list(data)
        schema = {nm: (i, data[nm][0]) for i, nm in enumerate(names)}
        table = Table.from_pydict(data)
        text = "s LIKE " + K.sql_quote(pattern)
        prog = compile_predicate(text, schema)   # no generated pattern may be declined
        want = [K.verdict("like", pattern, s) for s in data["s"][1]]
        got = _eval_lib(prog.code, prog.pool, table, names)
        assert got == want, (pattern, [(s, g, w) for s, g, w in zip(data["s"][1], got, want) if g != w][:5])
        both += (True in want) and (False in want)
        neg = compile_predicate("s NOT LIKE " + K.sql_quote(pattern), schema)
        assert _eval_lib(neg.code, neg.pool, table, names) == [K.k_not(w) for w in want]
        otable = _otable(data)
        for form in range(4):
            other = K.OTHERS[int(rng.integers(len(K.OTHERS)))]
            sql, fn = K.combine(form, text, other)
            combined += 1
            try:
                cprog = compile_predicate(sql, schema)
            except UnsupportedPredicate:
                compile_predicate(text, schema)
                with pytest.raises(UnsupportedPredicate):   # ... for a reason on the other side only
                    compile_predicate(other, schema)
                declined_other += 1
                continue
            expect = [fn(w, o) for w, o in zip(want, O.eval_predicate(other, otable))]
            assert _eval_lib(cprog.code, cprog.pool, table, names) == expect, sql
    assert both >= 0.8 * len(cases), "only %d of %d patterns gave both verdicts" % (both, len(cases))
    assert declined_other <= 0.05 * combined


def test_generator_is_deterministic_and_within_its_limits():
    a, b = K.generated_like(5, 30, 10), K.generated_like(5, 30, 10)
    assert a == b and a != K.generated_like(6, 30, 10)
    for seed in GEN_SEEDS:
        for pattern, _ in K.generated_like(seed, PER_SEED, 2):
            assert 1 <= len(pattern) <= 24 and "\\" not in pattern and "'" not in pattern
            for seg in pattern.split("%")[1:]:
                assert seg.count("_") <= 6
    assert any(seg.count("_") == 6 for p in K.EXTREME_LIKE for seg in p.split("%")[1:])


# ---------------------------------------------------------------------------- 4. the reference's fixture
def _fixture_tables():
    import deequ_amd as d
    fx = K.known_answers()
    def make(rows):
        cols = list(zip(*rows)) if rows else [[] for _ in fx["columns"]]
        return d.Table.from_pydict({nm: (t, list(c)) for nm, t, c in zip(fx["columns"], fx["types"], cols)})
    return fx, make(fx["initial"]), make(fx["delta"]), make(fx["initial"] + fx["delta"])


def test_reference_fixture_compiles_and_evaluates_on_the_host():
    """IncrementalAnalysisTest.scala:69-71 over :108-160, on the host build of the interpreter: the
    counts are the hand matcher's (the GPU run of the same analyzers and the state merge are in
    test_gpu_like.py)."""
    fx, initial, delta, everything = _fixture_tables()
    assert initial.num_rows == 20 and delta.num_rows == 20
    names = fx["columns"]
    schema = {nm: (k, t) for k, (nm, t) in enumerate(zip(names, fx["types"]))}
    counts = {}
    for a in fx["analyzers"][1:]:
        prog = compile_predicate(a["predicate"], schema)
        for label, table, rows in (("initial", initial, fx["initial"]), ("delta", delta, fx["delta"]),
                                   ("everything", everything, fx["initial"] + fx["delta"])):
            got = _eval_lib(prog.code, prog.pool, table, names)
            want = [K.like_match(a["like"], r[2]) for r in rows]
            assert got == want
            counts[a["instance"], label] = sum(want)
    assert counts["categoryAttribute", "initial"] == 12 and counts["categoryAttribute", "delta"] == 0
    assert counts["attributeKeyword", "initial"] == 0 and counts["attributeKeyword", "delta"] == 20
    assert counts["attributeKeyword", "everything"] == 20 and counts["categoryAttribute", "everything"] == 12
