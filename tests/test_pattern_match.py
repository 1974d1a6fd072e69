"""PatternMatch (PatternMatch.scala:37-55) without a GPU: the host build of the regex engine
(dq_diag_regex_match: the compiler plan creation runs and the table walker the kernel runs) against
an independent oracle -- Python's re.search(p, s, re.ASCII) with a non-empty group 0 -- over a fixed
pattern list covering every supported construct; Java's line-terminator rules by hand; everything
the compiler must decline; and the op through every host layer (dq_op_supported, the packed blob,
state merge / metric, the state provider, the analyzer's string form).  GPU runs: test_gpu_pattern_match.py."""
import ctypes
import struct

import pytest

import deequ_amd as d
from deequ_amd import _lib as L
from deequ_amd.engine import OpSpec, op_spec_for, op_supported, pack_ops

import pattern_cases as C


def regex_match(pattern: str, text: str):
    """(status, matched, n_states, n_classes, message) of dq_diag_regex_match."""
    pb, tb = pattern.encode("utf-8"), text.encode("utf-8")
    m, ns, nc = ctypes.c_int32(-1), ctypes.c_int32(0), ctypes.c_int32(0)
    st = L.lib().dq_diag_regex_match(pb, len(pb), tb, len(tb), ctypes.byref(m), ctypes.byref(ns), ctypes.byref(nc))
    return st, m.value, ns.value, nc.value, L.lib().dq_last_error().decode("utf-8", "replace")


def test_pattern_list_covers_the_issue():
    assert len(C.PATTERNS) >= 25
    pats = [p for p, _ in C.PATTERNS]
    assert C.EMAIL in pats and C.URL in pats and C.UUID in pats and "^" + C.UUID + "$" in pats


@pytest.mark.parametrize("index", range(len(C.PATTERNS)), ids=lambda i: "p%02d" % i)
def test_engine_equals_oracle(index):
    pattern, strings = C.pattern_inputs(index)
    assert len(strings) >= 3000 and min(map(len, strings)) == 0 and max(map(len, strings)) == 70
    assert any(len(s.encode("utf-8")) > len(s) for s in strings)  # multi-byte characters
    assert not any(c in s for s in strings for c in "\r\u0085\u2028\u2029")
    want = [C.oracle(pattern, s) for s in strings]
    rate = sum(want) / len(want)
    print("pattern %r: oracle match rate %.3f" % (pattern, rate))
    assert 0.1 <= rate <= 0.9, (pattern, rate)  # (an always-true or always-false engine cannot pass)
    for seed in C.PATTERNS[index][1]:
        assert C.oracle(pattern, seed) == 1, (pattern, seed)
    bad = []
    for s, w in zip(strings, want):
        st, got, _, _, msg = regex_match(pattern, s)
        assert st == L.DQ_OK, (pattern, msg)
        if got != w:
            bad.append((s, w, got))
    assert not bad, (pattern, len(bad), bad[:5])


@pytest.mark.parametrize("pattern,text,want", C.JAVA_LINE_CASES)
def test_java_line_terminators(pattern, text, want):
    st, got, _, _, msg = regex_match(pattern, text)
    assert st == L.DQ_OK, msg
    assert got == want, (pattern, text)


def test_table_shape_is_reported():
    st, got, n_states, n_classes, msg = regex_match(C.EMAIL, "someone@somewhere.org")
    assert (st, got) == (L.DQ_OK, 1), msg
    # a few hundred states and a few dozen byte classes (+ the end-of-input column): a table of
    # a few KiB, far below the kernel's 48 KiB LDS budget
    assert 50 <= n_states <= 400 and 10 <= n_classes <= 40, (n_states, n_classes)
    assert regex_match(C.URL, "h://test")[:2] == (L.DQ_OK, 0)
    st, _, n_states, n_classes, _ = regex_match("a", "")
    assert (st, n_states, n_classes) == (L.DQ_OK, 2, 3)  # states {accept, searching}, columns {a, any other byte, end}


@pytest.mark.parametrize("pattern", C.MUST_REJECT, ids=lambda p: repr(p[:24]))
def test_unsupported_patterns_are_declined(pattern):
    st, _, _, _, msg = regex_match(pattern, "x")
    assert st == L.DQ_ERR_UNSUPPORTED, (pattern, st, msg)
    assert "offset" in msg and "regex" in msg, msg  # names the construct and where it is


def test_invalid_pattern_text_is_declined_not_read_past():
    for raw in (b"\xff", b"a\xc3", b"\xe4\xbe", b"[a-\xf0\x9f]", b"\\", b"(", b"[", b"[a", b"a{", b"a{2", b"a{2,", b"\\x4",
                b"\\u00e", b"(?", b"(?<", b"a|*", b"a{3,2}", b"[z-a]", b"a{1001}", b")", b"a)"):
        m = ctypes.c_int32(-1)
        st = L.lib().dq_diag_regex_match(raw, len(raw), b"x", 1, ctypes.byref(m), None, None)
        assert st == L.DQ_ERR_UNSUPPORTED, raw


def test_state_cap_declines_quickly():
    st, _, _, _, msg = regex_match(C.STATE_CAP_PATTERN, "ab")
    # declined by the state cap itself (2048 subsets of a 50-node NFA), not by a table that was
    # built to its 32768 states and then found too large
    assert st == L.DQ_ERR_UNSUPPORTED and "more than 2048 states" in msg, msg
    st, _, _, _, msg = regex_match(r"(a|b)*a(a|b){200}", "ab")
    assert st == L.DQ_ERR_UNSUPPORTED, msg
    st, _, _, _, msg = regex_match(r"((((a{1000}){1000}){1000}){1000}){1000}", "a")
    assert st == L.DQ_ERR_UNSUPPORTED and "NFA" in msg, msg


def test_op_supported_by_type_and_pattern():
    string_schema, float_schema = {"some": "string"}, {"some": "float64"}
    ok = d.PatternMatch("some", r"\d\.\d")
    op_supported(op_spec_for(ok, string_schema), string_schema)
    with pytest.raises(L.UnsupportedOnGpu):  # Spark would cast the column to string; this path does not
        op_supported(op_spec_for(ok, float_schema), float_schema)
    # the remembered answer is per pattern: a declined pattern after an accepted one on the same column
    for bad in (C.CREDITCARD, C.SSN, r"\d*"):
        with pytest.raises(L.UnsupportedOnGpu):
            op_supported(op_spec_for(d.PatternMatch("some", bad), string_schema), string_schema)
    op_supported(op_spec_for(d.PatternMatch("some", C.EMAIL, "some IS NOT NULL"), string_schema), string_schema)
    op_supported(op_spec_for(ok, string_schema), string_schema)
    # an instruction in the pattern's predicate slot is malformed, not unsupported
    op = L.DqOp()
    OpSpec(L.DQ_OP_PATTERN_MATCH, 0, [(L.DQ_P_TRUE, 0, 0, 0.0)]).fill(op)
    types = (ctypes.c_int32 * 1)(L.DQ_T_UTF8)
    assert L.lib().dq_op_supported(ctypes.byref(op), types, 1) == L.DQ_ERR_INVALID
    assert L.lib().dq_abi_version() == 4


def test_packed_blob_carries_the_pattern():
    schema = {"s": "string", "i": "int64"}
    an = [d.PatternMatch("s", C.URL), d.Completeness("s"), d.PatternMatch("s", "é+x", "i > 3")]
    blob = pack_ops([op_spec_for(a, schema) for a in an])
    magic, version, n = struct.unpack_from("<III", blob)
    assert (magic, version, n) == (0x504F5144, 1, 3)
    at, seen = 12, []
    for _ in range(n):  # the layout of include/deequ_amd.h, decoded independently
        kind, col, col2, n_pred, n_ps, n_where, n_ws = struct.unpack_from("<7i", blob, at)
        at += 28 + 24 * n_pred
        pool = blob[at:at + n_ps]
        at += n_ps + 24 * n_where + n_ws
        seen.append((kind, col, n_pred, pool, n_where))
    assert at == len(blob)
    url, lit = C.URL.encode("utf-8"), "é+x".encode("utf-8")
    assert seen[0] == (14, 0, 0, url, 0) and seen[1][:3] == (2, 0, 0) and seen[2][:4] == (14, 0, 0, lit)
    assert seen[2][4] > 0
    # the library decodes it completely and reaches dq_plan_create (no context on this host)
    types = (ctypes.c_int32 * 2)(L.DQ_T_UTF8, L.DQ_T_INT64)
    h = ctypes.c_void_p()
    st = L.lib().dq_plan_create_packed(None, blob, len(blob), types, 2, ctypes.byref(h))
    assert st == L.DQ_ERR_INVALID and "NULL argument" in L.lib().dq_last_error().decode()
    st = L.lib().dq_plan_create_packed(None, blob[:-1], len(blob) - 1, types, 2, ctypes.byref(h))
    assert st == L.DQ_ERR_INVALID and "NULL argument" not in L.lib().dq_last_error().decode()


def _state(kind, has, matches, count):
    s = L.DqState()
    s.kind, s.has_value, s.num_matches, s.count = kind, has, matches, count
    return s


def test_state_merge_and_metric():
    K = L.DQ_OP_PATTERN_MATCH
    a, b, out, v = _state(K, 1, 3, 4), _state(K, 1, 10, 13), L.DqState(), ctypes.c_double()
    assert L.lib().dq_state_merge(ctypes.byref(a), ctypes.byref(b), ctypes.byref(out)) == L.DQ_OK
    assert (out.kind, out.has_value, out.num_matches, out.count) == (K, 1, 13, 17)
    assert L.lib().dq_state_metric(ctypes.byref(out), ctypes.byref(v)) == L.DQ_OK and v.value == 13 / 17
    none = _state(K, 0, 0, 0)  # Analyzers.merge: None is the identity
    assert L.lib().dq_state_merge(ctypes.byref(none), ctypes.byref(a), ctypes.byref(out)) == L.DQ_OK
    assert (out.has_value, out.num_matches, out.count) == (1, 3, 4)
    assert L.lib().dq_state_metric(ctypes.byref(none), ctypes.byref(v)) == L.DQ_ERR_STATE
    other = _state(L.DQ_OP_COMPLETENESS, 1, 1, 1)
    assert L.lib().dq_state_merge(ctypes.byref(a), ctypes.byref(other), ctypes.byref(out)) == L.DQ_ERR_INVALID
    # two ranks' states folded as dq_group_allgather_merge folds them
    gathered = (L.DqState * 4)(_state(K, 1, 1, 2), _state(K, 0, 0, 0), _state(K, 1, 5, 6), _state(K, 0, 0, 0))
    folded = (L.DqState * 2)()
    assert L.lib().dq_states_merge_ranks(gathered, 2, 2, folded) == L.DQ_OK
    assert (folded[0].has_value, folded[0].num_matches, folded[0].count) == (1, 6, 8) and folded[1].has_value == 0
    # the Python mirror maps kind 14 onto NumMatchesAndCount
    from deequ_amd.states import state_from_dq
    assert state_from_dq(a) == d.NumMatchesAndCount(3, 4) and state_from_dq(none) is None
    assert d.NumMatchesAndCount(3, 4).sum(d.NumMatchesAndCount(1, 1)).metricValue() == 0.8


def test_state_provider_round_trip(tmp_path):
    a = d.PatternMatch("some", C.EMAIL)
    provider = d.HdfsStateProvider(str(tmp_path / "states"))
    provider.persist(a, d.NumMatchesAndCount(3, 4))
    assert provider.load(a) == d.NumMatchesAndCount(3, 4)
    # the layout Completeness uses (StateProvider.scala:94,151): two big-endian longs
    files = [p for p in (tmp_path).rglob("*") if p.is_file() and not p.name.startswith(".") and p.suffix != ".crc"]
    assert [p.read_bytes() for p in files] == [struct.pack(">qq", 3, 4)], files
    # another pattern is another analyzer: nothing stored under its identifier
    with pytest.raises(FileNotFoundError):
        provider.load(d.PatternMatch("some", C.URL))
    mem = d.InMemoryStateProvider()
    mem.persist(a, d.NumMatchesAndCount(1, 2))
    assert mem.load(a) == d.NumMatchesAndCount(1, 2)
    m = a.calculateMetric(d.NumMatchesAndCount(2, 2), aggregateWith=mem)
    assert m.value.get() == 0.75 and (m.name, m.instance) == ("PatternMatch", "some")


def test_analyzer_string_form_and_mirror():
    assert str(d.PatternMatch("col", "pattern")) == "PatternMatch(col,pattern,None)"
    assert str(d.PatternMatch("att1", r"\d+", "att2 > 0")) == r"PatternMatch(att1,\d+,Some(att2 > 0))"
    a = d.PatternMatch("some", r"\d")
    assert isinstance(a, d.StandardScanShareableAnalyzer) and a.DQ_KIND == 14 == L.DQ_OP_PATTERN_MATCH
    assert a.preconditions() == []  # the reference declares none
    assert a == d.PatternMatch("some", r"\d") and hash(a) == hash(d.PatternMatch("some", r"\d"))
    assert a != d.PatternMatch("some", r"\D")
    assert not hasattr(d, "Patterns")
    failure = a.computeMetricFrom(None)
    assert failure.value.isFailure and isinstance(failure.value.exception, d.EmptyStateException)
