"""`where` on the frequency analyzers, without a GPU: what an unfiltered analyzer prints, equals and
hashes to is what it was before the field existed; a filter shows as `,Some(<where>)`, takes part in
== / hash, separates the runner's frequency tables, and a filter that does not parse, names a missing
column or leaves the GPU subset is a failure metric, not an exception out of the runner."""
import dataclasses
from types import SimpleNamespace

import numpy as np
import pytest

import deequ_amd as d
from deequ_amd import frequencies as F
from deequ_amd.analyzers import (CountDistinct, Distinctness, Entropy, MutualInformation, Preconditions,
                                 UniqueValueRatio, Uniqueness)
from deequ_amd.predicates import UnsupportedPredicate
from deequ_amd.runner import AnalysisRunner, grouping_key

MULTI = (Uniqueness, Distinctness, CountDistinct, UniqueValueRatio)

# (analyzer, str, repr, the compared fields it had before `where`)
UNFILTERED = [
    (Uniqueness(["a"]), "Uniqueness(List(a))", "Uniqueness(columns=('a',))", (("a",),)),
    (Uniqueness(["a", "b"]), "Uniqueness(List(a, b))", "Uniqueness(columns=('a', 'b'))", (("a", "b"),)),
    (Distinctness(["a"]), "Distinctness(List(a))", "Distinctness(columns=('a',))", (("a",),)),
    (CountDistinct("a"), "CountDistinct(List(a))", "CountDistinct(columns=('a',))", (("a",),)),
    (UniqueValueRatio(["b", "a"]), "UniqueValueRatio(List(b, a))", "UniqueValueRatio(columns=('b', 'a'))",
     (("b", "a"),)),
    (Entropy("a"), "Entropy(a)", "Entropy(column='a')", ("a",)),
    (MutualInformation(["a", "b"]), "MutualInformation(List(a, b))", "MutualInformation(columns=('a', 'b'))",
     (("a", "b"),)),
    (MutualInformation("a", "b"), "MutualInformation(List(a, b))", "MutualInformation(columns=('a', 'b'))",
     (("a", "b"),)),
]


@pytest.mark.parametrize("a,text,rep,fields", UNFILTERED, ids=[u[1] + str(i) for i, u in enumerate(UNFILTERED)])
def test_unfiltered_analyzer_is_what_it_was(a, text, rep, fields):
    assert a.where is None
    assert str(a) == text
    assert repr(a) == rep
    # the generated hash of the fields it had, with the class mixed in (analyzers._memoise_hashes)
    assert hash(a) == hash((type(a).__qualname__, hash(fields)))
    same = type(a)(*[getattr(a, f.name) for f in dataclasses.fields(a) if f.name != "where"])
    assert a == same and hash(a) == hash(same)
    assert type(a)(*[getattr(a, f.name) for f in dataclasses.fields(a)]) == a  # where=None spelled out


def test_fields_by_position():
    for cls in MULTI:
        assert [f.name for f in dataclasses.fields(cls)] == ["columns", "where"]
        assert cls(["a"], "x > 1") == cls(["a"], where="x > 1")
    assert [f.name for f in dataclasses.fields(Entropy)] == ["column", "where"]
    assert [f.name for f in dataclasses.fields(MutualInformation)] == ["columns", "columnB", "where"]
    assert Entropy("a", "x > 1").where == "x > 1"
    assert MutualInformation("a", "b", "x > 1") == MutualInformation(["a", "b"], where="x > 1")
    # the second positional argument is columnB: a filter put there is named, not taken as a column
    with pytest.raises(ValueError, match="pass a filter as where="):
        MutualInformation(["a", "b"], "x > 1")


def test_filtered_strings():
    assert str(Uniqueness(["a"], "x > 1")) == "Uniqueness(List(a),Some(x > 1))"
    assert str(Distinctness(["a", "b"], "x > 1")) == "Distinctness(List(a, b),Some(x > 1))"
    assert str(CountDistinct(["a"], "s LIKE 'k%'")) == "CountDistinct(List(a),Some(s LIKE 'k%'))"
    assert str(UniqueValueRatio(["a"], "x IS NULL")) == "UniqueValueRatio(List(a),Some(x IS NULL))"
    assert str(Entropy("a", "x > 1")) == "Entropy(a,Some(x > 1))"
    assert str(MutualInformation(["a", "b"], where="x > 1")) == "MutualInformation(List(a, b),Some(x > 1))"
    assert repr(Uniqueness(["a"], "x > 1")) == "Uniqueness(columns=('a',), where='x > 1')"
    assert repr(Entropy("a", "x > 1")) == "Entropy(column='a', where='x > 1')"


@pytest.mark.parametrize("make", [lambda w: Uniqueness(["a"], w), lambda w: Distinctness(["a"], w),
                                  lambda w: CountDistinct(["a"], w), lambda w: UniqueValueRatio(["a"], w),
                                  lambda w: Entropy("a", w), lambda w: MutualInformation(["a", "b"], where=w)])
def test_where_takes_part_in_eq_and_hash(make):
    plain, f1, f1b, f2 = make(None), make("x > 1"), make("x > 1"), make("x > 2")
    assert f1 == f1b and hash(f1) == hash(f1b)
    assert plain != f1 and f1 != f2 and plain != f2
    assert len({plain, f1, f1b, f2}) == 3
    assert len({str(plain), str(f1), str(f2)}) == 3  # (the state providers' identifiers come from str)


def test_grouping_key():
    assert grouping_key(Uniqueness(["a"])) == (("a",), None)
    assert grouping_key(Uniqueness(["b", "a"], "x > 1")) == (("a", "b"), "x > 1")
    keys = {grouping_key(a) for a in (Uniqueness(["a"]), Uniqueness(["a"], "x > 1"), Uniqueness(["a"], "x > 2"))}
    assert len(keys) == 3
    assert grouping_key(Distinctness(["a"], "x > 1")) == grouping_key(Entropy("a", "x > 1"))


class _State:
    def __init__(self, cols, where):
        self.cols, self.where = cols, where

    def summary(self):
        n = {None: 10, "x > 1": 5, "x > 2": 4}[self.where]
        return SimpleNamespace(num_rows=n, num_groups=2, num_unique=1, grouped_rows=n, entropy=0.5)


def test_runner_builds_one_table_per_columns_and_where(monkeypatch):
    calls = []

    def fake(data, cols, histogram=False, where=None):
        calls.append((tuple(cols), where))
        return _State(tuple(cols), where)

    monkeypatch.setattr(F, "compute_frequencies", fake)
    analyzers = [Uniqueness(["a"]), Uniqueness(["a"], "x > 1"), Uniqueness(["a"], "x > 2"),
                 Distinctness(["a"], "x > 1"), Entropy("a", "x > 1"), Distinctness(["a"])]
    tables = {}
    ctx = AnalysisRunner._runGroupingAnalyzers(None, analyzers, None, None, tables)
    assert calls == [(("a",), None), (("a",), "x > 1"), (("a",), "x > 2")]
    assert ctx.metric(Uniqueness(["a"])).value.get() == 1 / 10
    assert ctx.metric(Uniqueness(["a"], "x > 1")).value.get() == 1 / 5
    assert ctx.metric(Uniqueness(["a"], "x > 2")).value.get() == 1 / 4
    assert ctx.metric(Distinctness(["a"], "x > 1")).value.get() == 2 / 5
    assert ctx.metric(Distinctness(["a"])).value.get() == 2 / 10
    # only the unfiltered table is offered to a Histogram of the same column
    assert list(tables) == [("a",)] and tables[("a",)].where is None


def test_aggregated_states_are_keyed_by_where():
    schema = {"a": "int64", "x": "int64"}
    plain, filt = Uniqueness(["a"]), Uniqueness(["a"], "x > 1")
    loader = SimpleNamespace(load=lambda a: {plain: _State(("a",), None), filt: _State(("a",), "x > 1")}.get(a))
    # Distinctness(a, x > 1) has no state of its own: it reads the one of its (columns, where)
    analysis = d.Analysis([plain, filt, Distinctness(["a"], "x > 1"), Distinctness(["a"], "x > 2")])
    ctx = AnalysisRunner.runOnAggregatedStates(schema, analysis, [loader])
    assert ctx.metric(plain).value.get() == 1 / 10
    assert ctx.metric(filt).value.get() == 1 / 5
    assert ctx.metric(Distinctness(["a"], "x > 1")).value.get() == 2 / 5
    assert not ctx.metric(Distinctness(["a"], "x > 2")).value.is_success()


def _host_table():
    return d.Table({"a": d.Column.from_numpy(np.arange(4), None, "int64"),
                    "x": d.Column.from_numpy(np.arange(4), None, "int64")})


@pytest.mark.parametrize("where,needle", [("x >", "x >"), ("nope > 1", "Input data does not include column nope!")])
@pytest.mark.parametrize("make", [lambda w: Uniqueness(["a"], w), lambda w: Entropy("a", w),
                                  lambda w: MutualInformation(["a", "x"], where=w)])
def test_bad_where_is_a_failure_metric(make, where, needle):
    a = make(where)
    ctx = AnalysisRunner.onData(_host_table()).addAnalyzer(a).run()  # (nothing passes: no GPU work)
    m = ctx.metric(a)
    assert not m.value.is_success()
    assert needle in str(m.value.exception)


def test_unsupported_where_surfaces_its_message():
    a = CountDistinct(["a"], "x + 1 > 2")
    err = Preconditions.findFirstFailing({"a": "int64", "x": "int64"}, a.preconditions())
    assert isinstance(err, UnsupportedPredicate)
    ctx = AnalysisRunner.onData(_host_table()).addAnalyzer(a).run()
    m = ctx.metric(a)
    assert not m.value.is_success()
    assert str(err) in str(m.value.exception)
    assert "arithmetic (+) is not GPU-eligible" in str(m.value.exception)


def test_where_resolves_names_like_the_scan_analyzers():
    schema = {"a": "int64", "X": "int64"}
    assert Preconditions.findFirstFailing(schema, Uniqueness(["a"], "x > 1").preconditions()) is None
    amb = {"a": "int64", "X": "int64", "x": "int64"}
    err = Preconditions.findFirstFailing(amb, Uniqueness(["a"], "x > 1").preconditions())
    assert str(err) == "Reference 'x' is ambiguous, could be: X, x"  # the predicate module's own error
    err = Preconditions.findFirstFailing(amb, Uniqueness(["a"], "xX > 1").preconditions())
    assert str(err) == "Input data does not include column xX!"
