"""Seeded generator of SQL predicates over the grammar `deequ_amd.predicates._Parser` accepts, and
the boundary-value table they are evaluated on.  Shared by the host test (test_pred_generated.py:
`dq_diag_eval_predicate` against the oracle row by row) and the GPU test
(test_gpu_pred_generated.py: the same texts through real plans).

`generate(seed, count, family)` draws from `random.Random(seed)` alone (no hashing, no sets), so a
seed gives the same texts on every machine.  Family "numeric" uses the columns l d g i b, family
"string" adds the string column s and string literals (string equality and ordering, IN lists of
strings, string against number = Spark 2.2 PromoteStrings).

Covered: the comparison operators = == != <> < <= > >= <=>, [NOT] IN of 1 to 4 items (NULL
included), [NOT] BETWEEN, IS [NOT] NULL, AND / OR / NOT / parentheses two levels deep, the bare
boolean forms b / TRUE / cast(x as boolean), COALESCE of 2 to 3 arguments, CAST to every name of
`_CAST_TYPES` (nested one level), unary minus, keywords and column names in varied case (and
`quoted` names), and -- a fixed share -- exactly the forms the fused scan evaluates inline
(dq_api.cpp fast_form): `col CMP literal`, `literal CMP col`, `COALESCE(col, literal) CMP literal`,
`col IS [NOT] NULL`, a boolean column, TRUE / FALSE.

Left out, because the compiler declines them by design (each has its own decline test; the
message is the compiler's):
  * arithmetic                                "arithmetic (+) is not GPU-eligible in ..."
  * functions other than COALESCE and CAST    "function abs() is not GPU-eligible"
  * COALESCE of a string with a non-string    "COALESCE of a string with a non-string"
  * COALESCE of a boolean with a number       "COALESCE of mixed boolean/numeric"
  * IN lists mixing strings and numbers       "IN list mixing strings and numbers"
  * IN lists mixing booleans and numbers      "IN list mixing booleans and numbers"
  * unary minus on a column or an expression  "unary - on a non-literal in ..."
Still generated, rarely, so that the decline path is exercised and counted (the tests cap the
declined share): CAST of a string to anything but DOUBLE, CAST of a decimal literal to FLOAT, a
string compared with a boolean, and a decimal-typed COALESCE in an integer comparison.
"""
import random
import re

from deequ_amd import _lib as L
from deequ_amd.predicates import _CAST_TYPES
from test_pred_casts import BOOLS, DOUBLES, FLOATS, INTS, LONGS, STRINGS

# the cast-test pool plus the empty string (parses to NULL), the text of the 'a''b' literal, an
# exponent form and Java's "NaN" (Double.parseDouble accepts both)
STRING_VALUES = STRINGS + ["", "ab", "1e2", "NaN"]

POOLS = {"l": ("int64", LONGS), "d": ("float64", DOUBLES), "g": ("float32", FLOATS), "i": ("int32", INTS),
         "b": ("bool", BOOLS), "s": ("string", STRING_VALUES)}


def table(n, seed):
    """{name: (dtype, values)} of n rows picked from the pools; for n >= 64 every pool value (None
    included) occurs at least once in its column, at seeded positions."""
    rng = random.Random(seed)
    out = {}
    for name, (dtype, pool) in POOLS.items():
        vals = [pool[rng.randrange(len(pool))] for _ in range(n)]
        if n >= 64:
            for v, pos in zip(pool, rng.sample(range(n), len(pool))):
                vals[pos] = v
        out[name] = (dtype, vals)
    return out


INT_LITERALS = ["0", "3", "-3", "4", "-4", "127", "128", "16777216", "16777217", "2147483647", "2147483648",
                "-2147483649", "9223372036854775807", "-9223372036854775808", "9223372036854775808",
                "99999999999999999999", "- 3", "- -4", "18446744073709551619", "-9223372036854775809"]
DEC_LITERALS = ["3.5", "-3.5", "4.0", "0.1", "2.5", "2147483647.5", "16777217.0", "9223372036854775806.5",
                "9223372036854775807.5", "-9223372036854775808.5", "99999999999999999999.5", ".5", "- 2.5"]
DBL_LITERALS = ["3.5e0", "0.1D", "1e300", "-0.0e0", "1.6777217e7", "9.3e18", "3.4028235e38", "3D", "2147483647.5d",
                "- 9.3E18"]
STR_LITERALS = ["'3'", "' 4 '", "'x'", "'2.5'", "''", "'a''b'", "'a' 'b'"]

OPERATORS = ["=", "==", "!=", "<>", "<", "<=", ">", ">=", "<=>"]
NUMERIC_CASTS = [t for t in _CAST_TYPES if t != "BOOLEAN"]


class _Gen:
    def __init__(self, rng, family):
        self.rng = rng
        self.strings = family == "string"

    # ------------------------------------------------------------------ lexical variety
    def kw(self, word):
        r = self.rng.random()
        return word if r < 0.6 else word.lower() if r < 0.85 else word.capitalize()

    def col(self, name):
        r = self.rng.random()
        return name if r < 0.7 else name.upper() if r < 0.85 else "`%s`" % (name if r < 0.95 else name.upper())

    def pick(self, xs):
        return xs[self.rng.randrange(len(xs))]

    def op(self, nullsafe=True):
        return self.pick(OPERATORS if nullsafe else OPERATORS[:-1])

    # ------------------------------------------------------------------ values
    def number(self, decimals=0.35):
        r = self.rng.random()
        if r < decimals:
            return self.pick(DEC_LITERALS)
        return self.pick(INT_LITERALS) if r < decimals + 0.45 else self.pick(DBL_LITERALS)

    def num_col(self):
        return self.col(self.pick("ldgi"))

    def cast(self, inner, target=None):
        return "%s(%s %s %s)" % (self.kw("CAST"), inner, self.kw("AS"), self.kw(target or self.pick(NUMERIC_CASTS)))

    def num_value(self, level=1):
        r = self.rng.random()
        if level == 0 or r < 0.5:
            return self.num_col() if r < 0.35 or level == 0 and r < 0.75 else self.number()
        if r < 0.8:
            q = self.rng.random()
            if q < 0.04:
                return self.cast(self.kw("NULL"))
            if q < 0.12:
                return self.cast(self.col("b"))
            if self.strings and q < 0.30:  # only DOUBLE is evaluated on the GPU; the rest is declined
                return self.cast(self.col("s"), "DOUBLE" if q < 0.27 else None)
            return self.cast(self.num_value(level - 1))
        return self.coalesce([self.num_col()] + [self.coalesce_arg(level - 1) for _ in range(self.rng.randrange(1, 3))])

    def coalesce_arg(self, level):
        r = self.rng.random()
        if r < 0.12:
            return self.kw("NULL")
        if r < 0.55:
            return self.number(decimals=0.12)
        return self.num_value(level)

    def coalesce(self, args):
        return "%s(%s)" % (self.kw("COALESCE"), ", ".join(args))

    def str_value(self):
        r = self.rng.random()
        if r < 0.55:
            return self.col("s")
        if r < 0.8:
            return self.pick(STR_LITERALS)
        args = [self.col("s")] + [self.pick([self.col("s"), self.kw("NULL")] + STR_LITERALS)
                                  for _ in range(self.rng.randrange(1, 3))]
        return self.coalesce(args)

    def bool_value(self):
        r = self.rng.random()
        if r < 0.6:
            return self.col("b")
        if r < 0.8:
            return self.kw(self.pick(["TRUE", "FALSE"]))
        if r < 0.9:
            return self.coalesce([self.col("b"), self.kw(self.pick(["TRUE", "FALSE", "NULL"]))])
        return self.cast(self.num_value(0), "BOOLEAN")

    # ------------------------------------------------------------------ atoms
    def in_list(self, left, item):
        items = [item() for _ in range(self.rng.randrange(1, 5))]
        if self.rng.random() < 0.3:
            items[self.rng.randrange(len(items))] = self.kw("NULL")
        neg = self.kw("NOT") + " " if self.rng.random() < 0.4 else ""
        return "%s %s%s (%s)" % (left, neg, self.kw("IN"), ", ".join(items))

    def between(self, left, bound):
        neg = self.kw("NOT") + " " if self.rng.random() < 0.3 else ""
        return "%s %s%s %s %s %s" % (left, neg, self.kw("BETWEEN"), bound(), self.kw("AND"), bound())

    def is_null(self, value):
        neg = " " + self.kw("NOT") if self.rng.random() < 0.4 else ""
        return "%s %s%s %s" % (value, self.kw("IS"), neg, self.kw("NULL"))

    def inline_form(self):
        """Exactly the shapes dq_api.cpp fast_form recognises (whether a text ends up inline is
        decided from its compiled program, not here)."""
        r = self.rng.random()
        c = self.col(self.pick("ldgi"))
        if r < 0.45:
            return "%s %s %s" % (c, self.op(False), self.number())
        if r < 0.65:
            return "%s %s %s" % (self.number(), self.op(False), c)
        if r < 0.8:
            return "%s %s %s" % (self.coalesce([c, self.number(0.1)]), self.op(False), self.number(0.2))
        if r < 0.92:
            return self.is_null(self.col(self.pick("ldgibs" if self.strings else "ldgib")))
        return self.col("b") if r < 0.97 else self.kw(self.pick(["TRUE", "FALSE"]))

    def numeric_atom(self):
        r = self.rng.random()
        if r < 0.42:
            a, b = self.num_value(), self.num_value()
            if self.rng.random() < 0.5:  # at least one side a plain column or literal
                b = self.number() if self.rng.random() < 0.7 else self.num_col()
            if self.rng.random() < 0.5:
                a, b = b, a
            return "%s %s %s" % (a, self.op(), b)
        if r < 0.57:
            return self.in_list(self.num_value(), lambda: self.number() if self.rng.random() < 0.85 else self.num_col())
        if r < 0.69:
            return self.between(self.num_value(), lambda: self.number() if self.rng.random() < 0.85 else self.num_col())
        if r < 0.78:
            return self.is_null(self.pick([self.num_value, self.bool_value])())
        if r < 0.84:  # comparisons with the NULL literal
            v, n = self.num_value(), self.kw("NULL")
            return "%s %s %s" % ((v, self.op(), n) if self.rng.random() < 0.5 else (n, self.op(), v))
        if r < 0.93:  # bare boolean forms
            return self.bool_value()
        q = self.rng.random()  # boolean comparisons (Spark 2.2 BooleanEquality: = and <=> only)
        if q < 0.4:
            return "%s %s %s" % (self.bool_value(), self.pick(["=", "==", "<=>", "!=", "<>"]), self.bool_value())
        if q < 0.6:
            return "%s %s %s" % (self.col("b"), self.pick(["=", "<=>"]), self.pick(["0", "1"]))
        if q < 0.8:
            return "%s %s %s" % (self.cast(self.col("b")), self.op(), self.number())
        return self.in_list(self.col("b"), lambda: self.kw(self.pick(["TRUE", "FALSE"])))

    def string_atom(self):
        r = self.rng.random()
        if r < 0.3:  # string equality and ordering (UTF8String.compareTo)
            return "%s %s %s" % (self.str_value(), self.op(), self.str_value())
        if r < 0.42:
            return self.in_list(self.str_value(), lambda: self.pick(STR_LITERALS))
        if r < 0.5:
            return self.between(self.str_value(), lambda: self.pick(STR_LITERALS))
        if r < 0.58:
            return self.is_null(self.str_value())
        if r < 0.9:  # PromoteStrings: the string side is Cast to double
            a = self.str_value()
            b = self.num_value() if self.rng.random() < 0.5 else self.number()
            if self.rng.random() < 0.15:
                return self.between(a, self.number)
            if self.rng.random() < 0.5:
                a, b = b, a
            return "%s %s %s" % (a, self.op(), b)
        if r < 0.95:
            n = self.kw("NULL")
            return "%s %s %s" % ((self.str_value(), self.op(), n) if self.rng.random() < 0.5 else (n, self.op(), self.str_value()))
        return "%s %s %s" % (self.str_value(), self.pick(["=", "<=>"]), self.bool_value())  # declined

    def atom(self):
        if self.rng.random() < 0.15:
            return self.inline_form()
        if self.strings and self.rng.random() < 0.55:
            return self.string_atom()
        return self.numeric_atom()

    # ------------------------------------------------------------------ boolean structure
    def pred(self, depth):
        """(text, binding): binding in atom / not / and / or decides where parentheses are needed."""
        r = self.rng.random()
        if depth == 0 or r < 0.35:
            return self.atom(), "atom"
        if r < 0.45:
            return "(%s)" % self.pred(depth - 1)[0], "atom"
        if r < 0.6:
            t, b = self.pred(depth - 1)
            return "%s %s" % (self.kw("NOT"), "(%s)" % t if b in ("and", "or") else t), "not"
        word = "AND" if r < 0.8 else "OR"
        parts = []
        for t, b in (self.pred(depth - 1), self.pred(depth - 1)):
            parts.append("(%s)" % t if word == "AND" and b == "or" or self.rng.random() < 0.15 else t)
        return (" %s " % self.kw(word)).join(parts), word.lower()


def generate(seed, count, family):
    """`count` predicate texts of `family` ("numeric" or "string"), a function of the seed alone.
    A quarter are bare inline forms (see the module docstring), the rest two levels deep."""
    if family not in ("numeric", "string"):
        raise ValueError(family)
    g = _Gen(random.Random(seed), family)
    return [g.inline_form() if g.rng.random() < 0.25 else g.pred(2)[0] for _ in range(count)]


# ---------------------------------------------------------------------- what a text contains
_STRING_RE = re.compile(r"'[^']*'")
_OP_RE = re.compile(r"<=>|<=|>=|!=|<>|==|<|>|=")
_CAST_RE = re.compile(r"\bAS\s+(\w+)\s*\)")
FEATURES = OPERATORS + ["IN", "NOT IN", "BETWEEN", "IS NULL", "COALESCE"] + ["CAST " + t for t in _CAST_TYPES]


def features(text):
    """The members of FEATURES that occur in `text`."""
    up = _STRING_RE.sub("''", text).upper()
    found = set(_OP_RE.findall(up))
    if re.search(r"\bNOT\s+IN\b", up):
        found.add("NOT IN")
    if re.search(r"(?<!NOT)\s+IN\s*\(", up):
        found.add("IN")
    for word, pat in (("BETWEEN", r"\bBETWEEN\b"), ("IS NULL", r"\bIS\s+NULL\b"), ("COALESCE", r"\bCOALESCE\s*\(")):
        if re.search(pat, up):
            found.add(word)
    found.update("CAST " + t for t in _CAST_RE.findall(up) if t in _CAST_TYPES)
    return [f for f in FEATURES if f in found]


# ---------------------------------------------------------------------- which device path
def is_inline(prog, dtypes):
    """True when the fused scan evaluates the compiled program inline (dq_api.cpp fast_form),
    False when dq_pred_kernel evaluates it into a row mask.  `dtypes[k]` is column k's dtype."""
    c = list(prog)
    lit = lambda ins: ins[0] in (L.DQ_P_LIT_INT, L.DQ_P_LIT_FLOAT)  # noqa: E731
    numeric = lambda ins: ins[0] == L.DQ_P_COLUMN and dtypes[ins[1]] not in ("bool", "string")  # noqa: E731
    integral = lambda ins: dtypes[ins[1]].startswith("int")  # noqa: E731
    compares = (L.DQ_P_EQ, L.DQ_P_NE, L.DQ_P_LT, L.DQ_P_LE, L.DQ_P_GT, L.DQ_P_GE)

    def literal_fits(ins, cmp_ins):  # an int64 comparison takes an integer literal only
        return cmp_ins[1] == L.DQ_CMP_AS_FLOAT64 or ins[0] == L.DQ_P_LIT_INT

    if len(c) == 1:
        return c[0][0] in (L.DQ_P_TRUE, L.DQ_P_FALSE) or (c[0][0] == L.DQ_P_COLUMN and dtypes[c[0][1]] == "bool")
    if len(c) == 2:
        return c[0][0] == L.DQ_P_COLUMN and c[1][0] in (L.DQ_P_IS_NULL, L.DQ_P_IS_NOT_NULL)
    if len(c) == 3 and c[2][0] in compares:
        for col, val in ((c[0], c[1]), (c[1], c[0])):
            if numeric(col) and lit(val):
                return (c[2][1] == L.DQ_CMP_AS_FLOAT64 or integral(col)) and literal_fits(val, c[2])
        return False
    if len(c) == 5 and numeric(c[0]) and lit(c[1]) and c[2][0] == L.DQ_P_COALESCE and lit(c[3]) and c[4][0] in compares:
        return ((c[4][1] == L.DQ_CMP_AS_FLOAT64 or integral(c[0])) and literal_fits(c[3], c[4])
                and literal_fits(c[1], c[4]))
    return False
