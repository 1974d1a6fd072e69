"""Generated regular expressions for the PatternMatch tests (test_regex_generated.py,
test_gpu_regex_generated.py): a seeded generator of patterns from the supported subset, kept as
ASTs; a sampler of strings that match, nearly match and do not match; and three rewrites that keep
a pattern's language.  Test infrastructure: it imports neither the library nor the package.

The oracle is pattern_cases.oracle (Python's `re`), so the generator keeps to what Java and Python
read alike:

  1. Every concatenation keeps one item whose minimum repeat is >= 1: no pattern matches "".
  2. No syntax on which the two differ: no quantifier on a quantifier, no `[` or `&&` inside a
     class (nor `--`, `||`, `~~`, which Python reserves: `-`, `|` and `~` are escaped there), no
     bare `{`, no \\x{..}, octal, \\e \\a \\cX \\Z \\h \\v \\R.
  3. U+000D, U+0085, U+2028 and U+2029 occur in no pattern and no string (Java's line terminators:
     pattern_cases.JAVA_LINE_CASES is their test).
  4. The oracle backtracks, so its work is bounded BY CONSTRUCTION.  A seed that hangs `re` is a
     broken test, not a slow one: a hang cannot be told from a long run and stops the whole suite.
       - An unbounded quantifier (* + {n,}) is applied only to a single character or to a group of
         fixed length: no alternation, no `?`, no other variable quantifier inside it.  ((\\w{1,3})+x
         has no nested unbounded quantifier and still takes tribonacci(40) steps to fail.)
       - No unbounded quantifier stands inside a group that is itself repeated.
       - `paths` below bounds the ways a pattern can split one string (alternatives add, items of a
         concatenation and copies of a repetition multiply, an unbounded quantifier counts 16); a
         pattern above MAX_PATHS is drawn again.  That allows at most four unbounded quantifiers.
       - Every string is at most MAX_CHARS = 40 characters.
"""
import random

MAX_CHARS = 40
MAX_PATHS = 100000
UNBOUNDED_PATHS = 16

BANNED = "\r\u0085\u2028\u2029"
META = ".*+?()[]{}|^$\\"
CLASS_ESCAPED = "\\]^-|~"            # escaped inside a class (rule 2)
CONTROL = {"\t": "\\t", "\n": "\\n", "\f": "\\f"}
LETTERS = "abcdexyzAQZ"
DIGITS = "01579"
PUNCT = "-_@/:,;!#% =<>~'\"&"
TWO, THREE, FOUR = "éßñàÿω", "例子测一鿿➡€", "\U0001F600\U0001D11E\U0001F60F"
UNIVERSE = LETTERS + DIGITS + PUNCT + META + "\t\n\f" + TWO + THREE + FOUR + "fgmQ_\x7f÷一"
RANGES = [("a", "f"), ("0", "9"), ("A", "Z"), ("a", "z"), ("0", "5"), ("m", "z"), ("à", "ÿ"), ("一", "鿿"),
          ("α", "ω"), ("\U0001F600", "\U0001F60F"), (" ", "/")]
PERL = {"d": "0123456789", "s": " \t\n\x0b\f\r",
        "w": "abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789_"}
assert not set(BANNED) & set(UNIVERSE)


def perl_has(letter, ch):
    inside = ch in PERL[letter.lower()]
    return inside if letter.islower() else not inside


# ------------------------------------------------------------------------------ the AST
class Lit:
    def __init__(self, ch, form):
        self.ch, self.form = ch, form   # form: raw | esc | x | u | ctl

    def has(self, ch):
        return ch == self.ch


class Dot:
    def has(self, ch):
        return ch != "\n"


class Perl:
    def __init__(self, letter):
        self.letter = letter

    def has(self, ch):
        return perl_has(self.letter, ch)


class Cls:
    def __init__(self, neg, items):
        self.neg, self.items = neg, items   # ("c", ch) | ("r", lo, hi) | ("p", letter)

    def has(self, ch):
        inside = any(ch == it[1] if it[0] == "c" else it[1] <= ch <= it[2] if it[0] == "r" else perl_has(it[1], ch)
                     for it in self.items)
        return inside != self.neg


class Group:
    def __init__(self, capture, alts):
        self.capture, self.alts = capture, alts   # alts: lists of items


class Rep:
    def __init__(self, atom, lo, hi, lazy):
        self.atom, self.lo, self.hi, self.lazy = atom, lo, hi, lazy   # hi None: unbounded


class Pattern:
    def __init__(self, branches):
        self.branches = branches   # (caret, items, dollar)

    def text(self, **how):
        return "|".join(("^" if c else "") + "".join(render(i, **how) for i in items) + ("$" if d else "")
                        for c, items, d in self.branches)


def _u(ch):
    return "\\u%04x" % ord(ch)


def _class_char(ch, uclass):
    if uclass and ord(ch) < 0x10000:
        return _u(ch)
    if ch in CONTROL:
        return CONTROL[ch]
    return "\\" + ch if ch in CLASS_ESCAPED else ch


def render(node, flip_lazy=False, noncapturing=False, uclass=False):
    """The pattern text of `node`.  The three flags are the rewrites that keep the language: every
    greedy quantifier lazy and every lazy one greedy, every (..) a (?:..), every class member
    (up to U+FFFF: \\u has four digits) as a \\uhhhh escape."""
    how = dict(flip_lazy=flip_lazy, noncapturing=noncapturing, uclass=uclass)
    if isinstance(node, Lit):
        return {"raw": node.ch, "esc": "\\" + node.ch, "x": "\\x%02x" % ord(node.ch), "u": _u(node.ch),
                "ctl": CONTROL.get(node.ch)}[node.form]
    if isinstance(node, Dot):
        return "."
    if isinstance(node, Perl):
        return "\\" + node.letter
    if isinstance(node, Cls):
        out = []
        for it in node.items:
            if it[0] == "c":
                out.append(_class_char(it[1], uclass))
            elif it[0] == "r":
                out.append(_class_char(it[1], uclass) + "-" + _class_char(it[2], uclass))
            else:
                out.append("\\" + it[1])
        return "[" + ("^" if node.neg else "") + "".join(out) + "]"
    if isinstance(node, Group):
        body = "|".join("".join(render(i, **how) for i in alt) for alt in node.alts)
        return ("(" if node.capture and not noncapturing else "(?:") + body + ")"
    lo, hi = node.lo, node.hi
    q = ("?" if (lo, hi) == (0, 1) else "*" if (lo, hi) == (0, None) else "+" if (lo, hi) == (1, None) else
         "{%d}" % lo if lo == hi else "{%d,}" % lo if hi is None else "{%d,%d}" % (lo, hi))
    return render(node.atom, **how) + q + ("?" if node.lazy != flip_lazy else "")


def paths(node):
    """Rule 4's bound on the ways `node` can split one string."""
    if isinstance(node, Pattern):
        return sum(paths(items) for _, items, _ in node.branches)
    if isinstance(node, list):
        p = 1
        for i in node:
            p *= paths(i)
        return p
    if isinstance(node, Group):
        return sum(paths(a) for a in node.alts)
    if isinstance(node, Rep):
        if node.hi is None:
            return UNBOUNDED_PATHS
        c = paths(node.atom)
        return sum(c ** k for k in range(node.lo, node.hi + 1))
    return 1


def min_chars(node):
    if isinstance(node, list):
        return sum(min_chars(i) for i in node)
    if isinstance(node, Group):
        return min(min_chars(a) for a in node.alts)
    if isinstance(node, Rep):
        return node.lo * min_chars(node.atom)
    return 1


def atoms(node):
    """Every single-character matcher of the pattern."""
    if isinstance(node, Pattern):
        for _, items, _ in node.branches:
            yield from atoms(items)
    elif isinstance(node, list):
        for i in node:
            yield from atoms(i)
    elif isinstance(node, Group):
        for a in node.alts:
            yield from atoms(a)
    elif isinstance(node, Rep):
        yield from atoms(node.atom)
    else:
        yield node


# ------------------------------------------------------------------------------ the generator
class _Ctx:
    def __init__(self, fixed=False, repeated=False):
        self.fixed, self.repeated = fixed, repeated   # inside an unbounded / a repeated group


def _literal(rng):
    u = rng.random()
    if u < 0.55:
        ch = rng.choice(LETTERS + DIGITS)
    elif u < 0.67:
        ch = rng.choice(PUNCT)
    elif u < 0.77:
        return Lit(rng.choice(META), "esc")
    elif u < 0.82:
        ch = rng.choice("\t\n\f")
        return Lit(ch, rng.choice(["ctl", "ctl", "x", "u"]))
    else:
        ch = rng.choice(TWO + THREE + FOUR)
    forms = ["raw"] * 5
    if ord(ch) < 0x100:
        forms.append("x")
    if ord(ch) < 0x10000:
        forms.append("u")
    if ch in PUNCT:
        forms.append("esc")   # an escaped non-alphabetic character is itself
    return Lit(ch, rng.choice(forms))


def _class(rng):
    items = []
    for _ in range(rng.choice([1, 2, 2, 3, 3, 4])):
        u = rng.random()
        if u < 0.45:
            pool = LETTERS + DIGITS + PUNCT + ".*+?(){}|^$\\]-" + "\t\n" + TWO + THREE + FOUR
            items.append(("c", rng.choice(pool.replace("&", "").replace("[", ""))))
        elif u < 0.8:
            items.append(("r",) + rng.choice(RANGES))
        else:
            items.append(("p", rng.choice("dswDSW" if rng.random() < 0.3 else "dsw")))
    return Cls(rng.random() < 0.3, items)


def _quantifier(rng, ctx, on_group):
    """(lo, hi, lazy) or None."""
    if rng.random() >= (0.45 if not on_group else 0.55):
        return None
    lazy = rng.random() < 0.25
    if ctx.fixed:
        return (rng.choice([1, 2, 2, 3]),) * 2 + (lazy,)
    kind = rng.choice(["?", "*", "+", "{n}", "{n}", "{n,}", "{n,m}", "{n,m}"])
    if ctx.repeated and kind in ("*", "+", "{n,}"):
        kind = "{n,m}"
    if kind == "?":
        return 0, 1, lazy
    if kind == "*":
        return 0, None, lazy
    if kind == "+":
        return 1, None, lazy
    n = rng.choice([0, 1, 1, 2, 2, 3, 4, 5] if kind != "{n}" else [1, 2, 2, 3, 3, 4, 5, 6, 8])
    if kind == "{n}":
        return n, n, lazy
    if kind == "{n,}":
        return min(n, 3), None, lazy
    return n, n + rng.choice([1, 1, 2, 3, 5]), lazy


def _item(rng, depth, ctx):
    u = rng.random()
    if u < 0.22 and depth < 2:
        q = _quantifier(rng, ctx, True)
        inner = _Ctx(fixed=ctx.fixed or (q is not None and q[1] is None),
                     repeated=ctx.repeated or (q is not None and (q[1] is None or q[1] > 1)))
        n_alts = 1 if inner.fixed else rng.choice([1, 1, 2, 2, 3])
        atom = Group(rng.random() < 0.5, [_cat(rng, depth + 1, inner, rng.choice([1, 2, 2, 3])) for _ in range(n_alts)])
    else:
        atom = (_literal(rng) if u < 0.62 else _class(rng) if u < 0.84 else
                Perl(rng.choice("dswDSW" if rng.random() < 0.35 else "dsw")) if u < 0.94 else Dot())
        q = _quantifier(rng, ctx, False)
    if q is None or q[:2] == (1, 1):
        return atom
    return Rep(atom, *q)


def _cat(rng, depth, ctx, n):
    items = [_item(rng, depth, ctx) for _ in range(n)]
    if all(isinstance(i, Rep) and i.lo == 0 for i in items):   # rule 1
        k = rng.randrange(len(items))
        items[k].lo = 1
        if items[k].hi == 1:
            items[k] = items[k].atom
    return items


def generate(seed, count):
    """`count` patterns (Pattern objects) of the supported subset, the same for the same seed."""
    rng = random.Random(seed)
    out = []
    while len(out) < count:
        branches = []
        for _ in range(rng.choice([1, 1, 1, 1, 2, 2, 3])):
            caret, dollar = rng.random() < 0.2, rng.random() < 0.2
            branches.append((caret, _cat(rng, 0, _Ctx(), rng.choice([2, 3, 3, 4, 4, 5, 6])), dollar))
        p = Pattern(branches)
        if paths(p) > MAX_PATHS or min(min_chars(items) for _, items, _ in branches) > MAX_CHARS // 2:
            continue
        out.append(p)
    return out


# ------------------------------------------------------------------------------ the sampler
def _pick(rng, atom, alphabet):
    """One character `atom` matches."""
    if isinstance(atom, Lit):
        return atom.ch
    if isinstance(atom, Cls) and not atom.neg and rng.random() < 0.8:
        it = rng.choice(atom.items)
        if it[0] == "c":
            return it[1]
        if it[0] == "r":
            for _ in range(8):
                ch = chr(rng.randint(ord(it[1]), ord(it[2])))
                if ch not in BANNED:
                    return ch
            return it[1]
        if it[1].islower():
            ch = rng.choice(PERL[it[1]])
            return ch if ch != "\r" else " "
    if isinstance(atom, Perl) and atom.letter.islower():
        ch = rng.choice(PERL[atom.letter])
        return ch if ch != "\r" else " "
    for _ in range(64):
        ch = rng.choice(alphabet)
        if atom.has(ch):
            return ch
    return next((ch for ch in UNIVERSE if atom.has(ch)), "a")


def _sample(rng, node, alphabet):
    if isinstance(node, list):
        return "".join(_sample(rng, i, alphabet) for i in node)
    if isinstance(node, Group):
        return _sample(rng, rng.choice(node.alts), alphabet)
    if isinstance(node, Rep):
        spare = 3 if node.hi is None else min(node.hi - node.lo, 3)
        count = node.lo + rng.randint(0, spare)
        if rng.random() < 0.3:   # the bounds themselves, and one copy beyond the upper one
            count = rng.choice([node.lo, node.lo + 4] if node.hi is None else [node.lo, node.hi, node.hi, node.hi + 1])
        return "".join(_sample(rng, node.atom, alphabet) for _ in range(count))
    return _pick(rng, node, alphabet)


def alphabet_of(pattern):
    """The pattern's own characters first (so that near-misses are likely), then the universe."""
    own = []
    for a in atoms(pattern):
        if isinstance(a, Lit):
            own.append(a.ch)
        elif isinstance(a, Cls):
            for it in a.items:
                own += [it[1]] if it[0] == "c" else [it[1], it[2]] if it[0] == "r" else []
    return "".join(dict.fromkeys(own)) * 3 + UNIVERSE


def complement_alphabet(pattern):
    """ASCII characters that no single-character matcher of the pattern takes ('#' if all are taken)."""
    all_atoms = list(atoms(pattern))
    out = [ch for ch in "#%=<>;qQ7z_ ,'!" if not any(a.has(ch) for a in all_atoms)]
    return out or ["#"]


def strings(pattern, seed, n_match=14, n_edit=14, n_random=8):
    """About 40 strings of at most MAX_CHARS characters: matches sampled from the AST (repetitions
    at their bounds among them, and now and then one copy past the upper bound) with and without a
    random prefix and suffix (rarely on an anchored side), one to three random edits of those,
    random strings, "" and "\\n"."""
    rng = random.Random(seed)
    alphabet = alphabet_of(pattern)
    noise = lambda k: "".join(rng.choice(alphabet) for _ in range(rng.randint(1, k)))  # noqa: E731
    matched = []
    for _ in range(n_match):
        caret, items, dollar = rng.choice(pattern.branches)
        s = _sample(rng, items, alphabet)
        if rng.random() < 0.6:
            if rng.random() < (0.1 if caret else 0.6):
                s = noise(8) + s
            if rng.random() < (0.1 if dollar else 0.6):
                s = s + noise(8)
        elif dollar and rng.random() < 0.3:
            s += "\n"
        matched.append(s[:MAX_CHARS])
    out = list(matched)
    for _ in range(n_edit):
        s = list(rng.choice(matched))
        for _ in range(rng.randint(1, 3)):
            op, i = rng.randrange(3), rng.randrange(len(s) + 1)
            if op == 0 and s:
                s[min(i, len(s) - 1)] = rng.choice(alphabet)
            elif op == 1 and s:
                del s[min(i, len(s) - 1)]
            else:
                s.insert(i, rng.choice(alphabet))
        out.append("".join(s)[:MAX_CHARS])
    for _ in range(n_random):
        out.append("".join(rng.choice(alphabet) for _ in range(rng.randint(1, MAX_CHARS))))
    out += ["", "\n"]
    assert all(len(s) <= MAX_CHARS and not set(s) & set(BANNED) for s in out)
    return out
