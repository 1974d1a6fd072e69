// dq_regex.cpp -- the host compiler of dq_regex.h: Java pattern text -> AST -> Thompson NFA over
// UTF-8 bytes -> search DFA by subset construction, with a byte -> column map.  Plain C++ (no HIP):
// tools/regex_fuzz.cpp links it under the host sanitizers.
//
// Java rules kept (java.util.regex.Pattern, JDK 8, no flags):
//   - `.` is one code point (a 1-4 byte sequence) other than \n, \r, U+0085, U+2028, U+2029;
//   - \d \s \w and their complements are ASCII-only; a negated class matches every other code point;
//   - `$` (Pattern.Dollar without MULTILINE) holds at the end of input, before a final \n not
//     preceded by \r, before a final \r, U+0085, U+2028 or U+2029, and before a final \r\n;
//   - lazy quantifiers accept the language of the greedy ones.
// In the find-non-empty mode (PatternMatch) a pattern that can match the empty string is declined:
// its leftmost match may be empty where a later one is not, which a DFA cannot tell
// (regexp_extract(...) != "" needs a NON-empty group 0).  The find mode (RLIKE: Matcher.find(0), any
// match) answers such patterns; compile_like builds the whole-value DFA of a SQL LIKE pattern from
// its own text.  All three share the subset construction and the image format.
#include "dq_regex.h"

#include <algorithm>
#include <cstring>
#include <map>
#include <utility>

namespace dq {
namespace regex {

namespace {

typedef std::pair<uint32_t, uint32_t> Range;  // code points, inclusive
constexpr uint32_t kMaxCp = 0x10FFFF;

enum AstKind { A_EMPTY, A_CLASS, A_CAT, A_ALT, A_REP };

struct Ast {
  int kind = A_EMPTY;
  std::vector<Range> ranges;  // A_CLASS (sorted, disjoint)
  std::vector<int> kids;      // A_CAT / A_ALT / A_REP (one)
  int min = 0, max = 0;       // A_REP; max < 0 = unbounded
};

struct Branch {  // one branch of the top-level alternation
  int ast;
  bool caret, dollar;
};

void normalize(std::vector<Range>& r) {
  std::sort(r.begin(), r.end());
  std::vector<Range> o;
  for (const Range& x : r) {
    if (!o.empty() && x.first <= o.back().second + 1) o.back().second = std::max(o.back().second, x.second);
    else o.push_back(x);
  }
  r.swap(o);
}

void negate(std::vector<Range>& r) {
  normalize(r);
  std::vector<Range> o;
  uint32_t next = 0;
  for (const Range& x : r) {
    if (x.first > next) o.push_back(Range(next, x.first - 1));
    next = x.second + 1;
  }
  if (next <= kMaxCp) o.push_back(Range(next, kMaxCp));
  r.swap(o);
}

struct Parser {
  const uint8_t* p;
  int32_t n, at = 0;
  std::vector<Ast> ast;
  std::string err;
  bool failed = false;

  bool fail(const std::string& what, int32_t where) {
    if (!failed) err = "regex: " + what + " at offset " + std::to_string(where) + " is not supported on the GPU path";
    failed = true;
    return false;
  }
  int node(int kind) {
    ast.push_back(Ast());
    ast.back().kind = kind;
    return (int)ast.size() - 1;
  }
  bool eof() const { return at >= n; }
  // the code point at `at` (UTF-8 of the pattern text); advances
  bool next_cp(uint32_t* cp) {
    const int32_t start = at;
    const uint32_t b = p[at];
    int len = b < 0x80 ? 1 : (b >> 5) == 6 ? 2 : (b >> 4) == 14 ? 3 : (b >> 3) == 30 ? 4 : 0;
    if (len == 0 || at + len > n) return fail("invalid UTF-8 in the pattern", start);
    uint32_t v = len == 1 ? b : b & (0xFFu >> (len + 1));
    for (int k = 1; k < len; ++k) {
      if ((p[at + k] & 0xC0) != 0x80) return fail("invalid UTF-8 in the pattern", start);
      v = (v << 6) | (p[at + k] & 0x3Fu);
    }
    static const uint32_t kMin[5] = {0, 0, 0x80, 0x800, 0x10000};
    if (v < kMin[len] || v > kMaxCp || (v >= 0xD800 && v <= 0xDFFF)) return fail("invalid UTF-8 in the pattern", start);
    at += len;
    *cp = v;
    return true;
  }
  static int hex(uint32_t c) {
    if (c >= '0' && c <= '9') return (int)(c - '0');
    if (c >= 'a' && c <= 'f') return (int)(c - 'a' + 10);
    if (c >= 'A' && c <= 'F') return (int)(c - 'A' + 10);
    return -1;
  }
  static void perl_class(uint32_t c, std::vector<Range>& r) {
    std::vector<Range> s;
    switch (c | 0x20) {
      case 'd': s.push_back(Range('0', '9')); break;
      case 's':
        s.push_back(Range('\t', '\r'));  // \t \n \x0B \f \r
        s.push_back(Range(' ', ' '));
        break;
      default:  // 'w'
        s.push_back(Range('0', '9'));
        s.push_back(Range('A', 'Z'));
        s.push_back(Range('_', '_'));
        s.push_back(Range('a', 'z'));
        break;
    }
    if (c < 'a') negate(s);
    r.insert(r.end(), s.begin(), s.end());
  }
  // After a backslash (at = the escape letter).  *single: the escape is one code point (*cp), else
  // a class appended to r.
  bool escape(std::vector<Range>& r, bool* single, uint32_t* cp) {
    const int32_t where = at - 1;
    if (eof()) return fail("a trailing backslash", where);
    uint32_t c;
    if (!next_cp(&c)) return false;
    *single = true;
    switch (c) {
      case 't': *cp = '\t'; return true;
      case 'n': *cp = '\n'; return true;
      case 'r': *cp = '\r'; return true;
      case 'f': *cp = '\f'; return true;
      case 'x': case 'u': {
        const int digits = c == 'x' ? 2 : 4;
        uint32_t v = 0;
        for (int k = 0; k < digits; ++k) {
          const int h = eof() ? -1 : hex(p[at]);
          if (h < 0) return fail(c == 'x' ? "the escape \\x without two hex digits" : "the escape \\u without four hex digits", where);
          v = v * 16 + (uint32_t)h;
          ++at;
        }
        if (v >= 0xD800 && v <= 0xDFFF) return fail("a surrogate \\u escape", where);
        *cp = v;
        return true;
      }
      case 'd': case 'D': case 's': case 'S': case 'w': case 'W':
        *single = false;
        perl_class(c, r);
        return true;
      default: break;
    }
    if (c >= '1' && c <= '9') return fail("a back-reference", where);
    if (c == 'b' || c == 'B' || c == 'A' || c == 'z' || c == 'Z' || c == 'G')
      return fail(std::string("the boundary matcher \\") + (char)c, where);
    if (c == 'p' || c == 'P') return fail("a \\p{..} property class", where);
    if (c == 'k') return fail("a named back-reference", where);
    if ((c >= 'a' && c <= 'z') || (c >= 'A' && c <= 'Z') || c == '0')
      return fail(std::string("the escape \\") + (char)c, where);
    *cp = c;  // an escaped metacharacter or any other non-alphabetic character: itself
    return true;
  }

  bool parse_class(int* out) {  // at = just past '['
    const int32_t where = at - 1;
    bool neg = false;
    if (!eof() && p[at] == '^') {
      neg = true;
      ++at;
    }
    std::vector<Range> r;
    bool first = true;
    for (;;) {
      if (eof()) return fail("an unclosed character class", where);
      if (p[at] == ']') {
        if (first) return fail("a character class that starts with ]", where);
        ++at;
        break;
      }
      first = false;
      if (p[at] == '[') return fail("a nested character class", at);
      if (p[at] == '&' && at + 1 < n && p[at + 1] == '&') return fail("a character class intersection", at);
      bool single = true;
      uint32_t lo = 0;
      const int32_t item = at;
      if (p[at] == '\\') {
        ++at;
        if (!escape(r, &single, &lo)) return false;
      } else if (!next_cp(&lo)) {
        return false;
      }
      if (!single) continue;
      if (at + 1 < n && p[at] == '-' && p[at + 1] != ']') {
        ++at;
        if (p[at] == '[') return fail("a nested character class", at);
        uint32_t hi = 0;
        bool hs = true;
        if (p[at] == '\\') {
          ++at;
          std::vector<Range> tmp;
          if (!escape(tmp, &hs, &hi)) return false;
          if (!hs) return fail("a class as the end of a character range", item);
        } else if (!next_cp(&hi)) {
          return false;
        }
        if (hi < lo) return fail("a reversed character range", item);
        r.push_back(Range(lo, hi));
      } else {
        r.push_back(Range(lo, lo));
      }
    }
    if (neg) negate(r);
    else normalize(r);
    const int id = node(A_CLASS);
    ast[id].ranges = r;
    *out = id;
    return true;
  }

  // A quantifier after atom `a` (if any): wraps it.
  bool parse_quantifier(int* a) {
    if (eof()) return true;
    const int32_t where = at;
    int mn, mx;
    const uint8_t c = p[at];
    if (c == '?') { mn = 0; mx = 1; ++at; }
    else if (c == '*') { mn = 0; mx = -1; ++at; }
    else if (c == '+') { mn = 1; mx = -1; ++at; }
    else if (c == '{') {
      ++at;
      auto number = [&](int* v) -> bool {
        if (eof() || p[at] < '0' || p[at] > '9') return false;
        int64_t x = 0;
        while (!eof() && p[at] >= '0' && p[at] <= '9') {
          x = x * 10 + (p[at] - '0');
          if (x > kMaxRepeat) x = kMaxRepeat + 1;
          ++at;
        }
        *v = (int)x;
        return true;
      };
      if (!number(&mn)) return fail("a malformed {n,m} repetition", where);
      mx = mn;
      if (!eof() && p[at] == ',') {
        ++at;
        mx = -1;
        if (!eof() && p[at] != '}' && !number(&mx)) return fail("a malformed {n,m} repetition", where);
      }
      if (eof() || p[at] != '}') return fail("a malformed {n,m} repetition", where);
      ++at;
      if (mn > kMaxRepeat || mx > kMaxRepeat)
        return fail("a repetition count above " + std::to_string(kMaxRepeat), where);
      if (mx >= 0 && mx < mn) return fail("a reversed {n,m} repetition", where);
    } else {
      return true;
    }
    if (!eof() && p[at] == '+') return fail("a possessive quantifier", where);
    if (!eof() && p[at] == '?') ++at;  // lazy: the same language
    if (!eof() && (p[at] == '?' || p[at] == '*' || p[at] == '+' || p[at] == '{'))
      return fail("a quantifier applied to a quantifier", at);
    const int id = node(A_REP);
    ast[id].kids.push_back(*a);
    ast[id].min = mn;
    ast[id].max = mx;
    *a = id;
    return true;
  }

  // One alternative (items up to '|' or ')').  top: a branch of the whole pattern, where ^ may
  // come first and $ last.
  bool parse_branch(int depth, bool top, Branch* br) {
    const int cat = node(A_CAT);
    bool caret = false, dollar = false;
    int items = 0;
    while (!eof() && p[at] != '|' && p[at] != ')') {
      const int32_t where = at;
      if (dollar) return fail("an item after $ (the anchor is supported only as the last item)", where);
      const uint8_t c = p[at];
      int a = -1;
      if (c == '^') {
        if (!top || items > 0 || caret)
          return fail("the anchor ^ anywhere but first in the pattern or a top-level alternative", where);
        ++at;
        caret = true;
        if (!eof() && (p[at] == '?' || p[at] == '*' || p[at] == '+' || p[at] == '{'))
          return fail("a quantifier applied to an anchor", at);
        continue;
      }
      if (c == '$') {
        if (!top) return fail("the anchor $ anywhere but last in the pattern or a top-level alternative", where);
        ++at;
        dollar = true;
        if (!eof() && (p[at] == '?' || p[at] == '*' || p[at] == '+' || p[at] == '{'))
          return fail("a quantifier applied to an anchor", at);
        continue;
      }
      if (c == '?' || c == '*' || c == '+' || c == '{') return fail("a dangling quantifier", where);
      if (c == '(') {
        ++at;
        if (!eof() && p[at] == '?') {
          if (at + 1 < n && p[at + 1] == ':') {
            at += 2;
          } else {
            const uint8_t k = at + 1 < n ? p[at + 1] : 0;
            const uint8_t k2 = at + 2 < n ? p[at + 2] : 0;
            if (k == '=' || k == '!' || (k == '<' && (k2 == '=' || k2 == '!'))) return fail("a look-around group", where);
            if (k == '<') return fail("a named group", where);
            if (k == '>') return fail("an atomic group", where);
            return fail("an inline flag group", where);
          }
        }
        if (depth + 1 > kMaxDepth) return fail("groups nested deeper than " + std::to_string(kMaxDepth), where);
        if (!parse_alt(depth + 1, &a)) return false;
        if (eof() || p[at] != ')') return fail("an unclosed group", where);
        ++at;
      } else if (c == '[') {
        ++at;
        if (!parse_class(&a)) return false;
      } else if (c == '.') {
        ++at;
        a = node(A_CLASS);
        std::vector<Range> r;
        r.push_back(Range('\n', '\n'));
        r.push_back(Range('\r', '\r'));
        r.push_back(Range(0x85, 0x85));
        r.push_back(Range(0x2028, 0x2029));
        negate(r);
        ast[a].ranges = r;
      } else if (c == '\\') {
        ++at;
        std::vector<Range> r;
        bool single = true;
        uint32_t cp = 0;
        if (!escape(r, &single, &cp)) return false;
        if (single) r.push_back(Range(cp, cp));
        normalize(r);
        a = node(A_CLASS);
        ast[a].ranges = r;
      } else {
        uint32_t cp;
        if (!next_cp(&cp)) return false;
        a = node(A_CLASS);
        ast[a].ranges.push_back(Range(cp, cp));
      }
      if (!parse_quantifier(&a)) return false;
      ast[cat].kids.push_back(a);
      ++items;
    }
    br->ast = cat;
    br->caret = caret;
    br->dollar = dollar;
    return true;
  }

  bool parse_alt(int depth, int* out) {  // inside a group
    const int alt = node(A_ALT);
    for (;;) {
      Branch br;
      if (!parse_branch(depth, false, &br)) return false;
      ast[alt].kids.push_back(br.ast);
      if (!eof() && p[at] == '|') {
        ++at;
        continue;
      }
      break;
    }
    *out = alt;
    return true;
  }

  bool parse_top(std::vector<Branch>* branches) {
    for (;;) {
      Branch br;
      if (!parse_branch(0, true, &br)) return false;
      branches->push_back(br);
      if (eof()) return true;
      if (p[at] == ')') return fail("an unmatched )", at);
      ++at;  // '|'
    }
  }

  bool nullable(int id) const {
    const Ast& a = ast[id];
    switch (a.kind) {
      case A_EMPTY: return true;
      case A_CLASS: return false;
      case A_CAT:
        for (int k : a.kids) if (!nullable(k)) return false;
        return true;
      case A_ALT:
        for (int k : a.kids) if (nullable(k)) return true;
        return false;
      default: return a.min == 0 || nullable(a.kids[0]);
    }
  }
};

// ------------------------------------------------------------------------------ NFA
enum NodeKind : uint8_t { N_EPS, N_BYTE, N_MATCH, N_END, N_COND };

struct Node {
  uint8_t kind = N_EPS, lo = 0, hi = 0;
  int out = -1;           // N_BYTE: target; N_COND: target taken unless the previous byte was \r
  int tag = 0;            // compile_like: 2 * (number of % before the node) + (1: inside that %'s loop)
  std::vector<int> eps;   // N_EPS
};

struct Nfa {
  std::vector<Node> nodes;
  bool failed = false;
  int cur_tag = 0;  // stamped on every node added

  int add(uint8_t kind) {
    if ((int)nodes.size() >= kMaxNfaNodes) {
      failed = true;
      return 0;
    }
    nodes.push_back(Node());
    nodes.back().kind = kind;
    nodes.back().tag = cur_tag;
    return (int)nodes.size() - 1;
  }
  // from --[one code point]--> to, for LIKE's `_` and `%`: a lead byte and the continuation bytes
  // its length asks for.  On valid UTF-8 that is exactly "any code point"; the three continuation
  // nodes are shared by the lead classes, so a subset carries at most three states per position.
  void any_cp(int from, int to) {
    byte_edge(from, 0x00, 0x7F, to);
    const int c1 = add(N_EPS), c2 = add(N_EPS), c3 = add(N_EPS);
    if (failed) return;
    byte_edge(from, 0xC0, 0xDF, c1);
    byte_edge(from, 0xE0, 0xEF, c2);
    byte_edge(from, 0xF0, 0xF7, c3);
    byte_edge(c3, 0x80, 0xBF, c2);
    byte_edge(c2, 0x80, 0xBF, c1);
    byte_edge(c1, 0x80, 0xBF, to);
  }
  void eps(int from, int to) {
    if (!failed) nodes[from].eps.push_back(to);
  }
  // from --[lo-hi]--> to
  void byte_edge(int from, uint8_t lo, uint8_t hi, int to) {
    const int b = add(N_BYTE);
    if (failed) return;
    nodes[b].lo = lo;
    nodes[b].hi = hi;
    nodes[b].out = to;
    eps(from, b);
  }
  void seq(int from, const uint8_t* lo, const uint8_t* hi, int len, int to) {
    int cur = from;
    for (int k = 0; k < len && !failed; ++k) {
      const int nxt = k + 1 == len ? to : add(N_EPS);
      byte_edge(cur, lo[k], hi[k], nxt);
      cur = nxt;
    }
  }
  static int encode(uint32_t cp, uint8_t* b) {
    if (cp < 0x80) { b[0] = (uint8_t)cp; return 1; }
    if (cp < 0x800) { b[0] = (uint8_t)(0xC0 | (cp >> 6)); b[1] = (uint8_t)(0x80 | (cp & 0x3F)); return 2; }
    if (cp < 0x10000) {
      b[0] = (uint8_t)(0xE0 | (cp >> 12)); b[1] = (uint8_t)(0x80 | ((cp >> 6) & 0x3F)); b[2] = (uint8_t)(0x80 | (cp & 0x3F));
      return 3;
    }
    b[0] = (uint8_t)(0xF0 | (cp >> 18)); b[1] = (uint8_t)(0x80 | ((cp >> 12) & 0x3F));
    b[2] = (uint8_t)(0x80 | ((cp >> 6) & 0x3F)); b[3] = (uint8_t)(0x80 | (cp & 0x3F));
    return 4;
  }
  // The code points lo..hi as sequences of byte ranges (split where the encoded length or a
  // continuation-byte boundary changes, as RE2's and utf8-ranges' compilers do).
  void cp_range(int from, uint32_t lo, uint32_t hi, int to, int depth = 0) {
    if (failed || lo > hi) return;
    if (depth > 16) {  // (the splits above nest a handful deep; a bound that declines, like every other)
      failed = true;
      return;
    }
    static const uint32_t kLenMax[3] = {0x7F, 0x7FF, 0xFFFF};
    for (uint32_t m : kLenMax)
      if (lo <= m && hi > m) {
        cp_range(from, lo, m, to, depth + 1);
        cp_range(from, m + 1, hi, to, depth + 1);
        return;
      }
    if (hi < 0x80) {
      byte_edge(from, (uint8_t)lo, (uint8_t)hi, to);
      return;
    }
    for (int i = 1; i < 4; ++i) {
      const uint32_t m = (1u << (6 * i)) - 1;
      if ((lo & ~m) != (hi & ~m)) {
        if ((lo & m) != 0) {
          cp_range(from, lo, lo | m, to, depth + 1);
          cp_range(from, (lo | m) + 1, hi, to, depth + 1);
          return;
        }
        if ((hi & m) != m) {
          cp_range(from, lo, (hi & ~m) - 1, to, depth + 1);
          cp_range(from, hi & ~m, hi, to, depth + 1);
          return;
        }
      }
    }
    uint8_t a[4], b[4];
    const int n = encode(lo, a);
    encode(hi, b);
    seq(from, a, b, n, to);
  }

  // Builds `id` between fresh nodes *s and *e.
  void build(const std::vector<Ast>& ast, int id, int* s, int* e) {
    *s = add(N_EPS);
    *e = add(N_EPS);
    if (failed) return;
    const Ast& a = ast[id];
    switch (a.kind) {
      case A_EMPTY: eps(*s, *e); break;
      case A_CLASS:
        for (const Range& r : a.ranges) cp_range(*s, r.first, r.second, *e);
        break;
      case A_CAT: {
        int cur = *s;
        for (int k : a.kids) {
          int ks, ke;
          build(ast, k, &ks, &ke);
          if (failed) return;
          eps(cur, ks);
          cur = ke;
        }
        eps(cur, *e);
        break;
      }
      case A_ALT:
        for (int k : a.kids) {
          int ks, ke;
          build(ast, k, &ks, &ke);
          if (failed) return;
          eps(*s, ks);
          eps(ke, *e);
        }
        break;
      default: {  // A_REP: min copies, then a star or (max - min) optional copies
        int cur = *s;
        for (int i = 0; i < a.min; ++i) {
          int ks, ke;
          build(ast, a.kids[0], &ks, &ke);
          if (failed) return;
          eps(cur, ks);
          cur = ke;
        }
        if (a.max < 0) {
          int ks, ke;
          build(ast, a.kids[0], &ks, &ke);
          if (failed) return;
          eps(cur, ks);
          eps(ke, ks);
          eps(ke, *e);
          eps(cur, *e);
        } else {
          for (int i = a.min; i < a.max; ++i) {  // x?x?..: each copy may stop
            int ks, ke;
            build(ast, a.kids[0], &ks, &ke);
            if (failed) return;
            eps(cur, *e);
            eps(cur, ks);
            cur = ke;
          }
          eps(cur, *e);
        }
        break;
      }
    }
  }

  // Pattern.Dollar after node `from`: the rest of the input is empty, \r, \r\n, U+0085, U+2028,
  // U+2029, or \n when the byte before it was not \r.
  void dollar(int from, int end) {
    eps(from, end);
    const int after_cr = add(N_EPS);
    if (failed) return;
    byte_edge(from, '\r', '\r', after_cr);
    eps(after_cr, end);
    byte_edge(after_cr, '\n', '\n', end);
    static const uint8_t k85[2] = {0xC2, 0x85}, k2028[3] = {0xE2, 0x80, 0xA8}, k2029[3] = {0xE2, 0x80, 0xA9};
    seq(from, k85, k85, 2, end);
    seq(from, k2028, k2029, 3, end);
    const int cond = add(N_COND), nl = add(N_EPS);
    if (failed) return;
    nodes[cond].out = nl;
    eps(from, cond);
    byte_edge(nl, '\n', '\n', end);
  }
};

struct Subset {
  const Nfa& nfa;
  std::vector<int> stamp;
  int tick = 0;
  std::vector<int> stack;
  explicit Subset(const Nfa& n) : nfa(n), stamp(n.nodes.size(), 0) {}

  void begin() { ++tick; }
  // adds the closure of `from` to `set` (N_BYTE / N_END nodes); true when it holds N_MATCH
  bool close(int from, bool prev_cr, std::vector<int>& set) {
    bool match = false;
    stack.push_back(from);
    while (!stack.empty()) {
      const int v = stack.back();
      stack.pop_back();
      if (stamp[v] == tick) continue;
      stamp[v] = tick;
      const Node& nd = nfa.nodes[v];
      switch (nd.kind) {
        case N_EPS:
          for (int t : nd.eps) stack.push_back(t);
          break;
        case N_COND:
          if (!prev_cr) stack.push_back(nd.out);
          break;
        case N_MATCH: match = true; break;
        default: set.push_back(v); break;
      }
    }
    return match;
  }
};

}  // namespace

std::vector<uint8_t> Dfa::image() const {
  const size_t bytes = kRegexHeaderBytes + 256 + table.size() * sizeof(uint16_t);
  std::vector<uint8_t> out((bytes + 15) & ~(size_t)15, 0);
  const uint32_t head[4] = {n_states, n_cols, start_row, (uint32_t)table.size()};
  std::memcpy(out.data(), head, sizeof(head));
  std::memcpy(out.data() + kRegexHeaderBytes, cmap, 256);
  if (!table.empty()) std::memcpy(out.data() + kRegexHeaderBytes + 256, table.data(), table.size() * sizeof(uint16_t));
  return out;
}

namespace {

// The image of "every row matches": the walk starts in the accept row and never leaves it.
void always_dfa(Dfa* out) {
  out->n_states = 1;
  out->n_cols = 2;  // one byte column and the end-of-input column, both back to row 0
  out->start_row = kRegexAccept;
  std::memset(out->cmap, 0, sizeof(out->cmap));
  out->table.assign(2, 0);
}

// Subset construction over `nfa` from the closures of start_free and start_caret.
//   search: the unanchored start's closure is re-added to every subset (find); without it the walk
//           is anchored at the first byte (LIKE).
//   accept_start: a start closure that already holds N_MATCH gives the always-matching image
//           (find, LIKE); without it the caller has ruled that out (find-non-empty).
//   prune: compile_like's subsets drop every node that lies before the last % whose loop they hold
//           (whatever such a node can still reach, that loop reaches too), which keeps the DFA of
//           '%a__%b__' the sum, not the product, of its parts'.
// `who` / `dfa` word the declines ("regex" / "search DFA", "LIKE" / "DFA").
bool construct(const Nfa& nfa, int start_free, int start_caret, bool any_dollar, bool search, bool accept_start,
               bool prune, const char* who, const char* dfa, Dfa* out, std::string* err) {
  auto decline = [&](const std::string& m) {
    if (err) *err = m;
    return false;
  };
  // byte intervals on which every edge agrees
  bool cut[257] = {};
  cut[0] = cut[256] = true;
  for (const Node& nd : nfa.nodes)
    if (nd.kind == N_BYTE) {
      cut[nd.lo] = true;
      cut[(int)nd.hi + 1] = true;
    }
  if (any_dollar) cut['\r'] = cut['\r' + 1] = true;  // N_COND asks whether the last byte was \r
  std::vector<int> rep;  // first byte of each interval
  uint8_t interval_of[256];
  for (int b = 0; b < 256; ++b) {
    if (cut[b]) rep.push_back(b);
    interval_of[b] = (uint8_t)(rep.size() - 1);
  }
  const int n_iv = (int)rep.size();

  auto pruned = [&](std::vector<int>& set) {
    if (!prune) return;
    int last = -1;
    for (int v : set)
      if (nfa.nodes[v].tag & 1) last = std::max(last, nfa.nodes[v].tag);
    if (last < 0) return;
    set.erase(std::remove_if(set.begin(), set.end(), [&](int v) { return nfa.nodes[v].tag < last - 1; }), set.end());
  };

  // subset construction; state 0 = accept (absorbing), state 1 = start
  Subset sub(nfa);
  // (each subset is stored once, as its map key; `sets` points at the keys, which never move)
  std::map<std::vector<int>, int> ids;
  std::vector<const std::vector<int>*> sets;
  std::vector<std::vector<uint16_t>> rows;  // n_iv byte columns + end of input
  size_t subset_nodes = 0;
  const std::vector<int> none;
  sets.push_back(&none);
  rows.push_back(std::vector<uint16_t>((size_t)n_iv + 1, 0));
  // the unanchored start's closure after a byte that is / is not \r: added to every subset
  std::vector<int> restart[2];
  if (search)
    for (int cr = 0; cr < 2; ++cr) {
      sub.begin();
      sub.close(start_free, cr != 0, restart[cr]);
    }
  {
    std::vector<int> s0;
    sub.begin();
    bool hit = sub.close(start_free, false, s0);
    hit = sub.close(start_caret, false, s0) || hit;
    if (hit && accept_start) {
      always_dfa(out);
      return true;
    }
    pruned(s0);
    std::sort(s0.begin(), s0.end());
    subset_nodes += s0.size();
    sets.push_back(&ids.emplace(s0, 1).first->first);
    rows.push_back(std::vector<uint16_t>());
  }
  for (size_t cur = 1; cur < sets.size(); ++cur) {
    std::vector<uint16_t> row((size_t)n_iv + 1, 0);
    const std::vector<int>& from = *sets[cur];
    std::map<std::vector<int>, uint16_t> seen;  // byte columns that take the same edges go the same way
    std::vector<int> taken;
    for (int c = 0; c < n_iv; ++c) {
      const int b = rep[c];
      taken.clear();
      taken.push_back(b == '\r');
      for (int v : from) {
        const Node& nd = nfa.nodes[v];
        if (nd.kind == N_BYTE && b >= nd.lo && b <= nd.hi) taken.push_back(nd.out);
      }
      const auto known = seen.find(taken);
      if (known != seen.end()) {
        row[c] = known->second;
        continue;
      }
      std::vector<int> to;
      sub.begin();
      bool hit = false;
      for (int v : restart[b == '\r']) {  // the search may start at the next byte
        sub.stamp[v] = sub.tick;
        to.push_back(v);
      }
      for (size_t k = 1; k < taken.size(); ++k) hit = sub.close(taken[k], b == '\r', to) || hit;
      if (hit) {
        row[c] = 0;
        seen[taken] = 0;
        continue;
      }
      pruned(to);
      std::sort(to.begin(), to.end());
      auto it = ids.find(to);
      if (it == ids.end()) {
        if ((int)sets.size() >= kMaxStates)
          return decline(std::string(who) + ": the pattern's " + dfa + " has more than " + std::to_string(kMaxStates) +
                         " states (cap reached at offset 0): not supported on the GPU path");
        subset_nodes += to.size();
        if (subset_nodes > (size_t)kMaxSubsetNodes)
          return decline(std::string(who) + ": the pattern's " + dfa + " holds more than " + std::to_string(kMaxSubsetNodes) +
                         " NFA nodes in its subsets (cap reached at offset 0): not supported on the GPU path");
        it = ids.emplace(to, (int)sets.size()).first;
        sets.push_back(&it->first);
        rows.push_back(std::vector<uint16_t>());
      }
      row[c] = (uint16_t)it->second;
      seen[taken] = row[c];
    }
    bool at_end = false;
    for (int v : from) at_end = at_end || nfa.nodes[v].kind == N_END;
    row[n_iv] = at_end ? 0 : (uint16_t)cur;
    rows[cur] = row;
  }

  // merge byte columns that are equal in every state
  const int n_states = (int)rows.size();
  std::map<std::vector<uint16_t>, int> col_ids;
  std::vector<int> col_of(n_iv);
  std::vector<int> col_src;
  for (int c = 0; c < n_iv; ++c) {
    std::vector<uint16_t> col(n_states);
    for (int s = 0; s < n_states; ++s) col[s] = rows[s][c];
    auto it = col_ids.find(col);
    if (it == col_ids.end()) {
      it = col_ids.emplace(col, (int)col_src.size()).first;
      col_src.push_back(c);
    }
    col_of[c] = it->second;
  }
  const int n_cols = (int)col_src.size() + 1;
  const size_t entries = (size_t)n_states * n_cols;
  if (entries * sizeof(uint16_t) > (size_t)kMaxTableBytes || entries > 65535)
    return decline(std::string(who) + ": the pattern's transition table (" + std::to_string(n_states) + " states x " +
                   std::to_string(n_cols) + " columns at offset 0) is over the " + std::to_string(kMaxTableBytes) +
                   "-byte LDS budget: not supported on the GPU path");
  out->n_states = (uint32_t)n_states;
  out->n_cols = (uint32_t)n_cols;
  out->start_row = (uint32_t)n_cols;  // state 1
  for (int b = 0; b < 256; ++b) out->cmap[b] = (uint8_t)col_of[interval_of[b]];
  out->table.assign(entries, 0);
  for (int s = 0; s < n_states; ++s) {
    for (int k = 0; k + 1 < n_cols; ++k) out->table[(size_t)s * n_cols + k] = (uint16_t)(rows[s][col_src[k]] * n_cols);
    out->table[(size_t)s * n_cols + n_cols - 1] = (uint16_t)(rows[s][n_iv] * n_cols);
  }
  return true;
}

}  // namespace

bool compile_mode(const uint8_t* pattern, int32_t len, Mode mode, Dfa* out, std::string* err) {
  auto decline = [&](const std::string& m) {
    if (err) *err = m;
    return false;
  };
  if (mode != kFindNonEmpty && mode != kFind) return decline("regex: unknown matching mode");
  if (len < 0 || (len > 0 && !pattern)) return decline("regex: NULL pattern");
  if (len > kMaxPatternBytes) return decline("regex: a pattern longer than " + std::to_string(kMaxPatternBytes) + " bytes is not supported on the GPU path");
  Parser ps;
  ps.p = pattern;
  ps.n = len;
  std::vector<Branch> branches;
  if (!ps.parse_top(&branches)) return decline(ps.err);
  if (mode == kFindNonEmpty)
    for (const Branch& b : branches)
      if (ps.nullable(b.ast))
        return decline("regex: a pattern that can match the empty string at offset 0 is not supported on the GPU path "
                       "(its leftmost match may be empty where a later one is not)");

  Nfa nfa;
  const int match = nfa.add(N_MATCH), end = nfa.add(N_END);
  const int start_free = nfa.add(N_EPS), start_caret = nfa.add(N_EPS);
  bool any_dollar = false;
  for (const Branch& b : branches) {
    int s, e;
    nfa.build(ps.ast, b.ast, &s, &e);
    if (nfa.failed) break;
    nfa.eps(b.caret ? start_caret : start_free, s);
    if (b.dollar) {
      nfa.dollar(e, end);
      any_dollar = true;
    } else {
      nfa.eps(e, match);
    }
  }
  if (nfa.failed)
    return decline("regex: the pattern needs more than " + std::to_string(kMaxNfaNodes) +
                   " NFA nodes (counted repetitions are unrolled) at offset 0: not supported on the GPU path");
  return construct(nfa, start_free, start_caret, any_dollar, true, mode == kFind, false, "regex", "search DFA", out, err);
}

bool compile(const uint8_t* pattern, int32_t len, Dfa* out, std::string* err) {
  return compile_mode(pattern, len, kFindNonEmpty, out, err);
}

bool compile_like(const uint8_t* pattern, int32_t len, Dfa* out, std::string* err) {
  auto decline = [&](const std::string& m) {
    if (err) *err = m;
    return false;
  };
  if (len < 0 || (len > 0 && !pattern)) return decline("LIKE: NULL pattern");
  if (len > kMaxPatternBytes) return decline("LIKE: a pattern longer than " + std::to_string(kMaxPatternBytes) + " bytes is not supported on the GPU path");
  Parser ps;  // (its UTF-8 decoder only)
  ps.p = pattern;
  ps.n = len;
  Nfa nfa;
  nfa.cur_tag = 1 << 30;  // the end node outlives every pruning
  const int match = nfa.add(N_MATCH), end = nfa.add(N_END);
  nfa.cur_tag = 0;
  const int start = nfa.add(N_EPS), unused = nfa.add(N_EPS);
  int cur = start, stars = 0;
  bool open_tail = false;  // the pattern read so far ends in %
  while (!ps.eof() && !nfa.failed) {
    const int32_t where = ps.at;
    uint32_t cp;
    if (!ps.next_cp(&cp)) return decline("LIKE: invalid UTF-8 in the pattern at offset " + std::to_string(where));
    if (cp == '\\')
      return decline("LIKE: a backslash in the pattern at offset " + std::to_string(where) +
                     " is not supported on the GPU path (Spark's LIKE escapes are not evaluated here)");
    if (cp == '%') {
      if (open_tail) continue;  // %% is %
      ++stars;
      nfa.cur_tag = 2 * stars + 1;
      const int loop = nfa.add(N_EPS);
      nfa.eps(cur, loop);
      nfa.any_cp(loop, loop);
      nfa.cur_tag = 2 * stars;
      cur = loop;
      open_tail = true;
      continue;
    }
    // (a trailing % never gets here again: what follows is matched from the loop node)
    open_tail = false;
    const int nxt = nfa.add(N_EPS);
    if (cp == '_') nfa.any_cp(cur, nxt);
    else nfa.cp_range(cur, cp, cp, nxt);
    cur = nxt;
  }
  if (nfa.failed)
    return decline("LIKE: the pattern needs more than " + std::to_string(kMaxNfaNodes) +
                   " NFA nodes at offset 0: not supported on the GPU path");
  // A trailing %: every continuation accepts, so the state is the accept row itself and the walker
  // stops reading there.  Otherwise only the end of the input accepts.
  nfa.eps(cur, open_tail ? match : end);
  return construct(nfa, start, unused, false, false, true, true, "LIKE", "DFA", out, err);
}


}  // namespace regex
}  // namespace dq
