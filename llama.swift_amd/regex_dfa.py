"""A small compiler from a regular expression to the byte automaton llamahip_constraint_new takes (Model.constraint(regex=...)).

Syntax: literals, escapes (\\d \\D \\w \\W \\s \\S \\n \\t \\r \\f \\v \\0 \\xHH, any other escaped byte stands for itself), `.` (any byte but
\\n), `[...]` classes with ranges, escapes and `^` negation, `( )` groups (`(?:` is accepted), `|`, `*`, `+`, `?`, `{m}`, `{m,}`, `{m,n}`.  No
anchors, back-references, look-around or lazy quantifiers: the automaton decides FULL matches, as re.fullmatch does on bytes.  A str pattern
is taken as its UTF-8 bytes, so a non-ASCII literal is its byte sequence (put it in a group before a quantifier).

Thompson construction, then the subset construction; no minimisation.  The C ABI takes tables, so this stays in Python."""
from __future__ import annotations

import numpy as np

MAX_STATES = 4096          # llamahip_constraint_new's limit
MAX_REPEAT = 4096
MAX_NFA = 1 << 16         # Thompson states: nested repeats multiply

_DIGIT = frozenset(range(0x30, 0x3A))
_WORD = frozenset(list(range(0x30, 0x3A)) + list(range(0x41, 0x5B)) + list(range(0x61, 0x7B)) + [0x5F])
_SPACE = frozenset(b" \t\n\r\f\v")
_ALL = frozenset(range(256))
_CLASS = {ord("d"): _DIGIT, ord("D"): _ALL - _DIGIT, ord("w"): _WORD, ord("W"): _ALL - _WORD, ord("s"): _SPACE, ord("S"): _ALL - _SPACE}
_CTRL = {ord("n"): 10, ord("t"): 9, ord("r"): 13, ord("f"): 12, ord("v"): 11, ord("0"): 0}


class RegexError(ValueError):
    pass


class _Parser:
    """pattern -> tree: ("set", frozenset) | ("cat", [..]) | ("alt", [..]) | ("rep", node, lo, hi or None)"""

    def __init__(self, p: bytes):
        self.p, self.i = p, 0

    def fail(self, what):
        raise RegexError(f"regex_dfa: {what} at byte {self.i} of {self.p!r}")

    def peek(self):
        return self.p[self.i] if self.i < len(self.p) else None

    def parse(self):
        node = self.alt()
        if self.i != len(self.p):
            self.fail("unbalanced ')'")
        return node

    def alt(self):
        arms = [self.cat()]
        while self.peek() == ord("|"):
            self.i += 1
            arms.append(self.cat())
        return arms[0] if len(arms) == 1 else ("alt", arms)

    def cat(self):
        items = []
        while self.peek() is not None and self.peek() not in b"|)":
            items.append(self.repeat())
        return ("cat", items)

    def repeat(self):
        node = self.atom()
        while True:
            c = self.peek()
            if c == ord("*"):
                lo, hi = 0, None
            elif c == ord("+"):
                lo, hi = 1, None
            elif c == ord("?"):
                lo, hi = 0, 1
            elif c == ord("{"):
                j = self.p.find(b"}", self.i)
                body = self.p[self.i + 1:j] if j > 0 else b""
                parts = body.split(b",")
                if j < 0 or len(parts) > 2 or not parts[0].isdigit() or (len(parts) == 2 and parts[1] and not parts[1].isdigit()):
                    self.fail("bad {m,n}")
                lo = int(parts[0])
                hi = lo if len(parts) == 1 else (int(parts[1]) if parts[1] else None)
                if (hi is not None and hi < lo) or max(lo, hi or 0) > MAX_REPEAT:
                    self.fail(f"bad repeat bounds (at most {MAX_REPEAT})")
                self.i = j
            else:
                return node
            self.i += 1
            if self.peek() is not None and self.peek() in b"*+?{":
                self.fail("a quantifier behind a quantifier (lazy, possessive and stacked repeats are not supported)")
            return ("rep", node, lo, hi)

    def escape(self):
        """behind a backslash: a set"""
        c = self.peek()
        if c is None:
            self.fail("dangling backslash")
        self.i += 1
        if c in _CLASS:
            return _CLASS[c]
        if c in _CTRL:
            return frozenset([_CTRL[c]])
        if c == ord("x"):
            h = self.p[self.i:self.i + 2]
            try:
                v = int(h, 16) if len(h) == 2 else self.fail("bad \\xHH")
            except ValueError:
                self.fail("bad \\xHH")
            self.i += 2
            return frozenset([v])
        if chr(c).isalnum():
            self.fail(f"unsupported escape \\{chr(c)}")
        return frozenset([c])

    def atom(self):
        c = self.peek()
        self.i += 1
        if c == ord("("):
            if self.p[self.i:self.i + 2] == b"?:":
                self.i += 2
            elif self.peek() == ord("?"):
                self.fail("unsupported group")
            node = self.alt()
            if self.peek() != ord(")"):
                self.fail("missing ')'")
            self.i += 1
            return node
        if c == ord("["):
            return ("set", self.klass())
        if c == ord("."):
            return ("set", _ALL - {10})
        if c == ord("\\"):
            return ("set", self.escape())
        if c in b"*+?{":
            self.i -= 1
            self.fail("nothing to repeat")
        if c in b"^$":
            self.i -= 1
            self.fail("anchors are not supported (the match is a full match)")
        return ("set", frozenset([c]))

    def klass(self):
        neg = self.peek() == ord("^")
        if neg:
            self.i += 1
        out, first = set(), True
        while True:
            c = self.peek()
            if c is None:
                self.fail("missing ']'")
            if c == ord("]") and not first:
                self.i += 1
                break
            first = False
            self.i += 1
            lo = self.escape() if c == ord("\\") else frozenset([c])
            if self.peek() == ord("-") and self.i + 1 < len(self.p) and self.p[self.i + 1] != ord("]"):
                self.i += 1
                d = self.peek()
                self.i += 1
                hi = self.escape() if d == ord("\\") else frozenset([d])
                if len(lo) != 1 or len(hi) != 1 or min(hi) < min(lo):
                    self.fail("bad character range")
                out.update(range(min(lo), min(hi) + 1))
            else:
                out.update(lo)
        return frozenset(_ALL - out if neg else out)


class _Nfa:
    def __init__(self):
        self.eps, self.edges = [], []          # per state: epsilon targets; (set, target) edges

    def new(self):
        if len(self.eps) >= MAX_NFA:
            raise RegexError(f"regex_dfa: the pattern needs more than {MAX_NFA} NFA states")
        self.eps.append([])
        self.edges.append([])
        return len(self.eps) - 1

    def build(self, node):
        """-> (entry, exit)"""
        kind = node[0]
        if kind == "set":
            a, b = self.new(), self.new()
            self.edges[a].append((node[1], b))
            return a, b
        if kind == "cat":
            a = b = self.new()
            for item in node[1]:
                s, e = self.build(item)
                self.eps[b].append(s)
                b = e
            return a, b
        if kind == "alt":
            a, b = self.new(), self.new()
            for arm in node[1]:
                s, e = self.build(arm)
                self.eps[a].append(s)
                self.eps[e].append(b)
            return a, b
        _, sub, lo, hi = node
        a = b = self.new()
        for _ in range(lo):
            s, e = self.build(sub)
            self.eps[b].append(s)
            b = e
        if hi is None:                          # a loop: zero or more
            s, e = self.build(sub)
            loop = self.new()
            self.eps[b].append(loop)
            self.eps[loop].append(s)
            self.eps[e].append(loop)
            return a, loop
        end = self.new()
        for _ in range(hi - lo):                # each optional copy may be skipped to the end
            self.eps[b].append(end)
            s, e = self.build(sub)
            self.eps[b].append(s)
            b = e
        self.eps[b].append(end)
        return a, end


def compile(pattern) -> tuple:
    """-> (trans int32 [n_states, 256] with -1 = dead, accept uint8 [n_states], start): the automaton of the pattern's full matches"""
    p = pattern.encode() if isinstance(pattern, str) else bytes(pattern)
    nfa = _Nfa()
    entry, exit_ = nfa.build(_Parser(p).parse())

    def closure(states):
        seen, stack = set(states), list(states)
        while stack:
            for t in nfa.eps[stack.pop()]:
                if t not in seen:
                    seen.add(t)
                    stack.append(t)
        return frozenset(seen)

    start = closure([entry])
    ids, order, rows = {start: 0}, [start], []
    k = 0
    while k < len(order):
        cur = order[k]
        k += 1
        row = np.full(256, -1, np.int32)
        moves: dict = {}
        for s in cur:
            for cs, t in nfa.edges[s]:
                for b in cs:
                    moves.setdefault(b, set()).add(t)
        memo: dict = {}
        for b, ts in moves.items():
            key = frozenset(ts)
            if key not in memo:
                nxt = closure(key)
                if nxt not in ids:
                    if len(order) >= MAX_STATES:
                        raise RegexError(f"regex_dfa: more than {MAX_STATES} states for {p!r}")
                    ids[nxt] = len(order)
                    order.append(nxt)
                memo[key] = ids[nxt]
            row[b] = memo[key]
        rows.append(row)
    accept = np.array([1 if exit_ in st else 0 for st in order], np.uint8)
    return np.stack(rows), accept, 0


def matches(dfa, data: bytes) -> bool:
    """the automaton run on data (the tests compare it with re.fullmatch)"""
    trans, accept, q = dfa
    for b in data:
        q = int(trans[q, b])
        if q < 0:
            return False
    return bool(accept[q])
