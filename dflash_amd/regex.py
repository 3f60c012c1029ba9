"""Regular expressions compiled to minimal byte automata.

compile_regex(pattern) -> ByteDFA(char_next int16 [Sc, 256] with -1 = dead, accepting, start): exactly what
TokenDFA.from_bytes takes.  Full-match semantics over UTF-8: classes and `.` are sets of Unicode scalars (surrogates
excluded), turned into byte-sequence alternations by the standard range split, so the automaton accepts well-formed UTF-8
only.  Pipeline: parse -> Thompson NFA -> subset construction -> trim -> Moore minimisation -> BFS renumbering from
start = 0 (deterministic output).  Pure Python / numpy.

Supported: literals; \\d \\D \\w \\W \\s \\S (ASCII); \\n \\r \\t \\f \\v \\\\; escaped metacharacters; \\xHH; \\uHHHH; `.`; classes with
ranges, escapes and negation; ( ) and (?: ); |; * + ? {m} {m,} {m,n}; `^` / `$` at the ends (ignored).  Everything else is
refused by name with ValueError.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

MAX_CP = 0x10FFFF
_SURR = (0xD800, 0xDFFF)
_DIGIT = [(48, 57)]
_WORD = [(48, 57), (65, 90), (95, 95), (97, 122)]
_SPACE = [(9, 13), (32, 32)]
_SIMPLE = {"n": 10, "r": 13, "t": 9, "f": 12, "v": 11}


class ByteDFA(NamedTuple):
    """char_next int16 [Sc, 256] (-1: dead), accepting: a sorted tuple of states, start."""
    char_next: np.ndarray
    accepting: tuple
    start: int

    @property
    def num_states(self) -> int:
        return int(self.char_next.shape[0])

    def matches(self, data: bytes) -> bool:
        s = self.start
        for b in bytes(data):
            s = int(self.char_next[s, b])
            if s < 0:
                return False
        return s in self.accepting


def _err(what: str, pattern: str, pos: int) -> ValueError:
    return ValueError(f"dflash_amd: regex: {what} is not supported (at {pos} in {pattern!r})")


# ------------------------------------------------------------------------------------------------- sets of code points
def _norm(ranges):
    """Sorted, merged ranges with the surrogates cut out."""
    out = []
    for lo, hi in sorted(ranges):
        for a, b in ((lo, min(hi, _SURR[0] - 1)), (max(lo, _SURR[1] + 1), hi)):
            if a > b:
                continue
            if out and a <= out[-1][1] + 1:
                out[-1] = (out[-1][0], max(out[-1][1], b))
            else:
                out.append((a, b))
    return out


def _complement(ranges):
    out, at = [], 0
    for lo, hi in _norm(ranges):
        if lo > at:
            out.append((at, lo - 1))
        at = hi + 1
    if at <= MAX_CP:
        out.append((at, MAX_CP))
    return _norm(out)


def _utf8_split(lo: int, hi: int):
    """The byte-range sequences whose concatenations are exactly the UTF-8 encodings of lo..hi (no surrogate inside)."""
    if lo > hi:
        return
    for mx in (0x7F, 0x7FF, 0xFFFF):
        if lo <= mx < hi:
            yield from _utf8_split(lo, mx)
            yield from _utf8_split(mx + 1, hi)
            return
    if hi <= 0x7F:
        yield [(lo, hi)]
        return
    for i in (1, 2, 3):
        m = (1 << (6 * i)) - 1
        if (lo & ~m) != (hi & ~m):
            if lo & m:
                yield from _utf8_split(lo, lo | m)
                yield from _utf8_split((lo | m) + 1, hi)
                return
            if (hi & m) != m:
                yield from _utf8_split(lo, (hi & ~m) - 1)
                yield from _utf8_split(hi & ~m, hi)
                return
    yield list(zip(chr(lo).encode("utf-8"), chr(hi).encode("utf-8")))


# ------------------------------------------------------------------------------------------------- the parser
# AST: ("set", ranges) | ("cat", [nodes]) | ("alt", [nodes]) | ("rep", node, m, n or None)
class _Parser:
    def __init__(self, pattern: str):
        if not isinstance(pattern, str):
            raise ValueError("dflash_amd: regex: the pattern is a str")
        self.p, self.i = pattern, 0
        self.end = len(pattern)

    def parse(self):
        if self.p.startswith("^"):
            self.i = 1
        if self.end > self.i and self.p.endswith("$"):   # (an escaped one is a literal)
            k = self.end - 1
            slashes = 0
            while k - 1 - slashes >= 0 and self.p[k - 1 - slashes] == "\\":
                slashes += 1
            if slashes % 2 == 0:
                self.end -= 1
        node = self.alt()
        if self.i < self.end:
            raise ValueError(f"dflash_amd: regex: unbalanced ')' at {self.i} in {self.p!r}")
        return node

    def peek(self):
        return self.p[self.i] if self.i < self.end else ""

    def alt(self):
        arms = [self.cat()]
        while self.peek() == "|":
            self.i += 1
            arms.append(self.cat())
        return arms[0] if len(arms) == 1 else ("alt", arms)

    def cat(self):
        items = []
        while self.i < self.end and self.peek() not in "|)":
            items.append(self.quantified())
        return ("cat", items)

    def quantified(self):
        at = self.i
        node = self.atom()
        c = self.peek()
        rep = None
        if c == "*":
            rep, self.i = (0, None), self.i + 1
        elif c == "+":
            rep, self.i = (1, None), self.i + 1
        elif c == "?":
            rep, self.i = (0, 1), self.i + 1
        elif c == "{":
            rep = self.braces()
        if rep is None:
            return node
        c = self.peek()
        if c == "?":
            raise _err("a lazy quantifier", self.p, self.i)
        if c == "+":
            raise _err("a possessive quantifier", self.p, self.i)
        if c == "*" or (c == "{" and self.braces(probe=True)):
            raise ValueError(f"dflash_amd: regex: multiple repeat at {self.i} in {self.p!r}")
        m, n = rep
        if n is not None and n < m:
            raise ValueError(f"dflash_amd: regex: repeat {{{m},{n}}} at {at} in {self.p!r}: min above max")
        return ("rep", node, m, n)

    def braces(self, probe: bool = False):
        """{m} {m,} {m,n} {,n} at self.i, or None (a literal brace, as `re` reads it)."""
        j = self.p.find("}", self.i, self.end)
        if j < 0:
            return None
        body = self.p[self.i + 1:j]
        lo, comma, hi = body.partition(",")
        if not ((lo.isdigit() or (lo == "" and comma and hi.isdigit())) and (hi == "" or hi.isdigit())) or not body.isascii():
            return None
        if not probe:
            self.i = j + 1
        m = int(lo) if lo else 0
        return (m, m) if not comma else (m, int(hi) if hi else None)

    def atom(self):
        c = self.peek()
        at = self.i
        self.i += 1
        if c == "(":
            if self.peek() == "?":
                nxt = self.p[self.i + 1:self.i + 3]
                if nxt[:1] == ":":
                    self.i += 2
                elif nxt[:1] in ("=", "!") or nxt in ("<=", "<!"):
                    raise _err("lookaround", self.p, at)
                elif nxt[:2] == "P=":
                    raise _err("a backreference", self.p, at)
                elif nxt[:1] in ("P", "<"):
                    raise _err("a named group", self.p, at)
                else:
                    raise _err("an inline flag (or another (?...) construct)", self.p, at)
            node = self.alt()
            if self.peek() != ")":
                raise ValueError(f"dflash_amd: regex: missing ')' for the group at {at} in {self.p!r}")
            self.i += 1
            return node
        if c == "[":
            return ("set", self.klass(at))
        if c == ".":
            return ("set", _complement([(10, 10)]))
        if c == "\\":
            r = self.escape(at, in_class=False)
            return ("set", _norm(r))
        if c in "*+?":
            raise ValueError(f"dflash_amd: regex: nothing to repeat at {at} in {self.p!r}")
        if c in "^$":
            raise _err("an anchor inside the pattern", self.p, at)
        return ("set", [(ord(c), ord(c))] if not _SURR[0] <= ord(c) <= _SURR[1] else self.surrogate(at))

    def surrogate(self, at):
        raise ValueError(f"dflash_amd: regex: a surrogate code point at {at} in {self.p!r} has no UTF-8 encoding")

    def hexes(self, n: int, at: int) -> int:
        h = self.p[self.i:self.i + n]
        if len(h) != n or self.i + n > self.end or any(ch not in "0123456789abcdefABCDEF" for ch in h):
            raise ValueError(f"dflash_amd: regex: bad hex escape at {at} in {self.p!r}")
        self.i += n
        return int(h, 16)

    def escape(self, at: int, in_class: bool):
        """The code point ranges of the escape whose backslash sits at `at` (self.i is behind the backslash)."""
        if self.i >= self.end:
            raise ValueError(f"dflash_amd: regex: a lone backslash ends {self.p!r}")
        c = self.p[self.i]
        self.i += 1
        if c in "dDwWsS":
            base = {"d": _DIGIT, "w": _WORD, "s": _SPACE}[c.lower()]
            return base if c.islower() else _complement(base)
        if c in _SIMPLE:
            return [(_SIMPLE[c], _SIMPLE[c])]
        if c == "x":
            v = self.hexes(2, at)
            return [(v, v)]
        if c == "u":
            v = self.hexes(4, at)
            if _SURR[0] <= v <= _SURR[1]:
                self.surrogate(at)
            return [(v, v)]
        if c in "bB":
            raise _err(f"\\{c}", self.p, at)
        if c.isdigit():
            raise _err("a backreference (or an octal escape)", self.p, at)
        if c.isascii() and c.isalpha():
            raise _err(f"the escape \\{c}", self.p, at)
        if _SURR[0] <= ord(c) <= _SURR[1]:
            self.surrogate(at)
        return [(ord(c), ord(c))]

    def klass(self, at: int):
        neg = self.peek() == "^"
        if neg:
            self.i += 1
        ranges, first = [], True
        while True:
            if self.i >= self.end:
                raise ValueError(f"dflash_amd: regex: unterminated class at {at} in {self.p!r}")
            c = self.p[self.i]
            if c == "]" and not first:
                self.i += 1
                break
            first = False
            lo = self.class_item()
            if (len(lo) == 1 and lo[0][0] == lo[0][1] and self.peek() == "-" and self.i + 1 < self.end
                    and self.p[self.i + 1] != "]"):
                self.i += 1
                hi = self.class_item()
                if not (len(hi) == 1 and hi[0][0] == hi[0][1]) or hi[0][0] < lo[0][0]:
                    raise ValueError(f"dflash_amd: regex: bad character range in the class at {at} in {self.p!r}")
                ranges.append((lo[0][0], hi[0][0]))
            else:
                ranges.extend(lo)
        return _complement(ranges) if neg else _norm(ranges)

    def class_item(self):
        c = self.p[self.i]
        at = self.i
        self.i += 1
        if c == "\\":
            return list(self.escape(at, in_class=True))
        if c == "[" and self.peek() == ":":
            raise _err("a POSIX class", self.p, at)
        if _SURR[0] <= ord(c) <= _SURR[1]:
            self.surrogate(at)
        return [(ord(c), ord(c))]


# ------------------------------------------------------------------------------------------------- Thompson NFA
class _NFA:
    def __init__(self):
        self.eps = []      # state -> [targets]
        self.edges = []    # state -> [(lo, hi, target)] over bytes

    def new(self) -> int:
        self.eps.append([])
        self.edges.append([])
        return len(self.eps) - 1

    def build(self, node):
        """(start, end) of a fragment for node."""
        kind = node[0]
        if kind == "set":
            s, e = self.new(), self.new()
            for lo, hi in node[1]:
                for seq in _utf8_split(lo, hi):
                    at = s
                    for k, (a, b) in enumerate(seq):
                        to = e if k == len(seq) - 1 else self.new()
                        self.edges[at].append((a, b, to))
                        at = to
            return s, e
        if kind == "cat":
            s = e = self.new()
            for item in node[1]:
                a, b = self.build(item)
                self.eps[e].append(a)
                e = b
            return s, e
        if kind == "alt":
            s, e = self.new(), self.new()
            for arm in node[1]:
                a, b = self.build(arm)
                self.eps[s].append(a)
                self.eps[b].append(e)
            return s, e
        _, sub, m, n = node
        s = e = self.new()
        for _ in range(m):
            a, b = self.build(sub)
            self.eps[e].append(a)
            e = b
        if n is None:                       # a star behind the m copies
            a, b = self.build(sub)
            loop = self.new()
            self.eps[e].append(loop)
            self.eps[loop].append(a)
            self.eps[b].append(loop)
            return s, loop
        out = self.new()
        for _ in range(n - m):              # each optional copy may leave for the end
            self.eps[e].append(out)
            a, b = self.build(sub)
            self.eps[e].append(a)
            e = b
        self.eps[e].append(out)
        return s, out


def _closures(nfa: _NFA):
    memo = {}

    def closure(s: int):
        got = memo.get(s)
        if got is None:
            seen, stack = {s}, [s]
            while stack:
                for t in nfa.eps[stack.pop()]:
                    if t not in seen:
                        seen.add(t)
                        stack.append(t)
            got = memo[s] = frozenset(seen)
        return got
    return closure


def _subsets(nfa: _NFA, start: int, final: int, max_states: int, pattern: str):
    """Subset construction: (next int32 [S, 256] with -1, accepting bool [S]); the state count is checked as it grows."""
    closure = _closures(nfa)
    first = closure(start)
    index, order, rows = {first: 0}, [first], []
    at = 0
    while at < len(order):
        cur = order[at]
        at += 1
        edges = [e for s in cur for e in nfa.edges[s]]
        row = np.full(256, -1, dtype=np.int32)
        cuts = sorted({lo for lo, _, _ in edges} | {hi + 1 for _, hi, _ in edges})
        for a, b in zip(cuts, cuts[1:]):    # bytes a .. b-1 leave by the same edges
            to = frozenset().union(*(closure(t) for lo, hi, t in edges if lo <= a <= hi))
            if not to:
                continue
            k = index.get(to)
            if k is None:
                k = index[to] = len(order)
                order.append(to)
                if len(order) > max_states:
                    raise ValueError(f"dflash_amd: regex: {pattern!r} needs more than max_states = {max_states} states")
            row[a:b] = k
        rows.append(row)
    return np.stack(rows), np.fromiter((final in s for s in order), dtype=bool, count=len(order))


def _trim(nxt, acc):
    """Transitions into states that reach no accepting state become -1; returns (next, alive)."""
    S = nxt.shape[0]
    alive = acc.copy()
    while True:
        reach = alive[np.where(nxt < 0, 0, nxt)] & (nxt >= 0)
        more = alive | reach.any(axis=1)
        if np.array_equal(more, alive):
            break
        alive = more
    out = np.where((nxt >= 0) & alive[np.where(nxt < 0, 0, nxt)], nxt, -1)
    out[~alive] = -1
    return out, alive


def _minimise(nxt, acc, alive):
    """Moore's partition refinement over the live states (the dead state is the class -1)."""
    S = nxt.shape[0]
    label = np.where(alive, acc.astype(np.int64), -1)
    count = -1
    while True:
        succ = np.where(nxt < 0, -1, label[np.where(nxt < 0, 0, nxt)])
        sig = np.concatenate([label[:, None], succ], axis=1)
        _, new = np.unique(sig, axis=0, return_inverse=True)
        new = new.reshape(S).astype(np.int64)
        new = np.where(alive, new, -1)
        n = len(np.unique(new[alive]))
        if n == count:
            return new
        count, label = n, new


def compile_regex(pattern: str, *, max_states: int = 4096) -> ByteDFA:
    """The minimal trimmed byte DFA of `pattern` (full match, UTF-8).  ValueError: unsupported syntax (named), an empty
    language, more than max_states states during the subset construction."""
    if not 1 <= int(max_states) <= 32767:
        raise ValueError(f"dflash_amd: regex: max_states = {max_states} outside 1..32767")
    ast = _Parser(pattern).parse()
    nfa = _NFA()
    s, e = nfa.build(ast)
    nxt, acc = _subsets(nfa, s, e, int(max_states), pattern)
    nxt, alive = _trim(nxt, acc)
    if not alive[0]:
        raise ValueError(f"dflash_amd: regex: {pattern!r} matches nothing (an empty language)")
    label = _minimise(nxt, acc, alive)
    # one representative per class, numbered in BFS order from the start over bytes 0..255
    rep = {}
    for st in range(nxt.shape[0]):
        if alive[st]:
            rep.setdefault(int(label[st]), st)
    number, queue, rows, accepting = {int(label[0]): 0}, [int(label[0])], [], []
    at = 0
    while at < len(queue):
        cls = queue[at]
        at += 1
        src = nxt[rep[cls]]
        row = np.full(256, -1, dtype=np.int16)
        for b in np.nonzero(src >= 0)[0]:
            c = int(label[src[b]])
            k = number.get(c)
            if k is None:
                k = number[c] = len(queue)
                queue.append(c)
            row[b] = k
        rows.append(row)
        if acc[rep[cls]]:
            accepting.append(number[cls])
    return ByteDFA(np.stack(rows), tuple(sorted(accepting)), 0)
