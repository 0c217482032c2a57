"""Guided decoding, host side: a pattern becomes a token-level automaton.

``compile_guide(kind, pattern, token_bytes, eos_ids, max_states)`` turns a
regular expression (``kind="regex"``, full-match semantics) or a list of strings
(``kind="choice"``: the alternation of the escaped strings) into a ``Guide``
whose table ``next`` (int16 [S, V]) says for every state and every token of the
vocabulary which state follows, or -1 when the token is not allowed there. The
engine uploads the table into its arena and ``ops.guide_`` (guide.hip) walks it
on the device, one state per sequence. NumPy only; no GPU.

The steps: parse -> byte NFA (Thompson) -> byte DFA (subset construction) ->
dead states removed -> minimised (Moore) -> token table, by walking every
token's bytes through the DFA for all tokens at once (one NumPy gather per byte
position), breadth first from the start state so that only states a token
sequence can reach get a row.

Supported regex subset: literals (non-ASCII ones as their UTF-8 bytes), ``.``
(any character but a newline), classes and negated classes of ASCII characters
and ranges, ``\\d \\w \\s \\D \\W \\S`` (ASCII), ``\\n \\t \\r \\f \\v \\xHH`` and
escaped punctuation, ``|``, groups ``(...)`` and ``(?:...)``, and the greedy
quantifiers ``* + ? {m} {m,} {m,n} {,n}`` with counts up to ``MAX_REPEAT``.
``.``, negated classes and ``\\D \\W \\S`` match one whole well-formed UTF-8
character, never a lone byte, so every string the automaton accepts is valid
UTF-8. Everything else is refused with a ``SamplingError`` that names the
construct.
"""
from __future__ import annotations

import hashlib

import numpy as np

from p2p_llm_tunnel_amd.models.params import SamplingError

MAX_PATTERN = 2048  # characters of a guided_regex
MAX_CHOICES = 256  # strings of a guided_choice
MAX_CHOICE_BYTES = 16384  # UTF-8 bytes of all the strings of a guided_choice together
MAX_REPEAT = 256  # largest count of {m}, {m,}, {m,n}
MAX_DEPTH = 32  # groups inside groups
MAX_NFA_STATES = 4096  # Thompson states of a regex, counted before any is built: nested counted repeats multiply
MAX_DFA_STATES = 16384  # byte-DFA states during the subset construction, whatever max_states is
DFA_PER_STATE = 4  # ... and at most DFA_PER_STATE * max_states + 256 of them (see ``dfa_limit``)
MAX_STATES = 32767  # states of a token table (its entries are int16)


# ---------------------------------------------------------------- parser
# AST: ("set", mask bool[256] over single bytes < 0x80, wide) where ``wide`` adds every multi-byte UTF-8 character;
# ("cat", [nodes]); ("alt", [nodes]); ("rep", node, lo, hi | None).

def _mask(chars=()) -> np.ndarray:
    m = np.zeros(256, dtype=bool)
    for c in chars:
        m[c] = True
    return m


_DIGIT = _mask(range(48, 58))
_WORD = _mask(list(range(48, 58)) + list(range(65, 91)) + list(range(97, 123)) + [95])
_SPACE = _mask([32, 9, 10, 13, 12, 11])
_ASCII = _mask(range(128))
_CLASSES = {"d": (_DIGIT, False), "w": (_WORD, False), "s": (_SPACE, False),
            "D": (_ASCII & ~_DIGIT, True), "W": (_ASCII & ~_WORD, True), "S": (_ASCII & ~_SPACE, True)}
_SIMPLE = {"n": 10, "t": 9, "r": 13, "f": 12, "v": 11}


def _literal(ch: str):
    b = ch.encode("utf-8")
    nodes = [("set", _mask([x]), False) for x in b]
    return nodes[0] if len(nodes) == 1 else ("cat", nodes)


class _Parser:
    def __init__(self, pattern: str):
        self.p = pattern
        self.i = 0
        self.depth = 0

    def fail(self, what: str):
        return SamplingError(f"guided_regex: {what} (at offset {self.i} of {self.p!r})")

    def peek(self) -> str:
        return self.p[self.i] if self.i < len(self.p) else ""

    def parse(self):
        node = self.alt()
        if self.i < len(self.p):
            raise self.fail("unbalanced ')'")
        return node

    def alt(self):
        arms = [self.cat()]
        while self.peek() == "|":
            self.i += 1
            arms.append(self.cat())
        return arms[0] if len(arms) == 1 else ("alt", arms)

    def cat(self):
        items = []
        while self.i < len(self.p) and self.peek() not in "|)":
            items.append(self.quantified())
        return ("cat", items)

    def quantified(self):
        atom = self.atom()
        for count in (0, 1):
            c = self.peek()
            lo_hi = None
            if c == "*":
                lo_hi, n = (0, None), 1
            elif c == "+":
                lo_hi, n = (1, None), 1
            elif c == "?":
                lo_hi, n = (0, 1), 1
            elif c == "{":
                lo_hi, n = self.braces()
            if lo_hi is None:
                return atom
            if count:
                raise self.fail("a quantifier on a quantifier (multiple repeat) is not supported; use a group")
            self.i += n
            if self.peek() == "?":
                raise self.fail("lazy quantifiers are not supported")
            if self.peek() == "+":
                raise self.fail("possessive quantifiers are not supported")
            lo, hi = lo_hi
            if lo > MAX_REPEAT or (hi is not None and hi > MAX_REPEAT):
                raise self.fail(f"counted repeats above {MAX_REPEAT} are not supported")
            if hi is not None and hi < lo:
                raise self.fail("a counted repeat's maximum is below its minimum")
            atom = ("rep", atom, lo, hi)

    def braces(self):
        """``{m}``, ``{m,}``, ``{m,n}``, ``{,n}``, ``{,}`` at the cursor: ((lo, hi), length), or (None, 0) for a literal brace."""
        j = self.p.find("}", self.i)
        if j < 0:
            return None, 0
        body = self.p[self.i + 1:j]
        lo, sep, hi = body.partition(",")
        if not ((lo.isascii() and lo.isdigit()) or (lo == "" and sep)) or not (hi == "" or (hi.isascii() and hi.isdigit())):
            return None, 0
        if not sep:
            return (int(lo), int(lo)), j - self.i + 1
        return (int(lo or 0), int(hi) if hi else None), j - self.i + 1

    def atom(self):
        c = self.peek()
        if c == "(":
            return self.group()
        if c == "[":
            return self.klass()
        if c == "\\":
            return self.escape(False)
        if c in "*+?":
            raise self.fail(f"nothing to repeat before {c!r}")
        if c in "^$":
            raise self.fail(f"anchors ({c!r}) are not supported: the pattern always matches the whole completion")
        self.i += 1
        if c == ".":
            m = _ASCII.copy()
            m[10] = False
            return ("set", m, True)
        return _literal(c)

    def group(self):
        self.depth += 1
        if self.depth > MAX_DEPTH:
            raise self.fail(f"groups nested deeper than {MAX_DEPTH} are not supported")
        try:
            return self.group_body()
        finally:
            self.depth -= 1

    def group_body(self):
        self.i += 1
        if self.peek() == "?":
            nxt = self.p[self.i + 1:self.i + 3]
            if nxt[:1] == ":":
                self.i += 2
            elif nxt[:1] in ("=", "!") or nxt in ("<=", "<!"):
                raise self.fail("look-around is not supported")
            elif nxt == "P=":
                raise self.fail("back-references are not supported")
            elif nxt[:1] == "P" or nxt[:1] == "<":
                raise self.fail("named groups are not supported")
            elif nxt[:1] == "#":
                raise self.fail("comments are not supported")
            elif nxt[:1] == "(":
                raise self.fail("conditional groups are not supported")
            else:
                raise self.fail("inline flags are not supported")
        node = self.alt()
        if self.peek() != ")":
            raise self.fail("missing ')'")
        self.i += 1
        return node

    def escape(self, in_class: bool):
        """An escape at the cursor: a ("set", ...) node, or a literal node."""
        self.i += 1
        c = self.peek()
        if not c:
            raise self.fail("a trailing backslash")
        self.i += 1
        if c in _CLASSES:
            m, wide = _CLASSES[c]
            return ("set", m.copy(), wide)
        if c in _SIMPLE:
            return ("set", _mask([_SIMPLE[c]]), False)
        if c == "x":
            h = self.p[self.i:self.i + 2]
            if len(h) != 2 or any(x not in "0123456789abcdefABCDEF" for x in h):
                raise self.fail("\\x needs two hex digits")
            self.i += 2
            return _literal(chr(int(h, 16)))
        if c.isdigit() and c != "0":
            raise self.fail("back-references are not supported")
        if c == "b" and in_class:
            return ("set", _mask([8]), False)
        if c in "bBAZ":
            raise self.fail(f"anchors and word boundaries (\\{c}) are not supported")
        if c.isascii() and not c.isalnum():
            return ("set", _mask([ord(c)]), False)
        raise self.fail(f"the escape \\{c} is not supported")

    def klass(self):
        self.i += 1
        negate = self.peek() == "^"
        if negate:
            self.i += 1
        m, wide, first = _mask(), False, True
        while True:
            c = self.peek()
            if not c:
                raise self.fail("missing ']'")
            if c == "]" and not first:
                self.i += 1
                break
            first = False
            lo = self.member()
            if isinstance(lo, tuple):  # \d and the like: no range
                m |= lo[0]
                wide |= lo[1]
                continue
            if self.peek() == "-" and self.p[self.i + 1:self.i + 2] not in ("]", ""):
                self.i += 1
                hi = self.member()
                if isinstance(hi, tuple):
                    raise self.fail("a class range cannot end in a character class")
                if hi < lo:
                    raise self.fail("a class range runs backwards")
                m[lo:hi + 1] = True
            else:
                m[lo] = True
        if negate:
            return ("set", _ASCII & ~m, not wide)
        return ("set", m, wide)

    def member(self):
        """One class member at the cursor: a byte < 0x80, or (mask, wide) for an escaped class."""
        c = self.peek()
        if c == "\\":
            node = self.escape(True)
            if node[0] != "set" or node[2] or node[1].sum() != 1:
                if node[0] == "set":
                    return node[1], node[2]
                raise self.fail("non-ASCII characters in a class are not supported")
            return int(np.nonzero(node[1])[0][0])
        self.i += 1
        if ord(c) >= 128:
            raise self.fail("non-ASCII characters in a class are not supported")
        return ord(c)


def _r(lo: int, hi: int) -> np.ndarray:
    m = np.zeros(256, dtype=bool)
    m[lo:hi + 1] = True
    return m


# Well-formed multi-byte UTF-8 (RFC 3629): no overlong forms, no surrogates, nothing above U+10FFFF.
_TAIL = _r(0x80, 0xBF)
_LEAD3 = _r(0xE1, 0xEC) | _r(0xEE, 0xEF)
_UTF8_EDGES = [("a", _r(0xC2, 0xDF), "t1"), ("a", _r(0xE0, 0xE0), "e0"), ("a", _LEAD3, "t2"), ("a", _r(0xED, 0xED), "ed"),
               ("a", _r(0xF0, 0xF0), "f0"), ("a", _r(0xF1, 0xF3), "t3"), ("a", _r(0xF4, 0xF4), "f4"),
               ("e0", _r(0xA0, 0xBF), "t1"), ("ed", _r(0x80, 0x9F), "t1"), ("f0", _r(0x90, 0xBF), "t2"),
               ("f4", _r(0x80, 0x8F), "t2"), ("t3", _TAIL, "t2"), ("t2", _TAIL, "t1"), ("t1", _TAIL, "b")]


# ---------------------------------------------------------------- automata
class _Nfa:
    def __init__(self):
        self.eps: list[list[int]] = []
        self.edges: list[list[tuple]] = []

    def state(self) -> int:
        self.eps.append([])
        self.edges.append([])
        return len(self.eps) - 1

    def build(self, node) -> tuple[int, int]:
        kind = node[0]
        if kind == "set":
            a, b = self.state(), self.state()
            if node[1].any():
                self.edges[a].append((node[1], b))
            if node[2]:  # t1, t2, t3: one, two, three continuation bytes to go; the tails are shared
                st = {name: self.state() for name in ("t1", "t2", "t3", "e0", "ed", "f0", "f4")}
                st["a"], st["b"] = a, b
                for at, m, to in _UTF8_EDGES:
                    self.edges[st[at]].append((m, st[to]))
            return a, b
        if kind == "cat":
            a = b = self.state()
            for item in node[1]:
                s, e = self.build(item)
                self.eps[b].append(s)
                b = e
            return a, b
        if kind == "alt":
            a, b = self.state(), self.state()
            for arm in node[1]:
                s, e = self.build(arm)
                self.eps[a].append(s)
                self.eps[e].append(b)
            return a, b
        _, inner, lo, hi = node
        a = b = self.state()
        for _ in range(lo):
            s, e = self.build(inner)
            self.eps[b].append(s)
            b = e
        if hi is None:  # a loop
            s, e = self.build(inner)
            end = self.state()
            self.eps[b] += [s, end]
            self.eps[e] += [s, end]
            return a, end
        end = self.state()
        self.eps[b].append(end)
        for _ in range(hi - lo):  # each further copy may stop
            s, e = self.build(inner)
            self.eps[b].append(s)
            self.eps[e].append(end)
            b = e
        return a, end


def nfa_size(node) -> int:
    """The number of states ``_Nfa.build`` makes for ``node``, from the tree alone (a counted repeat is one node
    there and ``hi`` copies in the automaton, so nested repeats multiply)."""
    kind = node[0]
    if kind == "set":
        return 2 + (7 if node[2] else 0)
    if kind == "cat":
        return 1 + sum(nfa_size(n) for n in node[1])
    if kind == "alt":
        return 2 + sum(nfa_size(n) for n in node[1])
    _, inner, lo, hi = node
    return 2 + nfa_size(inner) * (lo + 1 if hi is None else hi)


def dfa_limit(max_states: int) -> int:
    """Byte-DFA states the subset construction may make for a table of at most ``max_states`` token-level
    states. Every token-level state is a byte-level one; the others lie inside tokens or inside multi-byte
    characters (a ``.`` has up to seven of those before minimisation merges them), so a pattern that needs many
    times ``max_states`` of them would not fit the table either, and is refused before the work is done."""
    return min(MAX_DFA_STATES, DFA_PER_STATE * int(max_states) + 256)


def _determinize(nfa: _Nfa, start: int, final: int, limit: int = MAX_DFA_STATES):
    """Subset construction: (trans int32 [S, 256] with -1 = no move, accept bool [S]); state 0 is the start."""
    eps = nfa.eps

    def closure(states) -> frozenset:  # one walk from the whole set: linear in what it reaches
        seen = set(states)
        stack = list(seen)
        while stack:
            for t in eps[stack.pop()]:
                if t not in seen:
                    seen.add(t)
                    stack.append(t)
        return frozenset(seen)

    first = closure([start])
    index, order, rows = {first: 0}, [first], []
    i = 0
    while i < len(order):
        cur = order[i]
        i += 1
        by_mask: dict[bytes, list] = {}  # the few distinct byte sets of this state's moves, each with its targets
        for s in cur:
            for mk, t in nfa.edges[s]:
                got = by_mask.get(mk.tobytes())
                if got is None:
                    by_mask[mk.tobytes()] = [mk, {t}]
                else:
                    got[1].add(t)
        moves = list(by_mask.values())
        row = np.full(256, -1, dtype=np.int32)
        if moves:
            m = np.stack([mk for mk, _ in moves]).astype(np.uint8)
            cols, inv = np.unique(m, axis=1, return_inverse=True)
            inv = np.asarray(inv).reshape(-1)
            for j in range(cols.shape[1]):
                hit = np.nonzero(cols[:, j])[0]
                if not len(hit):
                    continue
                to = closure(set().union(*[moves[k][1] for k in hit]))
                k = index.get(to)
                if k is None:
                    if len(order) >= limit:
                        raise SamplingError(f"the pattern needs more than {limit} byte-level states (at most "
                                            f"{DFA_PER_STATE} x max_states + 256, and {MAX_DFA_STATES})")
                    k = index[to] = len(order)
                    order.append(to)
                row[inv == j] = k
        rows.append(row)
    return np.stack(rows), np.array([final in s for s in order], dtype=bool)


def _prune_dead(trans: np.ndarray, accept: np.ndarray):
    """Moves into states from which no accepting state can be reached become -1. One backward pass over the
    distinct (source, target) pairs: linear in their number, also for a chain."""
    n = trans.shape[0]
    src, dst = np.nonzero(trans >= 0)
    pairs = np.unique(src.astype(np.int64) * n + trans[src, dst])
    back: list[list[int]] = [[] for _ in range(n)]
    for a, b in zip((pairs // n).tolist(), (pairs % n).tolist()):
        back[b].append(a)
    live = accept.copy()
    stack = np.nonzero(accept)[0].tolist()
    while stack:
        for a in back[stack.pop()]:
            if not live[a]:
                live[a] = True
                stack.append(a)
    out = np.where((trans >= 0) & live[np.maximum(trans, 0)], trans, -1)
    return out, live


def _minimize(trans: np.ndarray, accept: np.ndarray):
    """Hopcroft's partition refinement, O(k n log n) for n states and k byte classes (bytes whose columns of
    ``trans`` are equal move alike and are refined once); -1 (no move) is a sink state of its own. Returns
    (trans, accept) of the states reachable from state 0, one per class, renumbered breadth first in byte order
    from the start, which stays state 0: two patterns with the same language give the same arrays."""
    n = trans.shape[0]
    cols = np.unique(trans, axis=1)  # [n, k]: one column per byte class
    k = cols.shape[1]
    total = np.concatenate([np.where(cols >= 0, cols, n), np.full((1, k), n, dtype=cols.dtype)])  # sink: state n
    pre = []  # pre[c][q]: the states that move to q on class c
    for c in range(k):
        into: list[list[int]] = [[] for _ in range(n + 1)]
        for a, b in enumerate(total[:, c].tolist()):
            into[b].append(a)
        pre.append(into)
    final = set(np.nonzero(accept)[0].tolist())
    blocks = [b for b in (final, set(range(n + 1)) - final) if b]
    block_of = [0] * (n + 1)
    for i, b in enumerate(blocks):
        for q in b:
            block_of[q] = i
    small = min(range(len(blocks)), key=lambda i: len(blocks[i]))
    work = {(small, c) for c in range(k)}
    while work:
        a, c = work.pop()
        into = pre[c]
        hit: dict[int, set] = {}
        for q in blocks[a]:
            for p in into[q]:
                hit.setdefault(block_of[p], set()).add(p)
        for y, part in hit.items():
            if len(part) == len(blocks[y]):
                continue
            blocks[y] -= part
            new = len(blocks)
            blocks.append(part)
            for p in part:
                block_of[p] = new
            less = new if len(part) <= len(blocks[y]) else y
            for c2 in range(k):
                work.add((new, c2) if (y, c2) in work else (less, c2))
    label = np.asarray(block_of[:n], dtype=np.int64)
    count = len(blocks)
    rep = np.full(count, -1, dtype=np.int64)  # one state per class
    for q in range(n - 1, -1, -1):
        rep[label[q]] = q
    order, seen, i = [int(label[0])], {int(label[0])}, 0
    while i < len(order):
        row = trans[rep[order[i]]]
        i += 1
        for t in row[np.sort(np.unique(row, return_index=True)[1])].tolist():  # first occurrences, in byte order
            if t >= 0 and int(label[t]) not in seen:
                seen.add(int(label[t]))
                order.append(int(label[t]))
    renum = np.full(count, -1, dtype=np.int64)
    renum[order] = np.arange(len(order))
    src = trans[rep[order]]
    out = np.where(src >= 0, renum[label[np.maximum(src, 0)]], -1).astype(np.int32)
    return out, accept[rep[order]]


def compile_dfa(kind: str, pattern, limit: int = MAX_DFA_STATES):
    """The minimal byte DFA of a pattern: (trans int32 [S, 256], -1 = the walk dies; accept bool [S]); state 0 is the
    start, and from every state an accepting state can be reached. ``limit``: byte-level states the subset
    construction may make before the pattern is refused."""
    if kind == "regex":
        if not isinstance(pattern, str):
            raise SamplingError(f"guided_regex must be a string, got {pattern!r}")
        if len(pattern) > MAX_PATTERN:
            raise SamplingError(f"guided_regex takes at most {MAX_PATTERN} characters, got {len(pattern)}")
        ast = _Parser(pattern).parse()
        size = nfa_size(ast)
        if size > MAX_NFA_STATES:
            raise SamplingError(f"guided_regex: the pattern is too large: its counted repeats and groups expand to "
                                f"{size} automaton states, at most {MAX_NFA_STATES} are accepted (nested counts "
                                "multiply)")
    elif kind == "choice":
        if not isinstance(pattern, (list, tuple)) or not pattern or \
                not all(isinstance(c, str) and c for c in pattern):
            raise SamplingError(f"guided_choice must be a non-empty list of non-empty strings, got {pattern!r}")
        if len(pattern) > MAX_CHOICES:
            raise SamplingError(f"guided_choice takes at most {MAX_CHOICES} strings, got {len(pattern)}")
        if sum(len(c.encode("utf-8")) for c in pattern) > MAX_CHOICE_BYTES:
            raise SamplingError(f"guided_choice takes at most {MAX_CHOICE_BYTES} bytes of text in all")
        ast = ("alt", [("cat", [("set", _mask([b]), False) for b in c.encode("utf-8")]) for c in dict.fromkeys(pattern)])
    else:
        raise SamplingError(f'a guide is a "regex" or a "choice", got {kind!r}')
    nfa = _Nfa()
    start, final = nfa.build(ast)
    trans, accept = _determinize(nfa, start, final, limit)
    trans, live = _prune_dead(trans, accept)
    if not live[0]:
        raise SamplingError("the pattern matches nothing")
    return _minimize(trans, accept)


class Guide:
    """A compiled pattern over one vocabulary. ``next``: int16 [S, V] (C
    order), the state after token t in state s or -1; state 0 is the start.
    ``accepting``: bool [S]. ``key`` identifies the table's bytes (the engine
    shares a resident table between requests with the same key). ``dfa`` /
    ``dfa_accept`` / ``dfa_state`` keep the byte DFA and each token state's
    byte-DFA state, for ``matches`` and ``viable``."""
    __slots__ = ("kind", "pattern", "next", "accepting", "key", "dfa", "dfa_accept", "dfa_state", "eos_ids")

    def __init__(self, kind, pattern, table, accepting, dfa, dfa_accept, dfa_state, eos_ids):
        self.kind, self.pattern = kind, pattern
        self.next = np.ascontiguousarray(table, dtype=np.int16)
        self.accepting = accepting
        self.dfa, self.dfa_accept, self.dfa_state = dfa, dfa_accept, dfa_state
        self.eos_ids = tuple(eos_ids)
        self.key = hashlib.sha1(self.next.tobytes()).hexdigest() + f":{self.next.shape[0]}x{self.next.shape[1]}"

    @property
    def n_states(self) -> int:
        return self.next.shape[0]

    @property
    def vocab(self) -> int:
        return self.next.shape[1]

    def walk(self, data: bytes) -> int:
        """The byte DFA's state after ``data`` from the start, -1 when the walk dies."""
        s = 0
        for b in data:
            s = int(self.dfa[s, b])
            if s < 0:
                return -1
        return s

    def matches(self, data: bytes) -> bool:
        s = self.walk(data)
        return s >= 0 and bool(self.dfa_accept[s])

    def viable(self, data: bytes) -> bool:
        """``data`` begins a string the pattern matches (dead states are gone, so: the walk survives)."""
        return self.walk(data) >= 0


_BLOCK = 32  # token-table rows computed together: [_BLOCK, V] int32 of working state


def token_table(trans: np.ndarray, accept: np.ndarray, token_bytes, eos_ids, max_states: int):
    """The token-level table of a byte DFA: (next int16 [S, V], accepting bool [S], the byte-DFA state of every
    row). Row 0 is the start; only states a sequence of tokens reaches get a row."""
    V = len(token_bytes)
    eos = sorted({int(e) for e in eos_ids})
    if not eos:
        raise SamplingError("guided decoding needs at least one EOS token id: a completion ends by sampling one")
    if any(not 0 <= e < V for e in eos):
        raise SamplingError(f"EOS ids {eos} are not all inside the vocabulary [0, {V})")
    max_states = min(int(max_states), MAX_STATES)
    lens = np.fromiter((len(b) for b in token_bytes), dtype=np.int64, count=V)
    lens[eos] = 0  # an EOS id never walks: it is allowed exactly in accepting states
    by_len = np.argsort(-lens, kind="stable")  # longest first: the tokens still walking at position p are a prefix
    longest = int(lens.max()) if V else 0
    padded = np.zeros((V, max(longest, 1)), dtype=np.uint8)
    for rank, t in enumerate(by_len):
        n = lens[t]
        if n == 0:
            break
        padded[rank, :n] = np.frombuffer(token_bytes[t], dtype=np.uint8)
    active = [int((lens > p).sum()) for p in range(longest)]
    sink = trans.shape[0]
    ext = np.concatenate([np.where(trans >= 0, trans, sink), np.full((1, 256), sink, dtype=trans.dtype)]).astype(np.int32)

    index, order, rows = {0: 0}, [0], []
    done = 0
    while done < len(order):
        block = order[done:done + _BLOCK]
        st = np.repeat(np.asarray(block, dtype=np.int32)[:, None], V, axis=1)  # columns in by_len order
        for p in range(longest):
            n = active[p]
            st[:, :n] = ext[st[:, :n], padded[None, :n, p]]
        for k, s in enumerate(block):
            row = np.full(V, -1, dtype=np.int16)  # byte-DFA states: at most MAX_DFA_STATES, which fits
            row[by_len] = np.where(st[k] == sink, -1, st[k])
            row[lens == 0] = -1  # control tokens, added tokens without bytes, EOS
            for t in np.unique(row[row >= 0]):
                if int(t) not in index:
                    index[int(t)] = len(order)
                    order.append(int(t))
                    if len(order) > max_states:
                        raise SamplingError(f"the pattern needs more than max_states = {max_states} token-level states")
            rows.append(row)
        done += len(block)
    remap = np.full(sink + 1, -1, dtype=np.int64)
    remap[order] = np.arange(len(order))
    table = np.stack([np.where(r >= 0, remap[np.maximum(r, 0)], -1) for r in rows]).astype(np.int16)
    accepting = accept[order]
    for s in range(len(order)):
        if accepting[s]:
            table[s, eos] = s
        elif not (table[s] >= 0).any():
            raise SamplingError(f"the pattern cannot be completed with this vocabulary: after some allowed text "
                                f"(token state {s}) no token continues it and it is not a full match")
    return table, accepting, np.asarray(order, dtype=np.int32)


def compile_guide(kind: str, pattern, token_bytes, eos_ids, max_states: int = 1024) -> Guide:
    """Compile ``pattern`` ("regex": a string in the subset the module
    docstring lists; "choice": a non-empty list of non-empty strings) for a
    vocabulary given as ``token_bytes`` (the bytes of every id; b"" for control
    tokens, which are never allowed) and its ``eos_ids`` (allowed exactly where
    the text so far is a full match, and leaving the state as it is). Raises
    ``SamplingError`` naming the reason: an unsupported construct, no EOS id, a
    state in which the vocabulary offers no token, more than ``max_states``
    token-level states."""
    trans, accept = compile_dfa(kind, pattern, dfa_limit(max_states))
    table, accepting, states = token_table(trans, accept, token_bytes, eos_ids, max_states)
    return Guide(kind, pattern if isinstance(pattern, str) else tuple(pattern), table, accepting, trans, accept, states,
                 sorted({int(e) for e in eos_ids}))
