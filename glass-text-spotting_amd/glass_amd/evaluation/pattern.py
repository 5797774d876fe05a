"""Patterns for pattern-constrained decoding: a regex, a character set or a lexicon trie as ONE deterministic finite
automaton (DFA) over the decoder's fold symbols, built once on the host and kept on the device - what glass_beam_search_dfa
(include/glass_hip_feature_dfa.h) consults at every decoding step (`ASTER_V2.beam_decode(pattern=...)`,
`RecognizerRCNNHeadV3.set_pattern`).  `LexiconTrie` (evaluation/lexicon.py) is the special case "the automaton is a tree".

Alphabet: `fold_table(characters, eos, case_insensitive)` of evaluation/lexicon.py - with case_insensitive=True a character
and its other case are one symbol, exactly as in the trie; the special tokens and `eos` have no symbol.

Regex subset, compiled here (not with `re`), with the meaning of `re.fullmatch` on strings over the character set (and of
`re.IGNORECASE` with case_insensitive=True):
    literal characters and \\-escaped literals (any character that is not an ASCII letter or digit may be escaped);
    .  (any character of the set);  [...] and [^...] with ranges;  \\d \\w \\s \\D \\W \\S, intersected with the set;
    (...)  (?:...)  |  and the quantifiers  *  +  ?  {m}  {m,}  {,n}  {m,n}.
Anything else - anchors, back-references, look-around, lazy or possessive quantifiers, named groups, inline flags, other
letter escapes - raises ValueError naming the construct and its position.  A literal or a class that holds no character of
the set is legal and matches nothing.

Construction: Thompson NFA -> subset construction -> states that cannot reach an accepting state removed -> Moore partition
refinement (minimize=True) -> states numbered breadth-first from the segments' start states, symbols ascending.  All segments
share one state array.

Decoding rule (the contract of the kernel, the float64 replay of the tests and the docs).  At step t (0-based, L = max_len) a
hypothesis in state q
    may emit class c iff f = fold[c] >= 0, q' = next[q][f] exists and t + 1 + dist[q'] <= L - 1;
    may emit the stop iff accept[q] >= 0 and t >= 1 (the empty string is never emitted, as with the trie).
So every live hypothesis can still complete; the language in force is {w in L(regex) : 1 <= |w| <= L - 1}.

`DecodePattern.weighted(lm=..., word_logprior=..., length_bonus=...)` (evaluation/weighted_pattern.py) puts a weight on every
transition of the automaton - a character n-gram model, word priors, a length bonus - for glass_beam_search_wdfa.
"""
from __future__ import annotations

import time
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from .lexicon import WEIGHTED_TABLE_CAP_BYTES, fold_table

MAX_STATES = (1 << 24) - 1                        # a target state has 24 bits of a table entry
NEXT_TABLE_CAP_BYTES = WEIGHTED_TABLE_CAP_BYTES   # most bytes of the `next` table (256 MiB)
NFA_STATE_CAP = 1 << 16                           # most Thompson states of one regex: {m,n} copies its operand
DIST_FIELD_MAX = 127                              # dist is stored as min(dist, 127) in bits 24..30
NO_PATH = np.iinfo(np.int32).max                  # dist of a state without a path to acceptance (the one state of an empty automaton)


# ------------------------------------------------------------------ the regex -> syntax tree
class _Alphabet:
    """the characters of the set (one per class that has a fold symbol) and their fold symbols; sets of fold symbols are
    Python ints used as bit masks"""

    def __init__(self, characters: Sequence[str], fold: np.ndarray, case_insensitive: bool):
        self.ci = case_insensitive
        self.chars = [(ch, int(f)) for ch, f in zip(characters, fold) if f >= 0]
        self.all = 0
        for _, f in self.chars:
            self.all |= 1 << f

    def where(self, pred) -> int:
        m = 0
        for ch, f in self.chars:
            if pred(ch):
                m |= 1 << f
        return m

    def _variants(self, ch: str) -> Tuple[str, ...]:
        if not self.ci:
            return (ch,)
        return tuple({ch} | {v for v in (ch.lower(), ch.upper()) if len(v) == 1})

    def literal(self, x: str):
        xs = set(self._variants(x))
        return lambda ch: any(v in xs for v in self._variants(ch))

    def range(self, lo: str, hi: str):
        return lambda ch: any(lo <= v <= hi for v in self._variants(ch))


_CLASS_ESCAPES = {"d": lambda ch: ch.isdecimal(), "w": lambda ch: ch.isalnum() or ch == "_", "s": lambda ch: ch.isspace()}


class _Parser:
    """recursive descent; the tree: ("set", mask) | ("cat", [nodes]) | ("alt", [nodes]) | ("rep", node, m, n or None)"""

    def __init__(self, pattern: str, alphabet: _Alphabet):
        self.p, self.i, self.al = pattern, 0, alphabet

    def fail(self, what: str, pos: Optional[int] = None):
        raise ValueError(f"DecodePattern: unsupported {what} at position {self.i if pos is None else pos} of {self.p!r}")

    def parse(self):
        node = self.alt()
        if self.i < len(self.p):
            self.fail("unbalanced ')'")
        return node

    def alt(self):
        branches = [self.cat()]
        while self.i < len(self.p) and self.p[self.i] == "|":
            self.i += 1
            branches.append(self.cat())
        return branches[0] if len(branches) == 1 else ("alt", branches)

    def cat(self):
        items = []
        while self.i < len(self.p) and self.p[self.i] not in "|)":
            items.append(self.repeat())
        return ("cat", items)

    def repeat(self):
        node = self.atom()
        quantified = False
        while self.i < len(self.p):
            c = self.p[self.i]
            if c in "*+?":
                m, n = {"*": (0, None), "+": (1, None), "?": (0, 1)}[c]
                end = self.i + 1
            elif c == "{":
                m, n, end = self.braces()
            else:
                break
            if quantified:
                self.fail("lazy quantifier" if c == "?" else "possessive quantifier" if c == "+" else "multiple repeat")
            self.i = end
            node = ("rep", node, m, n)
            quantified = True
        return node

    def braces(self):
        j = self.p.find("}", self.i)
        body = self.p[self.i + 1:j] if j >= 0 else ""
        lo, comma, hi = body.partition(",")
        if j < 0 or not (lo.isdigit() or (lo == "" and comma)) or not (hi.isdigit() or hi == "") or not body.isascii() or body == ",":
            self.fail("'{' that opens no {m}, {m,}, {,n} or {m,n}")
        m = int(lo) if lo else 0
        n = m if not comma else (int(hi) if hi else None)
        if n is not None and n < m:
            self.fail(f"quantifier {{{body}}} with max below min")
        return m, n, j + 1

    def atom(self):
        c = self.p[self.i]
        if c == "(":
            at = self.i
            self.i += 1
            if self.p.startswith("?", self.i):
                if not self.p.startswith("?:", self.i):
                    nxt = self.p[self.i + 1:self.i + 3]
                    what = ("look-around" if nxt[:1] in ("=", "!") or nxt in ("<=", "<!") else
                            "named group" if nxt[:1] == "P" or nxt[:1] == "<" else "inline flags or group extension")
                    self.fail(what, at)
                self.i += 2
            node = self.alt()
            if self.i >= len(self.p) or self.p[self.i] != ")":
                self.fail("unbalanced '('", at)
            self.i += 1
            return node
        if c == "[":
            return ("set", self.char_class())
        if c == ".":
            self.i += 1
            return ("set", self.al.all)
        if c in "^$":
            self.fail(f"anchor {c!r}")
        if c in "*+?{":
            self.fail(f"quantifier {c!r} with nothing to repeat")
        if c == "\\":
            pred = self.escape(in_class=False)
            return ("set", self.al.where(pred))
        self.i += 1
        return ("set", self.al.where(self.al.literal(c)))

    def escape(self, in_class: bool):
        """at a backslash -> the predicate of the escape; a (pred, char) pair is not needed: `self.last_literal` holds the
        character of a literal escape (None for a class escape), for ranges"""
        at = self.i
        if self.i + 1 >= len(self.p):
            self.fail("trailing backslash")
        e = self.p[self.i + 1]
        self.i += 2
        self.last_literal = None
        if e.lower() in _CLASS_ESCAPES:
            base = _CLASS_ESCAPES[e.lower()]
            return base if e.islower() else (lambda ch: not base(ch))
        if e.isascii() and e.isdigit():
            self.fail("back-reference or octal escape", at)
        if e.isascii() and e.isalpha():
            self.fail(f"anchor \\{e}" if e in "AZbB" and not in_class else f"escape \\{e}", at)
        self.last_literal = e
        return self.al.literal(e)

    def char_class(self) -> int:
        at = self.i
        self.i += 1
        negate = self.p.startswith("^", self.i)
        if negate:
            self.i += 1
        preds = []
        first = True
        while True:
            if self.i >= len(self.p):
                self.fail("unterminated '['", at)
            c = self.p[self.i]
            if c == "]" and not first:
                self.i += 1
                break
            first = False
            if c == "[" and self.p.startswith("[:", self.i):
                self.fail("POSIX class")
            if c == "\\":
                pred = self.escape(in_class=True)
                lo = self.last_literal
            else:
                self.i += 1
                pred, lo = self.al.literal(c), c
            if self.p.startswith("-", self.i) and self.i + 1 < len(self.p) and self.p[self.i + 1] != "]":
                dash = self.i
                self.i += 1
                if self.p[self.i] == "\\":
                    self.escape(in_class=True)
                    hi = self.last_literal
                else:
                    hi = self.p[self.i]
                    self.i += 1
                if lo is None or hi is None:
                    self.fail("range with a class escape as a bound", dash)
                if hi < lo:
                    self.fail(f"range {lo}-{hi} with its bounds reversed", dash)
                pred = self.al.range(lo, hi)
            preds.append(pred)
        if negate:
            return self.al.where(lambda ch: not any(p(ch) for p in preds))
        return self.al.where(lambda ch: any(p(ch) for p in preds))


# ------------------------------------------------------------------ syntax tree -> Thompson NFA -> DFA
class _Nfa:
    def __init__(self, cap: int):
        self.eps: List[List[int]] = []
        self.edges: List[List[Tuple[int, int]]] = []
        self.cap = cap

    def state(self) -> int:
        if len(self.eps) >= self.cap:
            raise ValueError(f"DecodePattern: the regex needs more than {self.cap} NFA states (the NFA size limit; "
                             "lower the {m,n} counts)")
        self.eps.append([])
        self.edges.append([])
        return len(self.eps) - 1

    def build(self, node) -> Tuple[int, int]:
        kind = node[0]
        if kind == "set":
            s, e = self.state(), self.state()
            if node[1]:
                self.edges[s].append((node[1], e))
            return s, e
        if kind == "cat":
            s = e = self.state()
            for item in node[1]:
                a, b = self.build(item)
                self.eps[e].append(a)
                e = b
            return s, e
        if kind == "alt":
            s, e = self.state(), self.state()
            for item in node[1]:
                a, b = self.build(item)
                self.eps[s].append(a)
                self.eps[b].append(e)
            return s, e
        _, body, m, n = node
        s = e = self.state()
        for _ in range(m):
            a, b = self.build(body)
            self.eps[e].append(a)
            e = b
        if n is None:                       # X*: a loop state
            loop, out = self.state(), self.state()
            a, b = self.build(body)
            self.eps[e].append(loop)
            self.eps[loop] += [a, out]
            self.eps[b].append(loop)
            return s, out
        for _ in range(n - m):              # X?: the copy, or past it
            a, b = self.build(body)
            out = self.state()
            self.eps[e] += [a, out]
            self.eps[b].append(out)
            e = out
        return s, e


def _subset_construction(nfa: _Nfa, s0: int, final: int, F: int, state_cap: int) -> Tuple[List[List[int]], List[bool]]:
    """-> (rows of F targets, -1 = none; accepting flags); state 0 is the start.  The empty set is no state."""
    closure_of: Dict[int, frozenset] = {}

    def closure(states) -> frozenset:
        out = set()
        for q in states:
            c = closure_of.get(q)
            if c is None:
                seen, stack = {q}, [q]
                while stack:
                    for r in nfa.eps[stack.pop()]:
                        if r not in seen:
                            seen.add(r)
                            stack.append(r)
                c = closure_of[q] = frozenset(seen)
            out |= c
        return frozenset(out)

    start = closure([s0])
    ids = {start: 0}
    order = [start]
    rows: List[List[int]] = []
    i = 0
    while i < len(order):
        by_mask: Dict[int, set] = {}
        for q in order[i]:
            for mask, tgt in nfa.edges[q]:
                by_mask.setdefault(mask, set()).add(tgt)
        row = [-1] * F
        cache: Dict[frozenset, int] = {}
        masks = list(by_mask.items())
        for f in range(F):
            bit = 1 << f
            key = frozenset(j for j, (mask, _) in enumerate(masks) if mask & bit)
            if not key:
                continue
            t = cache.get(key)
            if t is None:
                tset = closure(set().union(*(masks[j][1] for j in key)))
                t = ids.get(tset)
                if t is None:
                    if len(order) >= state_cap:
                        raise ValueError(f"DecodePattern: the automaton needs more than {state_cap} states (the limit of "
                                         "2^24 - 1 states and of the table's bytes)")
                    t = ids[tset] = len(order)
                    order.append(tset)
                cache[key] = t
            row[f] = t
        rows.append(row)
        i += 1
    return rows, [final in sset for sset in order]


def _distances(nxt: np.ndarray, accept: np.ndarray) -> np.ndarray:
    """fewest symbols from every state to an accepting one (NO_PATH where there is none): relaxation over the edge list"""
    N = nxt.shape[0]
    dist = np.where(accept >= 0, 0, NO_PATH).astype(np.int64)
    src, _ = np.nonzero(nxt >= 0)
    tgt = nxt[nxt >= 0].astype(np.int64)
    for _ in range(N + 1):
        cand = np.where(dist[tgt] < NO_PATH, dist[tgt] + 1, NO_PATH)
        new = dist.copy()
        np.minimum.at(new, src, cand)
        if np.array_equal(new, dist):
            break
        dist = new
    return dist.astype(np.int32)


def _moore(nxt: np.ndarray, accept: np.ndarray) -> np.ndarray:
    """Moore partition refinement -> the block of every state (blocks numbered arbitrarily)"""
    _, label = np.unique(accept, return_inverse=True)
    label = label.reshape(-1).astype(np.int64)
    count = int(label.max()) + 1 if label.size else 0
    while True:
        sig = np.concatenate([label[:, None], np.where(nxt >= 0, label[np.maximum(nxt, 0)], -1)], axis=1)
        _, new = np.unique(sig, axis=0, return_inverse=True)
        new = new.reshape(-1).astype(np.int64)
        n = int(new.max()) + 1 if new.size else 0
        if n == count:
            return new
        label, count = new, n


def _renumber(nxt: np.ndarray, accept: np.ndarray, starts: List[int]) -> Tuple[np.ndarray, np.ndarray, List[int]]:
    """breadth-first from the start states in segment order, symbols ascending; states no start reaches are dropped"""
    new_id = np.full(nxt.shape[0], -1, dtype=np.int64)
    order: List[int] = []
    for s in starts:
        if s < 0 or new_id[s] >= 0:
            continue
        new_id[s] = len(order)
        order.append(s)
        head = len(order) - 1
        while head < len(order):
            for t in nxt[order[head]]:
                if t >= 0 and new_id[t] < 0:
                    new_id[t] = len(order)
                    order.append(int(t))
            head += 1
    idx = np.asarray(order, dtype=np.int64)
    out = nxt[idx]
    out = np.where(out >= 0, new_id[np.maximum(out, 0)], -1).astype(np.int32)
    return out, accept[idx], [int(new_id[s]) if s >= 0 else -1 for s in starts]


class DecodePattern:
    """What the decoder may spell, as a DFA over fold symbols kept on the device (module docstring: alphabet, regex subset,
    construction, decoding rule).

    `patterns`: one regex string (one segment, key None) or a dict {key: regex} (one segment per key; `segment(key)`, `keys`
    and `len()` as in LexiconTrie / DeviceLexicon); `text_encoder_or_characters`: a TextEncoder or its list of class strings;
    `max_len`: the decoder's steps (a string needs one more step than it has characters, for the stop); `eos`: the stop class.

    numpy arrays, mirrored on the device in `tensors` (with the int "F"):
      `next` int32 [N, F]: -1 = no transition, else the target state in bits 0..23 and min(dist[target], 127) in bits 24..30 -
        one load per (beam, class) decides a candidate, with no dependent second load;
      `dist` int32 [N]: the fewest symbols to an accepting state (not uploaded; NO_PATH for the one state of an empty automaton);
      `accept` int32 [N]: -1, or a tag >= 0 (0 for a regex, the word index for `from_trie`);
      `start` int32 [S]: -1 for a segment whose language is empty at this max_len;  `fold` int32 [C];
      `group_start` int32 [F + 1], `group_cls` int32: `fold_groups()`, read only by a merged search (merge_case=True).
    Limits (ValueError): N <= 2^24 - 1, `next` at most `table_cap_bytes`, at most `nfa_cap` Thompson states per regex."""

    word_state = None         # from_trie only: int32 [words], the state every word of the trie ends at (-1: left out)
    segment_sizes = None      # from_trie only: the words of every segment

    def __init__(self, patterns: Union[str, Dict[object, str]], text_encoder_or_characters, max_len: int, eos: int,
                 case_insensitive: bool = False, minimize: bool = True, device=None, *,
                 table_cap_bytes: int = NEXT_TABLE_CAP_BYTES, nfa_cap: int = NFA_STATE_CAP):
        t0 = time.perf_counter()
        if isinstance(patterns, dict):
            self.keys = list(patterns.keys())
            regexes = [patterns[k] for k in self.keys]
        else:
            self.keys = [None]
            regexes = [patterns]
        for r in regexes:
            if not isinstance(r, str):
                raise TypeError(f"DecodePattern: a pattern must be a regex string (got {type(r).__name__})")
        self.patterns = list(regexes)
        self._alphabet(text_encoder_or_characters, max_len, eos, case_insensitive)
        self.minimize = bool(minimize)
        F = self.num_fold
        alphabet = _Alphabet(self._characters, self.fold, self.case_insensitive)
        state_cap = self._state_cap(F, table_cap_bytes)
        rows: List[List[int]] = []
        acc: List[bool] = []
        starts: List[int] = []
        for regex in regexes:
            nfa = _Nfa(int(nfa_cap))
            s0, final = nfa.build(_Parser(regex, alphabet).parse())
            r, a = _subset_construction(nfa, s0, final, F, state_cap - len(rows))
            base = len(rows)
            starts.append(base)
            rows += [[t + base if t >= 0 else -1 for t in row] for row in r]
            acc += a
        nxt = np.asarray(rows, dtype=np.int64).reshape(len(rows), F)
        accept = np.where(np.asarray(acc, dtype=bool), 0, -1).astype(np.int32)
        # ---- states without a path to acceptance go, and with them the segments whose start is one
        dead = _distances(nxt, accept) == NO_PATH
        nxt = np.where((nxt >= 0) & ~dead[np.maximum(nxt, 0)], nxt, -1)
        starts = [-1 if dead[s] else s for s in starts]
        if self.minimize:
            block = _moore(nxt, accept)
            first = np.full(int(block.max()) + 1, -1, dtype=np.int64)
            first[block[::-1]] = np.arange(len(block))[::-1]          # a representative of every block
            nxt = np.where(nxt[first] >= 0, block[np.maximum(nxt[first], 0)], -1)
            accept = accept[first]
            starts = [int(block[s]) if s >= 0 else -1 for s in starts]
        nxt, accept, starts = _renumber(nxt, accept, starts)
        self._finish(nxt, accept, np.asarray(starts, dtype=np.int32), table_cap_bytes, device, t0)

    # ---- shared by the constructors
    def _alphabet(self, text_encoder_or_characters, max_len, eos, case_insensitive) -> None:
        characters = list(getattr(text_encoder_or_characters, "character", text_encoder_or_characters))
        self._characters = characters
        self.num_classes, self.max_len, self.eos = len(characters), int(max_len), int(eos)
        self.case_insensitive = bool(case_insensitive)
        if not 0 <= self.eos < self.num_classes:
            raise ValueError(f"eos {eos} outside [0, {self.num_classes})")
        if self.max_len < 1:
            raise ValueError(f"max_len {max_len} (at least 1)")
        self.fold, self.fold_symbols = fold_table(characters, self.eos, self.case_insensitive)
        self.num_fold = len(self.fold_symbols)
        self._sym_id = {s: i for i, s in enumerate(self.fold_symbols)}

    @staticmethod
    def _state_cap(F: int, table_cap_bytes: int) -> int:
        return max(min(MAX_STATES, int(table_cap_bytes) // (4 * F)), 0)

    def _finish(self, nxt: np.ndarray, accept: np.ndarray, start: np.ndarray, table_cap_bytes: int, device, t0: float) -> None:
        F = self.num_fold
        if nxt.shape[0] == 0:               # no string at all: one state that no start points to, so that no array is empty
            nxt, accept = np.full((1, F), -1, dtype=np.int32), np.full(1, -1, dtype=np.int32)
        N = nxt.shape[0]
        if N > MAX_STATES:
            raise ValueError(f"DecodePattern: automaton of {N} states (the limit is 2^24 - 1 = {MAX_STATES})")
        if N * F * 4 > int(table_cap_bytes):
            raise ValueError(f"DecodePattern: transition table of {N} x {F} entries = {N * F * 4} bytes (the table limit is "
                             f"{int(table_cap_bytes)} bytes)")
        nxt = np.ascontiguousarray(nxt, dtype=np.int32)
        self.accept = np.ascontiguousarray(accept, dtype=np.int32)
        self.dist = _distances(nxt, self.accept)
        # a segment whose shortest string does not fit the steps has no string at this max_len
        start = np.asarray(start, dtype=np.int32).copy()
        ok = start >= 0
        start[ok] = np.where(self.dist[start[ok]] <= self.max_len - 1, start[ok], -1)
        self.start = start
        field = np.minimum(self.dist, DIST_FIELD_MAX).astype(np.int32)
        self.next = np.where(nxt >= 0, nxt | (field[np.maximum(nxt, 0)] << 24), -1).astype(np.int32)
        self.num_states = N
        self.nbytes = int(self.next.nbytes + self.accept.nbytes + self.start.nbytes + self.fold.nbytes)
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.tensors = {"next": torch.from_numpy(self.next).to(self.device), "accept": torch.from_numpy(self.accept).to(self.device),
                        "start": torch.from_numpy(self.start).to(self.device), "fold": torch.from_numpy(self.fold).to(self.device),
                        "F": F}
        self._upload_groups()
        self.build_seconds = time.perf_counter() - t0

    # ---- the fold groups of a merged search (include/glass_hip_feature_merged.h)
    def fold_groups(self) -> Tuple[np.ndarray, np.ndarray]:
        """(group_start int32 [F + 1], group_cls int32 [classes with a fold symbol]) from `self.fold`: the classes of fold
        symbol f are group_cls[group_start[f]:group_start[f + 1]], ascending - with case_insensitive=True a letter's two cases,
        otherwise one class each.  The stop and the specials (fold -1) are in no group.  Deterministic: a stable sort."""
        fold = np.asarray(self.fold, dtype=np.int64)
        cls = np.nonzero((fold >= 0) & (fold < self.num_fold))[0]
        cls = cls[np.argsort(fold[cls], kind="stable")]
        start = np.zeros(self.num_fold + 1, dtype=np.int64)
        np.cumsum(np.bincount(fold[cls], minlength=self.num_fold), out=start[1:])
        return start.astype(np.int32), cls.astype(np.int32)

    def _upload_groups(self) -> None:
        self.group_start, self.group_cls = self.fold_groups()
        self.tensors["group_start"] = torch.from_numpy(self.group_start).to(self.device)
        self.tensors["group_cls"] = torch.from_numpy(self.group_cls).to(self.device)

    # ---- the other constructors
    @classmethod
    def from_charset(cls, chars, text_encoder_or_characters, max_len: int, eos: int, case_insensitive: bool = False,
                     minimize: bool = True, device=None, **limits) -> "DecodePattern":
        """one or more characters of `chars`: the regex `[chars]+`"""
        chars = list(chars)
        if not chars or any(not isinstance(c, str) or len(c) != 1 for c in chars):
            raise ValueError("from_charset: needs at least one character, each a one-character string")
        body = "".join(c if (c.isascii() and c.isalnum()) or not c.isascii() else "\\" + c for c in chars)
        return cls("[" + body + "]+", text_encoder_or_characters, max_len, eos, case_insensitive, minimize, device, **limits)

    @classmethod
    def from_trie(cls, trie, device=None, table_cap_bytes: int = NEXT_TABLE_CAP_BYTES) -> "DecodePattern":
        """a LexiconTrie as a DFA: one state per node, the same fold and keys, accept = node_word, start = seg_root - the
        masks of the two searches are then identical, step for step"""
        t0 = time.perf_counter()
        self = cls.__new__(cls)
        self.keys = list(trie.keys)
        self.patterns = None
        self.minimize = False
        self.num_classes, self.max_len, self.eos = trie.num_classes, trie.max_len, trie.eos
        self.case_insensitive = trie.case_insensitive
        self.fold, self.fold_symbols, self.num_fold = trie.fold.copy(), list(trie.fold_symbols), trie.num_fold
        self._sym_id = {s: i for i, s in enumerate(self.fold_symbols)}
        N, F = trie.num_nodes, trie.num_fold
        if N > MAX_STATES:
            raise ValueError(f"DecodePattern: automaton of {N} states (the limit is 2^24 - 1 = {MAX_STATES})")
        if N * F * 4 > int(table_cap_bytes):
            raise ValueError(f"DecodePattern: transition table of {N} x {F} entries = {N * F * 4} bytes (the table limit is "
                             f"{int(table_cap_bytes)} bytes)")
        nxt = np.empty((N, F), dtype=np.int32)
        for a in range(0, N, 1 << 16):      # child(node, f) = child_base[node] + popcount(mask bits below f), in slices
            mask = trie.child_mask[a:a + (1 << 16)]
            bits = np.unpackbits(mask.view(np.uint8), axis=1, bitorder="little")[:, :F].astype(np.int32)
            rank = np.cumsum(bits, axis=1, dtype=np.int32) - bits
            nxt[a:a + len(mask)] = np.where(bits > 0, trie.child_base[a:a + len(mask), None] + rank, -1)
        self._finish(nxt, trie.node_word.copy(), trie.seg_root.copy(), table_cap_bytes,
                     device if device is not None else trie.device, t0)
        # what `weighted(word_logprior=...)` attaches a prior to: the state every word of `trie.upper` ends at (-1: left out)
        self.word_state, self.segment_sizes = trie.word_node.copy(), list(trie.segment_sizes)
        return self

    def weighted(self, lm=None, word_logprior=None, length_bonus: float = 0.0, table_cap_bytes: Optional[int] = None,
                 device=None) -> "WeightedPattern":
        """this pattern with a weight (a natural log) on every transition, stop and start, for glass_beam_search_wdfa: a
        character n-gram model `lm` (CharNgramLM) crossed with the states, word priors `word_logprior` pushed toward the root
        (a `from_trie` pattern only) and a `length_bonus` per symbol; the three add.  evaluation/weighted_pattern.py has the
        definitions; ValueError for a weight that is not finite and for an argument that does not fit the pattern."""
        from .weighted_pattern import WEIGHTED_TABLE_CAP_BYTES as cap, WeightedPattern
        return WeightedPattern(self, lm, word_logprior, length_bonus, cap if table_cap_bytes is None else table_cap_bytes, device)

    # ---- queries
    def __len__(self) -> int:
        return len(self.keys)

    def segment(self, key) -> int:
        """segment number of a key (None for a single regex); KeyError for an unknown key, as `patterns[key]`."""
        return self.keys.index(key) if key in self.keys else self._missing(key)

    @staticmethod
    def _missing(key):
        raise KeyError(key)

    def _walk(self, text: str, key=None) -> int:
        q = int(self.start[self.segment(key)])
        for ch in text:
            if q < 0:
                return -1
            up = ch.upper() if self.case_insensitive else ch
            f = self._sym_id.get(up if len(up) == 1 else ch, -1)
            if f < 0:
                return -1
            e = int(self.next[q, f])
            q = e & 0xFFFFFF if e >= 0 else -1
        return q

    def accepts(self, text: str, key=None) -> bool:
        """does the segment's automaton accept `text` - a walk over the arrays, without the decoder's length rule (but a
        segment whose shortest string does not fit max_len has no start state and accepts nothing)"""
        q = self._walk(text, key)
        return q >= 0 and int(self.accept[q]) >= 0

    def tag(self, text: str, key=None) -> int:
        """`accept` of the state `text` leads to, -1 where it is not accepted"""
        q = self._walk(text, key)
        return int(self.accept[q]) if q >= 0 else -1
