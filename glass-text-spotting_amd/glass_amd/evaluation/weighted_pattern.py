"""Weighted patterns: a `DecodePattern` with a weight (a natural log) on every transition, on every stop and on the start of
every segment - what glass_beam_search_wdfa (include/glass_hip_feature_wdfa.h) adds, times `weight_scale`, to the score its
beams are ranked by (`ASTER_V2.beam_decode(pattern=WeightedPattern, weight_scale=...)`, `RecognizerRCNNHeadV3.set_pattern`).
Shallow fusion: the model's own score and the path rows made from it stay what they were.

`DecodePattern.weighted(lm=None, word_logprior=None, length_bonus=0.0)` builds one; the three sources add.

`length_bonus=b`: every symbol transition weighs b (the stop and the start 0): a string of n characters carries n * b, against
the bias of a sum of log-probabilities toward short strings.  The states are the pattern's.

`word_logprior` (a `DecodePattern.from_trie` pattern only): log-priors of the words, a float array over `trie.upper` (file
order) or a dict {key: array over the segment's words}.  The prior P(q) of a state where words end is the maximum over the
words that end there; words the trie left out are ignored.  The weights are PUSHED toward the root in the tropical (max, +)
semiring: with V(q) = the maximum of P over the accepting states at or below q,
    start_w = V(root),   w(q -> q') = V(q') - V(q),   final_w(q) = P(q) - V(q),
so a prefix always carries the best prior still reachable below it - the look-ahead that keeps a likely word in a narrow beam
- and a completed word carries exactly its prior.

`lm` (`CharNgramLM`): the automaton becomes the product of the pattern's states with the model's contexts (strings of fold
symbols: with case_insensitive=True the model is trained on upper-cased words).  Only pairs reachable from the start states
are built, numbered breadth-first from the start states in segment order, fold symbols ascending; the context of a state is
the last order - 1 symbols read (with <s> in front of a word), and
    w((q, h), f) = lm.score(h, f),   final_w((q, h)) = lm.score(h, </s>),   start_w = 0;
tags and distances are the pattern's.  There is no minimisation.  A trie keeps its states: every node has one history.

Weights are built in float64 (`weight64` [N,F], `final64` [N], `start64` [S]) and uploaded as their float32 roundings, the
transition weights interleaved with `next` (`trans` int32 [N,F,2]: one 64-bit load per (beam, class)).  ValueError for any
weight that is not finite (in float32 too) and for an argument that does not fit the pattern.
"""
from __future__ import annotations

import math
import time
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .pattern import DIST_FIELD_MAX, MAX_STATES, NEXT_TABLE_CAP_BYTES, DecodePattern

WEIGHTED_TABLE_CAP_BYTES = 2 * NEXT_TABLE_CAP_BYTES   # most bytes of `trans`: what fits unweighted fits with its weights
BOS, EOS = "<s>", "</s>"
UNK_LOGP = -23.0                                      # log-probability of a symbol the model has no unigram for (about 1e-10)


class CharNgramLM:
    """A back-off n-gram model over single characters with ARPA semantics, natural logs.

    `logp[ngram]`: log p(last symbol | the symbols before it); `backoff[context]`: the back-off weight of a context; n-grams
    and contexts are tuples of symbols - one-character strings, `<s>` (only in front of a word) and `</s>` (only predicted).
    `score(h, c)` uses the longest suffix of `h` (its last order - 1 symbols at most) for which the n-gram is stored, adds the
    back-offs of the longer contexts that failed (a missing one is 0) and `unk_logp` for a symbol without a unigram."""

    def __init__(self, order: int, logp: Dict[Tuple[str, ...], float], backoff: Optional[Dict[Tuple[str, ...], float]] = None,
                 unk_logp: float = UNK_LOGP):
        self.order = int(order)
        if self.order < 1:
            raise ValueError(f"CharNgramLM: order {order} (at least 1)")
        self.logp = {tuple(g): float(v) for g, v in logp.items()}
        self.backoff = {tuple(h): float(v) for h, v in (backoff or {}).items()}
        self.unk_logp = float(unk_logp)
        for g in self.logp:
            if not 1 <= len(g) <= self.order:
                raise ValueError(f"CharNgramLM: n-gram {g!r} does not fit order {self.order}")

    def context(self, history: Sequence[str]) -> Tuple[str, ...]:
        """what `score` reads of a history: its last order - 1 symbols"""
        h = tuple(history)
        return h[len(h) - (self.order - 1):] if len(h) > self.order - 1 else h

    def score(self, history: Sequence[str], symbol: str) -> float:
        h = self.context(history)
        total = 0.0
        while True:
            v = self.logp.get(h + (symbol,))
            if v is not None:
                return total + v
            if not h:
                return total + self.unk_logp
            total += self.backoff.get(h, 0.0)
            h = h[1:]

    def word_score(self, word: Iterable[str]) -> float:
        """log p(word </s> | <s>), term by term in reading order"""
        h: Tuple[str, ...] = (BOS,)
        total = 0.0
        for c in list(word) + [EOS]:
            total += self.score(h, c)
            h = h + (c,)
        return total

    @classmethod
    def from_arpa(cls, text: str, unk_logp: float = UNK_LOGP) -> "CharNgramLM":
        """the standard ARPA text form: `\\data\\`, `ngram n=count` lines, `\\n-grams:` sections of
        `log10 p <tab> symbols separated by blanks [<tab> log10 back-off]`, `\\end\\`; log10 becomes ln"""
        ln10 = math.log(10.0)
        logp: Dict[Tuple[str, ...], float] = {}
        backoff: Dict[Tuple[str, ...], float] = {}
        n, order, seen_data = 0, 0, False
        for raw in text.splitlines():
            line = raw.strip()
            if not line:
                continue
            if line == "\\data\\":
                seen_data = True
            elif line == "\\end\\":
                break
            elif line.startswith("ngram ") and "=" in line:
                order = max(order, int(line[6:].split("=")[0]))
            elif line.startswith("\\") and line.endswith("-grams:"):
                n = int(line[1:-len("-grams:")])
                order = max(order, n)
            elif n > 0:
                tok = line.split()
                if len(tok) not in (n + 1, n + 2):
                    raise ValueError(f"CharNgramLM.from_arpa: {raw!r} is no {n}-gram line")
                gram = tuple(tok[1:n + 1])
                for s in gram:
                    if len(s) != 1 and s not in (BOS, EOS):
                        raise ValueError(f"CharNgramLM.from_arpa: symbol {s!r} is not a single character, {BOS} or {EOS}")
                logp[gram] = float(tok[0]) * ln10
                if len(tok) == n + 2:
                    backoff[gram] = float(tok[n + 1]) * ln10
        if not seen_data or order < 1:
            raise ValueError("CharNgramLM.from_arpa: no \\data\\ section or no n-grams")
        return cls(order, logp, backoff, unk_logp)

    @classmethod
    def estimate(cls, words: Iterable[str], order: int = 3, discount: float = 0.75, alphabet: Optional[Iterable[str]] = None,
                 unk_logp: float = UNK_LOGP) -> "CharNgramLM":
        """interpolated absolute discounting on the words' characters, each word read as <s> c1 .. cn </s>:
            p(c | h) = max(n(hc) - d, 0) / n(h) + d T(h) / n(h) p(c | h-),
        n(h) = the count of h as a context, T(h) = its distinct continuations, h- = h without its oldest symbol; below the
        unigram comes the uniform distribution over `alphabet` (default: the characters of the words) and </s>.  Stored in
        the back-off form: logp of every seen n-gram (and of every unigram of the alphabet), backoff[h] = log(d T(h) / n(h))."""
        order, d = int(order), float(discount)
        if order < 1 or not 0.0 < d < 1.0:
            raise ValueError(f"CharNgramLM.estimate: needs order >= 1 and 0 < discount < 1 (got {order}, {discount})")
        words = [list(w) for w in words]
        vocab = sorted(set(alphabet) if alphabet is not None else {c for w in words for c in w})
        if any(len(c) != 1 for c in vocab):
            raise ValueError("CharNgramLM.estimate: the alphabet must hold single characters")
        known = set(vocab)
        for w in words:
            if any(c not in known for c in w):
                raise ValueError(f"CharNgramLM.estimate: {''.join(w)!r} holds a character outside the alphabet")
        vocab.append(EOS)
        count: List[Dict[Tuple[str, ...], Dict[str, int]]] = [dict() for _ in range(order)]      # [len(h)][h][c]
        for w in words:
            s = [BOS] + w + [EOS]
            for i in range(1, len(s)):
                for m in range(min(order - 1, i) + 1):
                    by_c = count[m].setdefault(tuple(s[i - m:i]), {})
                    by_c[s[i]] = by_c.get(s[i], 0) + 1
        prob: Dict[Tuple[str, ...], float] = {}
        logp: Dict[Tuple[str, ...], float] = {}
        backoff: Dict[Tuple[str, ...], float] = {}
        uni = count[0].get((), {})
        total = sum(uni.values())
        for c in vocab:
            below = 1.0 / len(vocab)
            prob[(c,)] = (max(uni.get(c, 0) - d, 0.0) / total + d * len(uni) / total * below) if total else below
            logp[(c,)] = math.log(prob[(c,)])

        def p_of(h: Tuple[str, ...], c: str) -> float:
            """p(c | h) of the estimate, for any context"""
            v = prob.get(h + (c,))
            if v is not None:
                return v
            by_c = count[len(h)].get(h)
            lower = p_of(h[1:], c)
            return d * len(by_c) / sum(by_c.values()) * lower if by_c else lower

        for m in range(1, order):
            for h in sorted(count[m]):
                by_c = count[m][h]
                nh = sum(by_c.values())
                backoff[h] = math.log(d * len(by_c) / nh)
                for c in sorted(by_c):
                    prob[h + (c,)] = (by_c[c] - d) / nh + d * len(by_c) / nh * p_of(h[1:], c)
                    logp[h + (c,)] = math.log(prob[h + (c,)])
        return cls(order, logp, backoff, unk_logp)


class WeightedPattern(DecodePattern):
    """`DecodePattern.weighted(...)`: the pattern with its weights (module docstring).  It is a DecodePattern - keys, segments,
    `accepts` / `tag`, `next` / `accept` / `start` / `dist` / `fold` as there (of the product automaton with an `lm`) - plus
      `weight64` float64 [N,F] (0 where there is no transition), `final64` float64 [N] (0 for a state that does not accept),
        `start64` float64 [S] (0 for a segment without a start state);
      `trans` int32 [N,F,2]: `next`, then the bits of float32(weight64);  `final_w` / `start_w`: float32 of the other two;
      `base_state` int32 [N]: the state of the pattern it was built from;  `contexts`: with an `lm`, every state's context;
      `tensors`: trans, final_w, start_w, accept, start, fold (and the fold groups, group_start / group_cls) on the device,
        and the int "F".
    Limits (ValueError): N <= 2^24 - 1, `trans` at most `table_cap_bytes`."""

    def __init__(self, base: DecodePattern, lm: Optional[CharNgramLM] = None, word_logprior=None, length_bonus: float = 0.0,
                 table_cap_bytes: int = WEIGHTED_TABLE_CAP_BYTES, device=None):
        t0 = time.perf_counter()
        if isinstance(base, WeightedPattern):
            raise ValueError("WeightedPattern: the pattern is weighted already (weight the DecodePattern it was built from)")
        if lm is not None and not isinstance(lm, CharNgramLM):
            raise ValueError(f"WeightedPattern: lm must be a CharNgramLM (got {type(lm).__name__})")
        bonus = float(length_bonus)
        if not math.isfinite(bonus):
            raise ValueError(f"WeightedPattern: length_bonus {length_bonus} is not finite")
        for name in ("keys", "patterns", "minimize", "num_classes", "max_len", "eos", "case_insensitive", "fold_symbols", "num_fold",
                     "_sym_id", "word_state", "segment_sizes"):
            setattr(self, name, getattr(base, name))
        if hasattr(base, "_characters"):
            self._characters = base._characters
        self.fold = base.fold.copy()
        self.lm, self.length_bonus = lm, bonus
        F = self.num_fold
        target = np.where(base.next >= 0, base.next & 0xFFFFFF, -1).astype(np.int64)         # [N0, F]
        prior = self._pushed_priors(base, target, word_logprior)                              # (start, V, P - V) of the base, or None
        cap_states = max(min(MAX_STATES, int(table_cap_bytes) // (8 * F)), 0)
        if lm is None:
            nxt, state_of, start = target, np.arange(base.num_states, dtype=np.int64), base.start.astype(np.int64)
            weight = np.zeros(nxt.shape, dtype=np.float64)
            final = np.zeros(nxt.shape[0], dtype=np.float64)
            self.contexts = None
        else:
            nxt, state_of, start, weight, final, self.contexts = self._product(base, target, lm, cap_states)
        N = nxt.shape[0]
        if N > MAX_STATES:
            raise ValueError(f"WeightedPattern: automaton of {N} states (the limit is 2^24 - 1 = {MAX_STATES})")
        if N * F * 8 > int(table_cap_bytes):
            raise ValueError(f"WeightedPattern: transition table of {N} x {F} entries = {N * F * 8} bytes (the table limit is "
                             f"{int(table_cap_bytes)} bytes)")
        has = nxt >= 0
        weight = np.where(has, weight + bonus, 0.0)
        start64 = np.zeros(len(start), dtype=np.float64)
        if prior is not None:
            root_w, V, P = prior
            weight = np.where(has, weight + (V[state_of[np.maximum(nxt, 0)]] - V[state_of][:, None]), 0.0)
            final = final + np.where(base.accept[state_of] >= 0, P[state_of] - V[state_of], 0.0)
            start64 = np.where(start >= 0, root_w, 0.0)
        self.base_state = state_of.astype(np.int32)
        self.accept = np.ascontiguousarray(base.accept[state_of], dtype=np.int32)
        self.dist = np.ascontiguousarray(base.dist[state_of], dtype=np.int32)
        self.start = np.ascontiguousarray(start, dtype=np.int32)
        field = np.minimum(self.dist, DIST_FIELD_MAX).astype(np.int64)
        self.next = np.where(has, nxt | (field[np.maximum(nxt, 0)] << 24), -1).astype(np.int32)
        self.num_states = N
        self.weight64, self.final64, self.start64 = weight, np.where(self.accept >= 0, final, 0.0), start64
        with np.errstate(over="ignore"):
            w32, self.final_w, self.start_w = (a.astype(np.float32) for a in (self.weight64, self.final64, self.start64))
        for name, a in (("transition", w32), ("stop", self.final_w), ("start", self.start_w)):
            if not np.isfinite(a).all():
                raise ValueError(f"WeightedPattern: a {name} weight is not finite")
        self.trans = np.ascontiguousarray(np.stack([self.next, w32.view(np.int32)], axis=2))
        self.nbytes = int(self.trans.nbytes + self.final_w.nbytes + self.start_w.nbytes + self.accept.nbytes + self.start.nbytes +
                          self.fold.nbytes)
        self.device = torch.device(device) if device is not None else base.device
        self.tensors = {n: torch.from_numpy(getattr(self, n)).to(self.device) for n in ("trans", "final_w", "start_w", "accept", "start",
                                                                                        "fold")}
        self.tensors["F"] = F
        self._upload_groups()
        self.build_seconds = time.perf_counter() - t0

    # ---- word priors, pushed toward the root
    @staticmethod
    def _pushed_priors(base: DecodePattern, target: np.ndarray, word_logprior):
        if word_logprior is None:
            return None
        if base.word_state is None:
            raise ValueError("WeightedPattern: word_logprior needs a pattern built with DecodePattern.from_trie")
        if isinstance(word_logprior, dict):
            if set(word_logprior.keys()) != set(base.keys) or len(word_logprior) != len(base.keys):
                raise ValueError(f"WeightedPattern: word_logprior has keys {list(word_logprior)}, the pattern {list(base.keys)}")
            parts = [np.asarray(word_logprior[k], dtype=np.float64).reshape(-1) for k in base.keys]
            for k, part, size in zip(base.keys, parts, base.segment_sizes):
                if len(part) != size:
                    raise ValueError(f"WeightedPattern: word_logprior[{k!r}] has {len(part)} entries, the segment {size} words")
            logprior = np.concatenate(parts) if parts else np.zeros(0)
        else:
            logprior = np.asarray(word_logprior, dtype=np.float64).reshape(-1)
        if len(logprior) != len(base.word_state):
            raise ValueError(f"WeightedPattern: word_logprior has {len(logprior)} entries, the lexicon {len(base.word_state)} words")
        kept = base.word_state >= 0
        if not np.isfinite(logprior[kept]).all():
            raise ValueError("WeightedPattern: a word's log-prior is not finite")
        N0 = base.num_states
        P = np.full(N0, -np.inf, dtype=np.float64)
        np.maximum.at(P, base.word_state[kept], logprior[kept])
        V = P.copy()
        src, f = np.nonzero(target >= 0)
        tgt = target[src, f]
        for _ in range(base.max_len + 1):                 # a trie is no deeper than max_len - 1
            new = V.copy()
            np.maximum.at(new, src, V[tgt])
            if np.array_equal(new, V):
                break
            V = new
        # every node of a trie has a word below it; the one state of an empty automaton has none and no start points to it
        V = np.where(np.isfinite(V), V, 0.0)
        P = np.where(np.isfinite(P), P, 0.0)
        root_w = np.where(base.start >= 0, V[np.maximum(base.start, 0)], 0.0)
        return root_w, V, P

    # ---- the product with the contexts of an n-gram model
    @staticmethod
    def _product(base: DecodePattern, target: np.ndarray, lm: CharNgramLM, cap_states: int):
        F = base.num_fold
        symbols = list(base.fold_symbols)
        keep = lm.order - 1
        ids: Dict[Tuple[int, Tuple[str, ...]], int] = {}
        order: List[Tuple[int, Tuple[str, ...]]] = []
        cache: Dict[Tuple[Tuple[str, ...], str], float] = {}

        def score(h, c):
            v = cache.get((h, c))
            if v is None:
                v = cache[(h, c)] = lm.score(h, c)
            return v

        def state(q, h):
            i = ids.get((q, h))
            if i is None:
                if len(order) >= cap_states:
                    raise ValueError(f"WeightedPattern: the product automaton needs more than {cap_states} states (the limit of "
                                     "2^24 - 1 states and of the table's bytes)")
                i = ids[(q, h)] = len(order)
                order.append((q, h))
            return i

        h0 = lm.context((BOS,))
        edges = [np.nonzero(row >= 0)[0] for row in target]
        rows_t: List[np.ndarray] = []
        rows_w: List[np.ndarray] = []
        start = []
        head = 0
        for s in base.start:
            if s < 0:
                start.append(-1)
                continue
            start.append(state(int(s), h0))
            while head < len(order):                      # breadth-first, fold symbols ascending
                q, h = order[head]
                t_row, w_row = np.full(F, -1, dtype=np.int64), np.zeros(F, dtype=np.float64)
                for f in edges[q]:
                    c = symbols[f]
                    w_row[f] = score(h, c)
                    h2 = (h + (c,))[-keep:] if keep else ()
                    t_row[f] = state(int(target[q, f]), h2)
                rows_t.append(t_row)
                rows_w.append(w_row)
                head += 1
        if not order:                                     # no start state at all: the one state of an empty automaton
            return (np.full((1, F), -1, dtype=np.int64), np.zeros(1, dtype=np.int64), np.asarray(start, dtype=np.int64),
                    np.zeros((1, F)), np.zeros(1), [()])
        final = np.asarray([score(h, EOS) for _, h in order], dtype=np.float64)
        return (np.stack(rows_t), np.asarray([q for q, _ in order], dtype=np.int64), np.asarray(start, dtype=np.int64),
                np.stack(rows_w), final, [h for _, h in order])

    # ---- queries
    def weight_of(self, text: str, key=None) -> Optional[float]:
        """start64 + the walked weight64 + final64 of an accepted string, in float64; None where it is not accepted"""
        q = int(self.start[self.segment(key)])
        if q < 0:
            return None
        total = float(self.start64[self.segment(key)])
        for ch in text:
            up = ch.upper() if self.case_insensitive else ch
            f = self._sym_id.get(up if len(up) == 1 else ch, -1)
            if f < 0 or self.next[q, f] < 0:
                return None
            total += float(self.weight64[q, f])
            q = int(self.next[q, f]) & 0xFFFFFF
        return total + float(self.final64[q]) if self.accept[q] >= 0 else None
