"""The weighted-pattern beam search (evaluation/weighted_pattern.py, glass_beam_search_wdfa) restated in float64 on the CPU, and
its generated cases, for tests/test_weighted_pattern.py (CPU) and tests/test_gpu_weighted_beam.py.

Nothing here reads a product array.  The constraint is the dict trie over the ENUMERATED language of a case (as in
tests/pattern_cases.py; for a lexicon case, over its word list), and a candidate's weight comes from a callback on the emitted
prefix - `start()`, `symbol(prefix, ch)`, `stop(prefix)`, prefix and ch in fold keys - computed directly from the n-gram
model's dictionaries (`lm_score`, a brute-force back-off), the prior list (`PriorWeights`: maxima over the word list) and the
bonus; no automaton is involved.

`replay_with` is `lexicon_beam_cases.replay_with` with two float64 scores per slot: the model score m (running score +
log-softmax) and the weight sum a; a candidate's fused score is m' + scale * a'.  Selection, dead slots and finalisation are
those of the lexicon replay ON THE FUSED SCORE; both gaps are measured on it.
"""
import itertools
import math

import numpy as np
import torch

import beam_cases as BC
import lexicon_beam_cases as LC
import pattern_cases as PC

MARGIN, TOL = LC.MARGIN, LC.TOL
BOS, EOS = "<s>", "</s>"


def weight_bound(L, W):
    """the float32 accumulation bound of a fused score: the weight sum is L + 1 float32 additions at most (the start and one
    per step), the product and the fusion one rounding more - each within 2^-24 relative of a value no larger than
    W = max |scale * a|, |fused| along the hypothesis, hence 2 (L + 1) 2^-23 max(1, W) with room to spare"""
    return 2.0 * (L + 1) * 2.0 ** -23 * max(1.0, W)


# ------------------------------------------------------------------ weights, straight from their sources
def lm_score(logp, backoff, order, unk_logp, history, c):
    """ARPA back-off by brute force over the dictionaries: the longest suffix of the last order - 1 symbols of `history` for
    which the n-gram is stored, plus the back-offs of every longer suffix (0 where there is none)"""
    hist = tuple(history)[-(order - 1):] if order > 1 else ()
    for drop in range(len(hist) + 1):
        gram = hist[drop:] + (c,)
        if gram in logp:
            return sum(backoff.get(hist[j:], 0.0) for j in range(drop)) + logp[gram]
    return sum(backoff.get(hist[j:], 0.0) for j in range(len(hist))) + unk_logp


class LmWeights:
    def __init__(self, lm):
        self.args = (dict(lm.logp), dict(lm.backoff), lm.order, lm.unk_logp)

    def start(self):
        return 0.0

    def symbol(self, prefix, ch):
        return lm_score(*self.args, (BOS,) + tuple(prefix), ch)

    def stop(self, prefix):
        return lm_score(*self.args, (BOS,) + tuple(prefix), EOS)


class BonusWeights:
    def __init__(self, bonus):
        self.bonus = float(bonus)

    def start(self):
        return 0.0

    def symbol(self, prefix, ch):
        return self.bonus

    def stop(self, prefix):
        return 0.0


class PriorWeights:
    """`words`: the folded words of the item's segment that the search can spell, `priors`: their log-priors.  A prefix
    carries the best prior among the words it begins; a completed word its own (the best of equal words)."""

    def __init__(self, words, priors):
        self.words, self.priors = list(words), [float(p) for p in priors]
        self.memo = {}

    def best(self, prefix):
        if prefix not in self.memo:
            self.memo[prefix] = max(p for w, p in zip(self.words, self.priors) if w.startswith(prefix))
        return self.memo[prefix]

    def start(self):
        return self.best("")

    def symbol(self, prefix, ch):
        return self.best(prefix + ch) - self.best(prefix)

    def stop(self, prefix):
        return max(p for w, p in zip(self.words, self.priors) if w == prefix) - self.best(prefix)


class SumWeights:
    def __init__(self, parts):
        self.parts = list(parts)

    def start(self):
        return sum(p.start() for p in self.parts)

    def symbol(self, prefix, ch):
        return sum(p.symbol(prefix, ch) for p in self.parts)

    def stop(self, prefix):
        return sum(p.stop(prefix) for p in self.parts)

    def total(self, word):
        """the weight of a whole word: start, its symbols, the stop"""
        return self.start() + sum(self.symbol(word[:i], word[i]) for i in range(len(word))) + self.stop(word)


# ------------------------------------------------------------------ the replay
def replay_with(step, state, B, k, C, L, eos, keys, item_roots, item_weights, scale):
    """lexicon_beam_cases.replay_with with weights: item_weights [B] = the callback object of every item (None where the item
    has no root).  -> dict: symbols [B,k,L], scores [B,k] (fused), model_scores [B,k], lengths [B,k], words [B,k], step_scores
    [B,k,L] (model), W [B,k] (largest |scale * a| or |fused| along the hypothesis), sel_gap [B], done_gap [B], completed [B]"""
    run = torch.full((B, k), -math.inf, dtype=torch.float64)             # model scores
    acc = torch.zeros((B, k), dtype=torch.float64)                       # weight sums
    nodes = [[None] * k for _ in range(B)]
    prefixes = [[""] * k for _ in range(B)]
    for b in range(B):
        if item_roots[b] is not None:
            run[b, 0] = 0.0
            acc[b, 0] = item_weights[b].start()
            nodes[b][0] = item_roots[b]
    y_prev = torch.zeros((B * k,), dtype=torch.long)
    sc = torch.zeros((L, B, k), dtype=torch.float64)                     # model
    wa = torch.zeros((L, B, k), dtype=torch.float64)
    fu = torch.zeros((L, B, k), dtype=torch.float64)
    pr = torch.zeros((L, B, k), dtype=torch.long)
    sy = torch.zeros((L, B, k), dtype=torch.long)
    term = [[[None] * k for _ in range(B)] for _ in range(L)]
    sel_gap = torch.full((B,), math.inf, dtype=torch.float64)
    for t in range(L):
        logits, state = step(state, y_prev)
        lsm = torch.log_softmax(logits.detach().cpu().double().view(B, k, C), dim=2)
        for b in range(B):
            model = torch.full((k, C), -math.inf, dtype=torch.float64)
            wsum = torch.zeros((k, C), dtype=torch.float64)
            fused = torch.full((k, C), -math.inf, dtype=torch.float64)
            for r in range(k):
                if nodes[b][r] is not None and run[b, r] > -math.inf:
                    for c in range(C):
                        if LC.allowed(nodes[b][r], c, keys, eos):
                            w = item_weights[b].stop(prefixes[b][r]) if c == eos else item_weights[b].symbol(prefixes[b][r], keys[c])
                            model[r, c] = run[b, r] + lsm[b, r, c]
                            wsum[r, c] = acc[b, r] + w
                            fused[r, c] = model[r, c] + scale * wsum[r, c]
            model, wsum, fused = model.view(-1), wsum.view(-1), fused.view(-1)
            o = BC.order(fused)
            sel = o[:k]
            sc[t, b], wa[t, b], fu[t, b], pr[t, b], sy[t, b] = model[sel], wsum[sel], fused[sel], sel // C, sel % C
            if k < k * C and float(fused[o[k]]) > -math.inf:
                sel_gap[b] = min(float(sel_gap[b]), float(fused[o[k - 1]]) - float(fused[o[k]]))
            new, new_prefix = [], []
            for j in range(k):
                slot, c = int(pr[t, b, j]), int(sy[t, b, j])
                par = nodes[b][slot]
                if not float(fu[t, b, j]) > -math.inf:
                    new.append(None)
                    new_prefix.append("")
                elif c == eos:
                    term[t][b][j] = par
                    new.append(None)                      # the beam has ended
                    new_prefix.append("")
                else:
                    new.append(par["ch"][keys[c]])
                    new_prefix.append(prefixes[b][slot] + keys[c])
            nodes[b], prefixes[b] = new, new_prefix
            for j in range(k):
                run[b, j] = sc[t, b, j] if new[j] is not None else -math.inf
                acc[b, j] = wa[t, b, j] if new[j] is not None else 0.0
        flat = (pr[t] + torch.arange(B).view(B, 1) * k).view(-1)
        state = state.index_select(0, flat.to(state.device))
        y_prev = sy[t].reshape(-1).clone()
    sym = torch.full((B, k, L), eos, dtype=torch.long)
    scores = torch.full((B, k), -math.inf, dtype=torch.float64)
    model_scores = torch.full((B, k), -math.inf, dtype=torch.float64)
    lengths = torch.zeros((B, k), dtype=torch.long)
    words = torch.full((B, k), -1, dtype=torch.long)
    steps = torch.zeros((B, k, L), dtype=torch.float64)
    big = torch.zeros((B, k), dtype=torch.float64)
    done_gap = torch.full((B,), math.inf, dtype=torch.float64)
    completed = torch.zeros((B,), dtype=torch.long)
    for b in range(B):
        done = [(-float(fu[t, b, j]), t, j) for t in range(L) for j in range(k)
                if int(sy[t, b, j]) == eos and math.isfinite(float(fu[t, b, j]))]
        done.sort()
        completed[b] = len(done)
        for i in range(min(k, len(done) - 1)):
            done_gap[b] = min(float(done_gap[b]), done[i + 1][0] - done[i][0])
        for i, (neg, t, j) in enumerate(done[:k]):
            scores[b, i], model_scores[b, i], lengths[b, i], words[b, i] = -neg, sc[t, b, j], t + 1, term[t][b][j]["word"]
            slot = j
            for tt in range(t, -1, -1):
                sym[b, i, tt], steps[b, i, tt] = sy[tt, b, slot], sc[tt, b, slot]
                big[b, i] = max(float(big[b, i]), abs(scale * float(wa[tt, b, slot])), abs(float(fu[tt, b, slot])))
                slot = int(pr[tt, b, slot])
            big[b, i] = max(float(big[b, i]), abs(scale * item_weights[b].start()))
    return {"symbols": sym, "scores": scores, "model_scores": model_scores, "lengths": lengths, "words": words, "step_scores": steps,
            "W": big, "sel_gap": sel_gap, "done_gap": done_gap, "completed": completed}


def replay(sd, x, k, C, L, eos, keys, item_roots, item_weights, scale):
    """the weighted search in float64 from the state-dict weights: x [B,T,D] float32"""
    B = x.shape[0]
    f = BC.f64_step(sd, x, BC.xproj_f64(sd, x))
    item = torch.arange(B).repeat_interleave(k)
    return replay_with(lambda state, y: f(state, y, item), torch.zeros((B * k, 256), dtype=torch.float64), B, k, C, L, eos,
                       keys, item_roots, item_weights, scale)


# ------------------------------------------------------------------ the cases
C13 = PC.C13
_product = PC._product

AB_WORDS = ["ab", "abb", "ba", "aab", "b", "bab", "abab", "a"]                     # what the [ab]+ models are estimated from
MIX_WORDS = ["ab", "cd", "a0", "b1", "dc3", "0123", "abcd", "d", "c2", "33", "ba", "dab", "1a"]
AB63 = ["a" * n for n in (1, 2, 3, 63)]
T64_WORDS = ["a", "aa", "ab", "aab", "-1", "-0", "aaab", "-4"]
LEX = {"p": ["ab", "abc", "b", "ba", "c0", "cab", "a"], "q": ["0", "01", "2a", "b"]}     # a dict-lexicon over C13, two segments
LEX_PRIOR = {"p": [-9.0, -0.1, -9.0, -9.0, -9.0, -9.0, -9.0], "q": [-6.0, -2.0, -0.5, -6.0]}   # V(root): -0.1 / -0.5
TWIN = ["ab", "b", "AB", "ba", "Ab", "a"]                # case-insensitive: "ab", "AB" and "Ab" end at one node
TWIN_PRIOR = [-5.0, -3.0, -0.25, -4.0, -2.0, -6.0]


def _hi_words():
    h = PC._hi_chars()
    return [h[0] + h[1], h[2] + h[3] + h[4], h[4] + h[0], h[1] + h[1] + h[2], h[3] + h[0] + h[0] + h[1]]


# name -> a case of pattern_cases.CASES (regex cases: `patterns` + `candidates`) or a lexicon case (`lexicon`: word list or
# {key: list}; the pattern under test is DecodePattern.from_trie of it), plus the weights: `lm` = (training words, order) or
# None, `bonus`, `priors` (as the lexicon: a list or {key: list}), `scale` = weight_scale.  Shapes: the smallest that cross each
# boundary, from pattern_cases.CASES.  Seeds: the first of 100.. for which every item's fused gaps in the replay exceed
# MARGIN + weight_bound (test_weighted_pattern.py asserts it, on the replay alone).
CASES = {
    "k1_lm_c13_l4": dict(B=3, k=1, T=7, L=4, C=13, eos=1, seed=100, chars=C13, ci=False, patterns=r"[ab]+", item_keys=[None] * 3,
                         candidates={None: _product("abc", 1, 3)}, lm=(AB_WORDS, 3), scale=1.0),
    "trigram_ab_l5_k5": dict(B=3, k=5, T=7, L=5, C=13, eos=1, seed=100, chars=C13, ci=False, patterns=r"[ab]+", item_keys=[None] * 3,
                             candidates={None: _product("ab", 1, 4)}, lm=(AB_WORDS, 3), scale=0.8),
    "bonus_longest_l6_k4": dict(B=2, k=4, T=7, L=6, C=13, eos=1, seed=101, chars=C13, ci=False, patterns=r"[ab]+", item_keys=[None] * 2,
                                candidates={None: _product("ab", 1, 5)}, bonus=9.0, scale=1.0),
    "bonus_negative_l5_k3": dict(B=3, k=3, T=7, L=5, C=13, eos=1, seed=100, chars=C13, ci=False, patterns=r"(a|b)*c", item_keys=[None] * 3,
                                 candidates={None: _product("abc", 1, 4)}, bonus=-1.5, scale=1.0),
    "priors_reverse_k3": dict(B=3, k=3, T=7, L=5, C=13, eos=1, seed=100, chars=C13, ci=False, lexicon={"p": LEX["p"]},
                              item_keys=["p"] * 3, priors={"p": LEX_PRIOR["p"]}, scale=1.0),
    "priors_twins_ci_k4": dict(B=2, k=4, T=7, L=4, C=13, eos=1, seed=100, chars=C13, ci=True, lexicon=TWIN, item_keys=[None] * 2,
                               priors=TWIN_PRIOR, scale=1.5),
    "two_segments_start_w": dict(B=5, k=3, T=7, L=5, C=13, eos=1, seed=100, chars=C13, ci=False, lexicon=LEX,
                                 item_keys=["p", "q", -1, 2, "q"], priors=LEX_PRIOR, bonus=0.25, scale=1.0),
    "rows512_b32_k16": dict(B=32, k=16, T=7, L=5, C=97, eos=1, seed=101, chars="shipped", ci=False, patterns=r"[a-d0-3]+",
                            item_keys=[None] * 32, candidates={None: _product("abcd0123", 1, 4)}, lm=(MIX_WORDS, 3), bonus=0.5,
                            scale=1.0),
    "c256_identity": dict(B=2, k=5, T=7, L=5, C=256, eos=0, seed=100, chars="generic", ci=False,
                          patterns=lambda: "[" + "".join(PC._hi_chars()) + "]{2,}", item_keys=[None] * 2,
                          candidates={None: lambda: _product(PC._hi_chars(), 1, 4)()}, lm=(_hi_words, 2), bonus=-0.5, scale=1.0),
    "t64": dict(B=2, k=3, T=64, L=5, C=13, eos=1, seed=100, chars=C13, ci=False, patterns=r"a+b?|-\d", item_keys=[None] * 2,
                candidates={None: _product("ab-01234", 1, 4)}, lm=(T64_WORDS, 3), scale=1.0),
    "l64_a63": dict(B=2, k=2, T=7, L=64, C=13, eos=1, seed=100, chars=C13, ci=False, patterns=r"a{63}", item_keys=[None] * 2,
                    candidates={None: lambda: iter(["a" * n for n in range(1, 64)])}, fc_scale=0.25, boost={"a": 12.0},
                    lm=(AB63, 3), bonus=0.125, scale=1.0),
}
# a language of at most k words, each shorter than L - 1: the finite hypotheses are exactly the language
EXHAUSTIVE = {
    "exhaustive_k4": dict(B=3, k=4, T=7, L=6, C=13, eos=1, seed=100, chars=C13, ci=False, patterns=r"ab?|b1|-", item_keys=[None] * 3,
                          candidates={None: _product("ab1-", 1, 5)}, lm=(["ab", "a", "b1", "-", "ab", "b1"], 2), bonus=0.75, scale=2.0),
}
CASES.update(EXHAUSTIVE)
REVERSING = "priors_reverse_k3"          # the prior reverses the model's first choice for at least one item
LONGEST = "bonus_longest_l6_k4"          # the bonus makes the longest string win

_DATA = {}
_LMS = {}


def lm_of(case, alphabet=None):
    """the case's n-gram model (glass_amd.evaluation.weighted_pattern.CharNgramLM.estimate), or None"""
    from glass_amd.evaluation.weighted_pattern import CharNgramLM
    if case.get("lm") is None:
        return None
    words, order = case["lm"]
    words = words() if callable(words) else words
    key = (tuple(words), order)
    if key not in _LMS:
        _LMS[key] = CharNgramLM.estimate(words, order=order)
    return _LMS[key]


def _as_dict(v):
    return v if isinstance(v, dict) else {None: v}


def case_inputs(name, seed=None):
    """everything of a case but the replay (`seed`: another seed than the case's, for the seed search)"""
    c = CASES[name]
    B, k, T, L, C, eos = (c[n] for n in ("B", "k", "T", "L", "C", "eos"))
    chars = PC.characters_of(c)
    assert len(chars) == C and len(c["item_keys"]) == B
    keys = LC.class_keys(chars, eos, c["ci"])
    if "lexicon" in c:
        patterns, lexicon = None, _as_dict(c["lexicon"])
        names = list(lexicon)
        fold = (lambda w: w.upper()) if c["ci"] else (lambda w: w)
        words = {key: [fold(w) for w in lexicon[key]] for key in names}          # every word of LEX / TWIN is kept by the trie
    else:
        patterns, lexicon = PC.patterns_of(c), None
        as_dict = _as_dict(patterns)
        names = list(as_dict)
        words = {key: PC.language(rx, c["candidates"][key](), L, c["ci"]) for key, rx in as_dict.items()}
    roots, skipped, _ = LC.dict_tries({key: words[key] for key in names}, chars, L, eos, c["ci"])
    assert skipped == {"empty": 0, "too_long": 0, "no_class": 0}, skipped
    lm = lm_of(c)
    priors = _as_dict(c["priors"]) if "priors" in c else None
    weights = {}
    for key in names:
        parts = []
        if lm is not None:
            parts.append(LmWeights(lm))
        if c.get("bonus", 0.0):
            parts.append(BonusWeights(c["bonus"]))
        if priors is not None:
            parts.append(PriorWeights(words[key], priors[key]))
        weights[key] = SumWeights(parts)
    sd = BC.decoder_sd(C, fc_scale=c.get("fc_scale", 1.0), eos=eos)
    for ch, add in c.get("boost", {}).items():
        sd[BC.Q + "fc.bias"][chars.index(ch)] += float(add)
    x = BC.rand_x(B, T, c["seed"] if seed is None else seed)
    item_roots = [roots[names.index(key)] if key in names else None for key in c["item_keys"]]
    item_weights = [weights[key] if key in names else None for key in c["item_keys"]]
    return dict(B=B, k=k, T=T, L=L, C=C, eos=eos, sd=sd, x=x, characters=chars, ci=c["ci"], patterns=patterns, lexicon=lexicon,
                segment_names=names, item_keys=c["item_keys"], words=words, keys=keys, roots=roots, item_roots=item_roots,
                weights=weights, item_weights=item_weights, lm=lm, bonus=float(c.get("bonus", 0.0)), priors=c.get("priors"),
                scale=float(c["scale"]))


def case_data(name):
    """case_inputs + f64 (the float64 weighted replay).  Built once and shared; nothing in it is changed afterwards."""
    if name not in _DATA:
        d = case_inputs(name)
        d["f64"] = replay(d["sd"], d["x"], d["k"], d["C"], d["L"], d["eos"], d["keys"], d["item_roots"], d["item_weights"], d["scale"])
        _DATA[name] = d
    return _DATA[name]


def gaps_clear(d, f64):
    """the seed rule: every item's fused gaps exceed MARGIN + the weight bound of the case"""
    fin = torch.isfinite(f64["scores"])
    W = float(f64["W"][fin].max()) if fin.any() else 0.0
    return min(float(f64["sel_gap"].min()), float(f64["done_gap"].min())) > MARGIN + weight_bound(d["L"], W)


def unweighted_replay(d):
    """the same case without its weights: lexicon_beam_cases.replay on the same tries"""
    return LC.replay(d["sd"], d["x"], d["k"], d["C"], d["L"], d["eos"], d["keys"], d["item_roots"])


item_segments = PC.item_segments
text_of = PC.text_of


def strings_up_to(alphabet, n):
    return PC.strings_up_to(alphabet, n)


def alphabet_of(d):
    """the fold keys a string of the case can hold (for the exhaustive walks of the CPU test): those of its words, or a few"""
    seen = sorted({ch for ws in d["words"].values() for w in ws for ch in w})
    return seen[:4] if len(seen) > 4 else seen


def build_pattern(d, device):
    """the product under test: the DecodePattern of the case and its WeightedPattern"""
    from glass_amd.evaluation.lexicon import LexiconTrie
    from glass_amd.evaluation.pattern import DecodePattern
    if d["lexicon"] is not None:
        lex = d["lexicon"] if list(d["lexicon"]) != [None] else d["lexicon"][None]
        trie = LexiconTrie(lex, d["characters"], d["L"], d["eos"], case_insensitive=d["ci"], device=device)
        base = DecodePattern.from_trie(trie)
    else:
        base = DecodePattern(d["patterns"], d["characters"], d["L"], d["eos"], case_insensitive=d["ci"], device=device)
    return base, base.weighted(lm=d["lm"], word_logprior=d["priors"], length_bonus=d["bonus"])
