"""The fold-merged constrained beam searches (include/glass_hip_feature_merged.h, ASTER_V2.beam_decode(merge_case=True))
restated in float64 on the CPU, and their generated cases, for tests/test_merged_beam.py (CPU) and
tests/test_gpu_merged_beam.py.

Nothing here reads a product array, an automaton or a group array.  The constraint is the dict trie of
tests/lexicon_beam_cases.py over the ENUMERATED language of a case (or over its word list), the weights come from the
callbacks of tests/weighted_pattern_cases.py, and the merge is stated directly: the candidates of a beam whose classes share a
fold key (`keys[c]`: the upper-cased character, or a hand-made key) are ONE candidate whose model score is
run + log(sum exp(log-softmax)) over those classes, emitted as the likeliest of them (ties: the lowest class).

`replay_with` keeps the live beams of an item in a dict keyed by their FOLDED prefix - two beams with one folded prefix would
collide, which the search's invariant excludes (asserted) - next to the k slots the decoder step is batched over.  It measures
every margin its discrete decisions depend on: the k-th selected candidate against the best finite one left out (on the fused
score), the representative against the runner-up inside every selected group, and neighbouring completed entries in final
order down to the (k+1)-th.  `case_data` rejects a seed whose smallest margin is below MARGIN = 1e-3, ten times the score
tolerance of the neighbouring suites, so symbols, lengths and words can be compared exactly.
"""
import itertools
import math

import numpy as np
import torch

import beam_cases as BC
import lexicon_beam_cases as LC
import pattern_cases as PC
import weighted_pattern_cases as WC

MARGIN = 1e-3            # ten times TOL: every discrete decision of a case is at least this far from flipping
TOL = LC.TOL             # 1e-4, the model-score tolerance of the neighbouring suites
SEEDS = range(100, 108)  # the seeds a case may try, in order; at most half of the tried ones may be rejected
weight_bound = WC.weight_bound


class NoWeights:
    def start(self):
        return 0.0

    def symbol(self, prefix, ch):
        return 0.0

    def stop(self, prefix):
        return 0.0


def groups_of(keys):
    """{fold key: classes ascending}"""
    g = {}
    for c, key in enumerate(keys):
        if key is not None:
            g.setdefault(key, []).append(c)
    return g


def replay_with(step, state, B, k, C, L, eos, keys, item_roots, item_weights=None, scale=0.0, merge_dtype=torch.float64):
    """the merged search with the decoder step from a callback: step(state [B*k,...], y_prev long [B*k]) -> (logits [B*k,C],
    state').  keys [C]: fold key of every class (None: in no string); item_roots [B]: dict trie of every item, or None;
    item_weights [B]: the weight callbacks (None: unweighted); `merge_dtype`: the arithmetic of the merge (float32: as the
    device does it, for the kernel-driven replay).
    -> dict: symbols [B,k,L] (the representatives), folded [B][k] (folded strings; None for an absent hypothesis), scores [B,k]
    (fused), model_scores [B,k], lengths [B,k], words [B,k], step_scores [B,k,L] (model), W [B,k], margin [B] (the smallest of
    the three margins), completed [B]"""
    if item_weights is None:
        item_weights = [NoWeights() for _ in range(B)]
    groups = groups_of(keys)
    slots = [[None] * k for _ in range(B)]           # per slot: dict(prefix, node, run, acc, syms, steps, big) or None
    for b in range(B):
        if item_roots[b] is not None:
            a0 = item_weights[b].start()
            slots[b][0] = dict(prefix="", node=item_roots[b], run=0.0, acc=a0, syms=[], steps=[], big=abs(scale * a0))
    y_prev = torch.zeros((B * k,), dtype=torch.long)
    margin = torch.full((B,), math.inf, dtype=torch.float64)
    done = [[] for _ in range(B)]
    for t in range(L):
        logits, state = step(state, y_prev)
        lsm = torch.log_softmax(logits.detach().cpu().double().view(B, k, C), dim=2)
        parent = torch.zeros((B, k), dtype=torch.long)
        y_new = torch.zeros((B, k), dtype=torch.long)
        for b in range(B):
            cands = []
            for r, beam in enumerate(slots[b]):
                if beam is None:
                    continue
                w = item_weights[b]
                if beam["node"]["word"] >= 0 and t >= 1:
                    m = beam["run"] + float(lsm[b, r, eos])
                    a = beam["acc"] + w.stop(beam["prefix"])
                    cands.append(dict(fused=m + scale * a, model=m, acc=a, slot=r, cls=eos, key=None, rep_gap=math.inf))
                for key in beam["node"]["ch"]:
                    cls = groups[key]
                    vals = (beam["run"] + lsm[b, r, cls]).to(merge_dtype)
                    top = float(vals.max())
                    if not top > -math.inf:
                        continue                            # a group that is all -inf: no finite candidate
                    rep = cls[int(torch.nonzero(vals == vals.max())[0])]
                    rest = sorted((float(v) for v in vals), reverse=True)
                    m = float(torch.logsumexp(vals, 0)) if len(cls) > 1 else top
                    a = beam["acc"] + w.symbol(beam["prefix"], key)
                    cands.append(dict(fused=m + scale * a, model=m, acc=a, slot=r, cls=rep, key=key,
                                      rep_gap=rest[0] - rest[1] if len(rest) > 1 else math.inf))
            cands.sort(key=lambda c: (-c["fused"], c["slot"] * C + c["cls"]))     # ties: the flat index of the representative
            chosen = cands[:k]
            if len(cands) > k:
                margin[b] = min(float(margin[b]), chosen[-1]["fused"] - cands[k]["fused"])
            new = [None] * k
            live = {}
            for j, c in enumerate(chosen):
                margin[b] = min(float(margin[b]), c["rep_gap"])
                par = slots[b][c["slot"]]
                parent[b, j], y_new[b, j] = c["slot"], c["cls"]
                entry = dict(syms=par["syms"] + [c["cls"]], steps=par["steps"] + [c["model"]],
                             big=max(par["big"], abs(scale * c["acc"]), abs(c["fused"])))
                if c["key"] is None:
                    done[b].append(dict(entry, fused=c["fused"], model=c["model"], t=t, slot=j, prefix=par["prefix"],
                                        word=par["node"]["word"]))
                else:
                    prefix = par["prefix"] + c["key"]
                    assert prefix not in live, "two beams with one folded prefix"
                    live[prefix] = new[j] = dict(entry, prefix=prefix, node=par["node"]["ch"][c["key"]], run=c["model"], acc=c["acc"])
            slots[b] = new
        flat = (parent + torch.arange(B).view(B, 1) * k).view(-1)
        state = state.index_select(0, flat.to(state.device))
        y_prev = y_new.reshape(-1).clone()
    sym = torch.full((B, k, L), eos, dtype=torch.long)
    scores = torch.full((B, k), -math.inf, dtype=torch.float64)
    model_scores = torch.full((B, k), -math.inf, dtype=torch.float64)
    lengths = torch.zeros((B, k), dtype=torch.long)
    words = torch.full((B, k), -1, dtype=torch.long)
    steps = torch.zeros((B, k, L), dtype=torch.float64)
    big = torch.zeros((B, k), dtype=torch.float64)
    completed = torch.zeros((B,), dtype=torch.long)
    folded = [[None] * k for _ in range(B)]
    for b in range(B):
        done[b].sort(key=lambda e: (-e["fused"], e["t"], e["slot"]))
        completed[b] = len(done[b])
        for i in range(min(k, len(done[b]) - 1)):
            margin[b] = min(float(margin[b]), done[b][i]["fused"] - done[b][i + 1]["fused"])
        for i, e in enumerate(done[b][:k]):
            n = len(e["syms"])
            scores[b, i], model_scores[b, i], lengths[b, i], words[b, i], big[b, i] = e["fused"], e["model"], n, e["word"], e["big"]
            sym[b, i, :n] = torch.tensor(e["syms"])
            steps[b, i, :n] = torch.tensor(e["steps"], dtype=torch.float64)
            folded[b][i] = e["prefix"]
    return {"symbols": sym, "folded": folded, "scores": scores, "model_scores": model_scores, "lengths": lengths, "words": words,
            "step_scores": steps, "W": big, "margin": margin, "completed": completed}


def replay(sd, x, k, C, L, eos, keys, item_roots, item_weights=None, scale=0.0):
    """the merged search in float64 from the state-dict weights: x [B,T,D] float32"""
    B = x.shape[0]
    f = BC.f64_step(sd, x, BC.xproj_f64(sd, x))
    item = torch.arange(B).repeat_interleave(k)
    return replay_with(lambda state, y: f(state, y, item), torch.zeros((B * k, 256), dtype=torch.float64), B, k, C, L, eos,
                       keys, item_roots, item_weights, scale)


# ------------------------------------------------------------------ the cases
C13 = PC.C13                                  # a small hand-made class set: a/A and b/B fold, eos = 1
_product = PC._product
TWINS = ["car", "Card", "CAR", "ca", "dog", "Dog", "do", "cat", "cart", "dot", "dig", "CaT"]     # case twins in the lexicon
FEW = ["ab", "Ab", "b1", "-"]                                                                    # three folded words
SEGS = {"p": ["ab", "AB", "ba", "b", "a1", "A1b"], "none": []}
LONG = ["hello", "Hello", "help", "HELP", "he", "world", "word", "wor", "w0rd", "World2", "a", "A1", "zebra", "Zed", "zoo",
        "x", "xy", "xyz", "XYZ0", "q1", "Q12", "q123", "hel", "helm"]

# name -> dict(B k T L C eos chars ci, then `patterns` + `candidates` (regex / charset cases, as pattern_cases.CASES) or
# `lexicon` (from_trie cases), item_keys, optionally bonus / priors / scale (weighted cases) and `charset` (the pattern under
# test is DecodePattern.from_charset of it)).  Shapes as in pattern_cases / lexicon_beam_cases: a handful of items, T 7 or 32,
# the real C = 97 or the hand-made 13 classes.  k covers every row block: 1, 2, 3 (KB 4), 5 and 8 (KB 8), 16.
# `seed`: the first of SEEDS whose margins clear MARGIN; `tried`: how many were tried (test_merged_beam.py re-derives both).
CASES = {
    "charset_k1_c13": dict(B=3, k=1, T=7, L=4, C=13, eos=1, chars=C13, ci=True, charset="ab1", patterns=r"[ab1]+",
                           item_keys=[None] * 3, candidates={None: _product("AB1", 1, 3)}),
    "star_k2_c13": dict(B=3, k=2, T=7, L=5, C=13, eos=1, chars=C13, ci=True, patterns=r"(a|b)*1", item_keys=[None] * 3,
                        candidates={None: _product("AB1", 1, 4)}),
    "alt_repeat_k3_c97": dict(B=3, k=3, T=7, L=6, C=97, eos=1, chars="shipped", ci=True, patterns=r"(ab|cd){1,2}e?|x[01]{1,2}",
                              item_keys=[None] * 3, candidates={None: _product("ABCDEX01", 1, 5)}),
    "trie_twins_k5_c97": dict(B=3, k=5, T=7, L=6, C=97, eos=1, chars="shipped", ci=True, lexicon=TWINS, item_keys=[None] * 3),
    "repeat_k8_c97": dict(B=2, k=8, T=7, L=5, C=97, eos=1, chars="shipped", ci=True, patterns=r"[a-c]{1,3}[01]?",
                          item_keys=[None] * 2, candidates={None: _product("ABC01", 1, 4)}),
    "charset_k16_c97": dict(B=4, k=16, T=7, L=5, C=97, eos=1, chars="shipped", ci=True, charset="abcd01", patterns=r"[abcd01]+",
                            item_keys=[None] * 4, candidates={None: _product("ABCD01", 1, 4)}),
    "bonus_k3_c13": dict(B=3, k=3, T=7, L=5, C=13, eos=1, chars=C13, ci=True, patterns=r"[ab]+", item_keys=[None] * 3,
                         candidates={None: _product("AB", 1, 4)}, bonus=0.7, scale=1.0),
    "priors_twins_k4_c13": dict(B=2, k=4, T=7, L=4, C=13, eos=1, chars=C13, ci=True, lexicon=WC.TWIN, item_keys=[None] * 2,
                                priors=WC.TWIN_PRIOR, scale=1.5),
    "exhausted_k5_c13": dict(B=3, k=5, T=7, L=6, C=13, eos=1, chars=C13, ci=True, lexicon=FEW, item_keys=[None] * 3),
    "empty_segment_k2_c13": dict(B=4, k=2, T=7, L=5, C=13, eos=1, chars=C13, ci=True, lexicon=SEGS, item_keys=["p", "none", 5, "p"]),
    "long_k16_c97_t32_l26": dict(B=2, k=16, T=32, L=26, C=97, eos=1, chars="shipped", ci=True, lexicon=LONG, item_keys=[None] * 2,
                                 fc_scale=0.25),
    "sensitive_k5_c97": dict(B=2, k=5, T=7, L=5, C=97, eos=1, chars="shipped", ci=False, patterns=r"[abAB]{1,3}",
                             item_keys=[None] * 2, candidates={None: _product("abAB", 1, 4)}),
}
for _name, _seed, _tried in (("charset_k1_c13", 100, 1), ("star_k2_c13", 100, 1), ("alt_repeat_k3_c97", 100, 1),
                             ("trie_twins_k5_c97", 100, 1), ("repeat_k8_c97", 100, 1), ("charset_k16_c97", 101, 2),
                             ("bonus_k3_c13", 100, 1), ("priors_twins_k4_c13", 100, 1), ("exhausted_k5_c13", 100, 1),
                             ("empty_segment_k2_c13", 100, 1), ("long_k16_c97_t32_l26", 100, 1), ("sensitive_k5_c97", 100, 1)):
    CASES[_name].update(seed=_seed, tried=_tried)
WEIGHTED = ("bonus_k3_c13", "priors_twins_k4_c13")
EXHAUSTED = "exhausted_k5_c13"           # three folded words under k = 5
EMPTY = "empty_segment_k2_c13"           # items 1 (an empty segment) and 2 (a segment out of range) have no hypothesis

_DATA = {}


def case_inputs(name, seed=None):
    """everything of a case but the replay, as weighted_pattern_cases.case_inputs lays it out"""
    c = CASES[name]
    B, k, T, L, C, eos = (c[n] for n in ("B", "k", "T", "L", "C", "eos"))
    chars = PC.characters_of(c)
    assert len(chars) == C and len(c["item_keys"]) == B
    keys = LC.class_keys(chars, eos, c["ci"])
    fold = (lambda w: w.upper()) if c["ci"] else (lambda w: w)
    if "lexicon" in c:
        patterns, lexicon = None, WC._as_dict(c["lexicon"])
        names = list(lexicon)
        words = {key: [fold(w) for w in lexicon[key]] for key in names}
    else:
        patterns, lexicon = c["patterns"], None
        names = [None]
        words = {None: PC.language(patterns, c["candidates"][None](), L, c["ci"])}
    roots, skipped, _ = LC.dict_tries({key: words[key] for key in names}, chars, L, eos, c["ci"])
    assert skipped == {"empty": 0, "too_long": 0, "no_class": 0}, skipped
    priors = WC._as_dict(c["priors"]) if "priors" in c else None
    weights = {}
    for key in names:
        parts = []
        if c.get("bonus", 0.0):
            parts.append(WC.BonusWeights(c["bonus"]))
        if priors is not None:
            parts.append(WC.PriorWeights(words[key], priors[key]))
        weights[key] = WC.SumWeights(parts)
    sd = BC.decoder_sd(C, fc_scale=c.get("fc_scale", 1.0), eos=eos)
    x = BC.rand_x(B, T, c["seed"] if seed is None else seed)
    item_roots = [roots[names.index(key)] if key in names else None for key in c["item_keys"]]
    item_weights = [weights[key] if key in names else NoWeights() for key in c["item_keys"]]
    return dict(B=B, k=k, T=T, L=L, C=C, eos=eos, sd=sd, x=x, characters=chars, ci=c["ci"], patterns=patterns, lexicon=lexicon,
                charset=c.get("charset"), segment_names=names, item_keys=c["item_keys"], words=words, keys=keys, roots=roots,
                item_roots=item_roots, weights=weights, item_weights=item_weights, bonus=float(c.get("bonus", 0.0)),
                priors=c.get("priors"), scale=float(c.get("scale", 0.0)), weighted=name in WEIGHTED)


def replay_of(d):
    return replay(d["sd"], d["x"], d["k"], d["C"], d["L"], d["eos"], d["keys"], d["item_roots"], d["item_weights"], d["scale"])


def find_seed(name):
    """-> (seed, tried, f64): the first of SEEDS whose smallest margin clears MARGIN; AssertionError if more than half of the
    tried seeds were rejected (one try is allowed to succeed at once) or none clears"""
    tried = 0
    for seed in SEEDS:
        tried += 1
        d = case_inputs(name, seed)
        f64 = replay_of(d)
        if float(f64["margin"].min()) >= MARGIN:
            assert 2 * (tried - 1) <= tried, (name, f"{tried - 1} of {tried} seeds rejected")
            return seed, tried, f64
    raise AssertionError(f"{name}: no seed of {list(SEEDS)} clears the margin {MARGIN}")


def case_data(name):
    """case_inputs + f64 (the float64 merged replay) at the committed seed, whose margins must clear MARGIN.  Built once and
    shared; nothing in it is changed afterwards."""
    if name not in _DATA:
        d = case_inputs(name)
        d["f64"] = replay_of(d)
        smallest = float(d["f64"]["margin"].min())
        assert smallest >= MARGIN, (name, CASES[name]["seed"], smallest)
        _DATA[name] = d
    return _DATA[name]


item_segments = PC.item_segments
text_of = PC.text_of


def build_pattern(d, device, case_insensitive=None):
    """the product under test: the DecodePattern of the case (weighted for a weighted case); `case_insensitive`: override the
    case's own mode (the neutrality tests build case-sensitive twins)"""
    from glass_amd.evaluation.lexicon import LexiconTrie
    from glass_amd.evaluation.pattern import DecodePattern
    ci = d["ci"] if case_insensitive is None else case_insensitive
    if d["lexicon"] is not None:
        lex = d["lexicon"] if list(d["lexicon"]) != [None] else d["lexicon"][None]
        base = DecodePattern.from_trie(LexiconTrie(lex, d["characters"], d["L"], d["eos"], case_insensitive=ci, device=device))
    elif d["charset"] is not None:
        base = DecodePattern.from_charset(d["charset"], d["characters"], d["L"], d["eos"], case_insensitive=ci, device=device)
    else:
        base = DecodePattern(d["patterns"], d["characters"], d["L"], d["eos"], case_insensitive=ci, device=device)
    return base.weighted(word_logprior=d["priors"], length_bonus=d["bonus"]) if d["weighted"] else base


# ------------------------------------------------------------------ hand-made groups of three and four
# 13 classes, eos = 0.  Fold symbols by hand (no case folding produces these): a group of three that holds class 1 (class 0's
# neighbour) and class 12 (the last class), a group of four, two single classes, and a group of two whose output-layer biases
# are -inf, so that it is all -inf in every row; classes 11 and the stop have no symbol.  The language is every string of
# 1 .. L - 1 symbols: ONE accepting state with a loop on every symbol.
HAND = dict(B=3, k=5, T=7, L=5, C=13, eos=0, seed=100, tried=1,
            fold=[-1, 0, 1, 1, 2, 0, 3, 1, 4, 1, 4, -1, 0], dead_symbol=4)
HAND_KEYS = [None if f < 0 else "PQRST"[f] for f in HAND["fold"]]


def hand_inputs(seed=None):
    c = HAND
    B, k, T, L, C, eos = (c[n] for n in ("B", "k", "T", "L", "C", "eos"))
    F = max(c["fold"]) + 1
    words = ["".join(w) for n in range(1, L) for w in itertools.product("PQRST"[:F], repeat=n)]
    root = {"ch": {}, "word": -1}
    for i, w in enumerate(words):
        node = root
        for ch in w:
            node = node["ch"].setdefault(ch, {"ch": {}, "word": -1})
        node["word"] = 0                                   # the tag of the one accepting state
    sd = BC.decoder_sd(C, fc_scale=1.0, eos=eos)
    for cls, f in enumerate(c["fold"]):
        if f == c["dead_symbol"]:
            sd[BC.Q + "fc.bias"][cls] = -math.inf
    x = BC.rand_x(B, T, c["seed"] if seed is None else seed)
    group_cls = sorted((cl for cl, f in enumerate(c["fold"]) if f >= 0), key=lambda cl: (c["fold"][cl], cl))
    group_start = [sum(1 for f in c["fold"] if 0 <= f < s) for s in range(F + 1)]
    tables = dict(next=np.zeros((1, F), dtype=np.int32), accept=np.zeros(1, dtype=np.int32), start=np.zeros(1, dtype=np.int32),
                  fold=np.asarray(c["fold"], dtype=np.int32), group_start=np.asarray(group_start, dtype=np.int32),
                  group_cls=np.asarray(group_cls, dtype=np.int32), F=F)
    return dict(B=B, k=k, T=T, L=L, C=C, eos=eos, sd=sd, x=x, keys=HAND_KEYS, item_roots=[root] * B, tables=tables, F=F)


def hand_data():
    if "hand" not in _DATA:
        d = hand_inputs()
        d["f64"] = replay(d["sd"], d["x"], d["k"], d["C"], d["L"], d["eos"], d["keys"], d["item_roots"])
        assert float(d["f64"]["margin"].min()) >= MARGIN, float(d["f64"]["margin"].min())
        _DATA["hand"] = d
    return _DATA["hand"]


# ------------------------------------------------------------------ the known answer: equal twins
KNOWN = dict(B=3, k=8, T=7, L=6, C=97, eos=1, seed=100, words=["ab", "a1", "7", "b2c", "42", "cab", "0"])


def known_sd():
    """decoder weights in which the output-layer rows, biases and embedding rows of every lower-case class are copies of its
    upper-case twin's: every letter group then splits its mass evenly, whatever the state"""
    chars = LC.shipped_characters()
    sd = BC.decoder_sd(KNOWN["C"], fc_scale=1.0, eos=KNOWN["eos"])
    for name in ("fc.weight", "fc.bias", "tgt_embedding.weight"):
        sd[BC.Q + name] = sd[BC.Q + name].clone()
    for c, ch in enumerate(chars):
        if len(ch) == 1 and ch.islower() and ch.upper() in chars:
            up = chars.index(ch.upper())
            sd[BC.Q + "fc.weight"][c] = sd[BC.Q + "fc.weight"][up]
            sd[BC.Q + "fc.bias"][c] = sd[BC.Q + "fc.bias"][up]
            sd[BC.Q + "tgt_embedding.weight"][c] = sd[BC.Q + "tgt_embedding.weight"][up]
    return sd, chars
