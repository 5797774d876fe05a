"""Lexicon-constrained beam search restated in float64 on the CPU, and the generated cases of its tests.

Nothing here reads the product's trie arrays: the lexicon is a dict-of-dicts trie (`dict_tries`), the allowed-class rule is
`allowed`, and `replay` / `replay_with` run the constrained search with `beam_cases.f64_step` (or a callback, so that a GPU
test can drive the arithmetic through `K.attention_decode_step`), float64 log-softmax and these rules:
  * candidate (beam r, class c) keeps its score if c != eos and the beam's node has a child for the class's fold symbol, or
    c == eos and a word ends at the node; everything else - and every candidate of a dead beam or of an item without a root -
    is -inf;
  * selection: score descending, then flat index beam*C + class ascending, -inf last in index order (`beam_cases.order`);
    a selected -inf candidate leaves a dead slot, a selected finite one moves to the child (eos: the search of that beam ends);
  * finalisation: the completed entries are the table entries (t, slot) with symbol eos and a finite score; the result is the
    k best by score descending, then t, then slot ascending, each walked back through the predecessor table; length t + 1,
    symbols from the length on eos, word = the first word that ends at the terminal node; missing hypotheses have score -inf,
    length 0, word -1 and all-eos symbols.
It also returns, per item, the smallest selection gap (k-th selected against the best finite candidate not selected, over
all steps) and the smallest gap between neighbouring completed entries in final order, down to the (k+1)-th.
"""
import math
import os

import numpy as np
import torch

import beam_cases as BC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the constants of tests/test_gpu_beam_search.py, measured there for the step arithmetic this search shares: symbols are
# compared exactly, so every item's gaps in the float64 replay must exceed MARGIN; scores and path rows agree within TOL
MARGIN = 10 * 3.6e-5
TOL = 1e-4
SPECIAL = ("[GO]", "[s]", "[UNK]", "[blank]")


def class_keys(characters, eos, case_insensitive=True):
    """fold key (a one-character string) of every class, None for a class no word can contain"""
    keys = []
    for c, ch in enumerate(characters):
        if c == eos or ch in SPECIAL or len(ch) != 1:
            keys.append(None)
        else:
            up = ch.upper() if case_insensitive else ch
            keys.append(up if len(up) == 1 else ch)
    return keys


def dict_tries(lexicon, characters, max_len, eos, case_insensitive=True):
    """-> (roots, skipped, upper): one dict trie per segment ({"ch": {key: node}, "word": first word index | -1}, None for
    a segment without a kept word), the left-out words per reason, the upper-cased words in file order"""
    lists = [list(lexicon[k]) for k in lexicon] if isinstance(lexicon, dict) else [list(lexicon)]
    known = {k for k in class_keys(characters, eos, case_insensitive) if k is not None}
    skipped = {"empty": 0, "too_long": 0, "no_class": 0}
    roots, upper, pos = [], [], 0
    for words in lists:
        root = {"ch": {}, "word": -1}
        kept = 0
        for j, w in enumerate(words):
            upper.append(w.upper())
            text = w.upper() if case_insensitive else w
            if not text:
                skipped["empty"] += 1
            elif len(text) > max_len - 1:
                skipped["too_long"] += 1
            elif any(ch not in known for ch in text):
                skipped["no_class"] += 1
            else:
                node = root
                for ch in text:
                    node = node["ch"].setdefault(ch, {"ch": {}, "word": -1})
                if node["word"] < 0:
                    node["word"] = pos + j
                kept += 1
        pos += len(words)
        roots.append(root if kept else None)
    return roots, skipped, upper


def allowed(node, c, keys, eos):
    """may a beam at `node` emit class c"""
    if node is None:
        return False
    if c == eos:
        return node["word"] >= 0
    return keys[c] is not None and keys[c] in node["ch"]


def replay_with(step, state, B, k, C, L, eos, keys, item_roots):
    """the constrained search with the decoder step from a callback: step(state [B*k,...], y_prev long [B*k]) -> (logits
    [B*k,C], state').  item_roots [B]: the dict trie of every item's segment, or None.
    -> dict: symbols [B,k,L], scores [B,k], lengths [B,k], words [B,k], step_scores [B,k,L], sel_gap [B], done_gap [B],
    completed [B] (number of completed entries)"""
    run = torch.full((B, k), -math.inf, dtype=torch.float64)
    nodes = [[None] * k for _ in range(B)]
    for b in range(B):
        if item_roots[b] is not None:
            run[b, 0] = 0.0
            nodes[b][0] = item_roots[b]
    y_prev = torch.zeros((B * k,), dtype=torch.long)
    sc = torch.zeros((L, B, k), dtype=torch.float64)
    pr = torch.zeros((L, B, k), dtype=torch.long)
    sy = torch.zeros((L, B, k), dtype=torch.long)
    term = [[[None] * k for _ in range(B)] for _ in range(L)]
    sel_gap = torch.full((B,), math.inf, dtype=torch.float64)
    for t in range(L):
        logits, state = step(state, y_prev)
        lsm = torch.log_softmax(logits.detach().cpu().double().view(B, k, C), dim=2)
        for b in range(B):
            cand = torch.full((k, C), -math.inf, dtype=torch.float64)
            for r in range(k):
                if nodes[b][r] is not None and run[b, r] > -math.inf:
                    ok = torch.tensor([allowed(nodes[b][r], c, keys, eos) for c in range(C)])
                    cand[r][ok] = run[b, r] + lsm[b, r][ok]
            cand = cand.view(-1)
            o = BC.order(cand)
            sel = o[:k]
            sc[t, b], pr[t, b], sy[t, b] = cand[sel], sel // C, sel % C
            if k < k * C and float(cand[o[k]]) > -math.inf:
                sel_gap[b] = min(float(sel_gap[b]), float(cand[o[k - 1]]) - float(cand[o[k]]))
            new = []
            for j in range(k):
                par, c = nodes[b][int(pr[t, b, j])], int(sy[t, b, j])
                if not float(sc[t, b, j]) > -math.inf:
                    new.append(None)
                elif c == eos:
                    term[t][b][j] = par
                    new.append(None)                      # the beam has ended
                else:
                    new.append(par["ch"][keys[c]])
            nodes[b] = new
            for j in range(k):
                run[b, j] = sc[t, b, j] if new[j] is not None else -math.inf
        flat = (pr[t] + torch.arange(B).view(B, 1) * k).view(-1)
        state = state.index_select(0, flat.to(state.device))
        y_prev = sy[t].reshape(-1).clone()
    sym = torch.full((B, k, L), eos, dtype=torch.long)
    scores = torch.full((B, k), -math.inf, dtype=torch.float64)
    lengths = torch.zeros((B, k), dtype=torch.long)
    words = torch.full((B, k), -1, dtype=torch.long)
    steps = torch.zeros((B, k, L), dtype=torch.float64)
    done_gap = torch.full((B,), math.inf, dtype=torch.float64)
    completed = torch.zeros((B,), dtype=torch.long)
    for b in range(B):
        done = [(-float(sc[t, b, j]), t, j) for t in range(L) for j in range(k)
                if int(sy[t, b, j]) == eos and math.isfinite(float(sc[t, b, j]))]
        done.sort()
        completed[b] = len(done)
        for i in range(min(k, len(done) - 1)):
            done_gap[b] = min(float(done_gap[b]), done[i + 1][0] - done[i][0])
        for i, (neg, t, j) in enumerate(done[:k]):
            scores[b, i], lengths[b, i], words[b, i] = -neg, t + 1, term[t][b][j]["word"]
            slot = j
            for tt in range(t, -1, -1):
                sym[b, i, tt], steps[b, i, tt] = sy[tt, b, slot], sc[tt, b, slot]
                slot = int(pr[tt, b, slot])
    return {"symbols": sym, "scores": scores, "lengths": lengths, "words": words, "step_scores": steps, "sel_gap": sel_gap,
            "done_gap": done_gap, "completed": completed}


def replay(sd, x, k, C, L, eos, keys, item_roots):
    """the constrained search in float64 from the state-dict weights: x [B,T,D] float32"""
    B = x.shape[0]
    f = BC.f64_step(sd, x, BC.xproj_f64(sd, x))
    item = torch.arange(B).repeat_interleave(k)
    return replay_with(lambda state, y: f(state, y, item), torch.zeros((B * k, 256), dtype=torch.float64), B, k, C, L, eos,
                       keys, item_roots)


# ------------------------------------------------------------------ the cases
def generic_characters(C):
    """the class strings of a decoder built with `beam_cases.decoder_cfg(C, .)`: Latin Extended-A from U+0100 on, where even
    code points are capitals and the next one is their small letter - so they fold in pairs unless case is kept"""
    return ["[GO]", "[s]"] + [chr(0x100 + i) for i in range(C - 2)]


def shipped_characters():
    from glass_amd.config import get_glass_cfg
    from glass_amd.modeling.recognition.text_encoder import TextEncoder
    cfg = get_glass_cfg(os.path.join(ROOT, "configs", "glass_icdar15_mi355x.yaml"), ["MODEL.DEVICE", "cpu"])
    return list(TextEncoder(cfg).character)


def random_words(rng, alphabet, n, lo, hi):
    return ["".join(alphabet[int(i)] for i in rng.integers(0, len(alphabet), int(rng.integers(lo, hi + 1)))) for _ in range(n)]


def _lex_l1(chars, rng):                 # max_len 1: no word fits, every item is without a completion
    return {"a": [chars[2], chars[3] + chars[4]]}, ["a"]


def _lex_c13(chars, rng):                # words of 1..3 characters (3 = ends at the last of 4 steps), two segments, all used
    al = chars[2:]
    return {"p": random_words(rng, al, 6, 1, 3) + [al[0] + al[1] + al[2]], "q": random_words(rng, al, 3, 2, 3)}, ["p", "q", "p"]


def _lex_shipped(chars, rng):
    """case folding on the shipped set; items in segments 0, 1, one past the end, the empty one, and the one whose only word
    has 25 characters (it ends at the last of 26 steps).  CAR / CARD: a terminal with children; with k = 3 and so few words
    several case variants of one word are alive at once (test_gpu_lexicon_beam.py asserts it)."""
    al = [c for c in chars[2:] if c.isalnum()]
    long_word = "".join(al[int(i)] for i in rng.integers(0, len(al), 25))
    lex = {"img1": ["car", "Card", "ca", "dog", "car"], "img2": ["Hello", "hELP", "he"], "none": [], "long": [long_word]}
    return lex, ["img1", "img2", 7, "none", "long"]


def _lex_mw8(chars, rng):                # identity fold over 254 symbols: 8 mask words, the words reach the last of them
    al = chars[2:]
    hi = al[-30:]
    return {"a": random_words(rng, hi, 4, 1, 4) + random_words(rng, al, 4, 2, 5), "b": random_words(rng, al, 12, 1, 5)}, ["a", "b"]


def _lex_rows512(chars, rng):            # 32 items over 4 segments of 30 words
    al = [c for c in chars[2:] if c.isalpha()]
    lex = {i: random_words(rng, al, 30, 1, 5) for i in range(4)}
    return lex, [i % 4 for i in range(32)]


def _lex_many(chars, rng):
    """40 words of one or two characters against k = 4.  With words of at most two characters the completed entries can never
    outnumber k (each of the k beams of step 1 ends at step 1 or at step 2), so every two-character word also gets two
    three-character extensions: then an item completes more words than the k it returns."""
    al = [c for c in chars[2:] if c.isdigit() or c.islower()]
    words = set()
    while len(words) < 40:
        words.update(random_words(rng, al, 1, 1, 2))
    words = sorted(words)
    longer = [w + al[int(i)] for w in words if len(w) == 2 for i in rng.integers(0, len(al), 2)]
    return words + sorted(set(longer)), [None, None]


def _lex_dead(chars, rng):               # identity fold, 3 words under k = 5: fewer allowed first symbols than k
    al = chars[2:]
    return {"a": [al[0] + al[1], al[0] + al[2] + al[1]], "b": [al[3]]}, ["a", "b", "a"]


def _lex_exh16(chars, rng):              # identity fold, at most 16 words per segment, all shorter than max_len - 1
    al = chars[2:12]
    return {"a": sorted(set(random_words(rng, al, 16, 1, 4))), "b": sorted(set(random_words(rng, al, 9, 1, 4)))}, ["a", "b", "a"]


# name -> (B, k, T, max_len, C, eos, seed, characters, case_insensitive, lexicon builder, fc_scale).  The smallest shapes that
# reach every path: k 1, 2, 3 (KB 4), 5 (KB 8), 16; C 5, 13, 97, 256; max_len 1, 4, 26; 512 state rows.  fc_scale is
# beam_cases.decoder_sd's.  The unconstrained tests use 6 (a sharp output layer separates the beams); a constrained search is
# FORCED along words the model finds unlikely, and at 6 their scores reach -380 in 6 steps, where one float32 rounding of the
# running sum is 3e-5 - a third of the tolerance per step, a property of the number format and not of the search.  At 1 (0.25
# for the 25-character word) every |score| stays under 120 (float64 replay: -18 .. -119), one rounding under 7.6e-6.
# Seeds: the first of 100.. for which every item's gaps in the float64 replay exceed MARGIN and the case has the property it
# is named for (k4_many_completions: every item completes more than k words) - properties of the inputs and the rules alone,
# asserted on the CPU by test_lexicon_beam.py
CASES = {
    "k1_c5_l1": (1, 1, 7, 1, 5, 0, 100, "generic", True, _lex_l1, 1.0),
    "k2_c13_l4": (3, 2, 7, 4, 13, 0, 100, "generic", False, _lex_c13, 1.0),
    "k3_c97_l26_shipped": (5, 3, 32, 26, 97, 1, 100, "shipped", True, _lex_shipped, 0.25),
    "k5_c256_l6_mw8": (2, 5, 7, 6, 256, 0, 100, "generic", False, _lex_mw8, 1.0),
    "k16_b32_l6_rows512": (32, 16, 7, 6, 97, 1, 100, "shipped", True, _lex_rows512, 1.0),
    "k4_many_completions": (2, 4, 7, 4, 97, 1, 101, "shipped", False, _lex_many, 1.0),
    "k5_dead_slots": (3, 5, 7, 6, 13, 0, 100, "generic", False, _lex_dead, 1.0),
    "k16_exhaustive": (3, 16, 7, 7, 21, 0, 100, "generic", False, _lex_exh16, 1.0),
}
EXHAUSTIVE = ("k5_dead_slots", "k16_exhaustive")      # identity fold, <= k words per segment, all shorter than max_len - 1

_DATA = {}


def case_data(name):
    """-> dict: B k T L C eos, sd, x [B,T,D] float32 (CPU), characters, case_insensitive, lexicon, item_keys (segment key of
    every item; an int that is no key = a segment number out of range), keys, roots, skipped, upper, f64 (the float64
    replay).  Built once and shared; nothing in it is changed afterwards."""
    if name not in _DATA:
        B, k, T, L, C, eos, seed, cs, ci, make, fc_scale = CASES[name]
        chars = generic_characters(C) if cs == "generic" else shipped_characters()
        assert len(chars) == C
        lexicon, item_keys = make(chars, np.random.default_rng(seed))
        assert len(item_keys) == B
        sd = BC.decoder_sd(C, fc_scale=fc_scale, eos=eos)
        x = BC.rand_x(B, T, seed)
        keys = class_keys(chars, eos, ci)
        roots, skipped, upper = dict_tries(lexicon, chars, L, eos, ci)
        names = list(lexicon) if isinstance(lexicon, dict) else [None]
        item_roots = [roots[names.index(key)] if key in names else None for key in item_keys]
        f64 = replay(sd, x, k, C, L, eos, keys, item_roots)
        _DATA[name] = dict(B=B, k=k, T=T, L=L, C=C, eos=eos, sd=sd, x=x, characters=chars, case_insensitive=ci, lexicon=lexicon,
                           item_keys=item_keys, segment_names=names, keys=keys, roots=roots, item_roots=item_roots,
                           skipped=skipped, upper=upper, f64=f64)
    return _DATA[name]


def item_segments(d):
    """segment number of every item of a case; a key that is no segment becomes len(segments) + 3 (out of range)"""
    names = d["segment_names"]
    return [names.index(key) if key in names else len(names) + 3 for key in d["item_keys"]]
