"""Cases on which the six decoder searches meet EXACT score ties, for tests/test_search_tie_cases.py (CPU) and
tests/test_gpu_search_ties.py.

Every search states one selection rule - score descending, then flat index beam*C + class ascending, -inf candidates last in
index order - and its finalisation a rule of its own (back-tracking: value, then slot; completed entries: score, then
t*k + slot).  The neighbouring suites compare symbols exactly and therefore keep every selection at least MARGIN away from a tie.
Here the ties are the point, so they have to be ties in ANY arithmetic, the device's float32 included:

  * the FLAT decoder: fc.weight = 0 and fc.bias = a vector of a few levels.  The logits are the bias whatever the state and
    the input, every beam's log-softmax row is one vector, and two candidates tie exactly when their scores are the same
    sequence of additions (all live beams descend from equally scored ancestors), or differ by commuting two terms;
  * the TWIN decoder: real weights in which the output row and bias of every lower-case class are copies of its upper-case
    twin's (the embedding rows are NOT copied: two beams that differ in case have different states).  'a' and 'A' tie inside
    every beam; the float64 step computes the upper-case logit and copies it to the twin, so that the equality does not rest
    on how a host matrix product orders its sums.

`restate` is the search of the existing replays written once more for all six searches with the accumulation run + lsm in a
chosen dtype: float64 must reproduce the existing replay (the reference of every comparison), float32 is the device's order of
additions.  It also lists, per step, the neighbouring candidates in rule order from the first selected down to the best one
not selected, and the neighbouring final scores / completed entries; `condition` requires each such pair to be exactly equal
in both arithmetics or more than MARGIN apart, and both arithmetics to reach the same decision tables.  A case that fails is
replaced, not excused.
"""
import itertools
import math

import torch

import beam_cases as BC
import lexicon_beam_cases as LC
import merged_beam_cases as MC
import pattern_cases as PC
import weighted_pattern_cases as WC

MARGIN, TOL = LC.MARGIN, LC.TOL
B, T = 3, 7
TOP, SECOND, LOW = 0.0, -1.0, -8.0               # the bias levels of a flat decoder: log-softmax gaps of 1 and 7
C13 = PC.C13                                      # [GO] [s] a b c 0 1 2 3 4 - A B, eos = 1
AB3 = ["".join(w) for n in (1, 2, 3) for w in itertools.product("ab", repeat=n)]
TRIE13 = ["a", "b", "A", "B", "ab", "aA", "bA", "Ab", "AA", "ba"]
TWIN_WORDS = ["car", "card", "ca", "dog", "do", "cat", "cart", "dot", "dig"]
SEEDS = range(100, 116)

# name -> dict(search, decoder, C, k, L, eos, ...).  search: plain | lexicon | dfa | wdfa | merged | merged_w.
# flat decoders: `top` / `second` = the classes of the two upper levels (every other class is LOW), or `only` = the one class
# with a finite bias.  k 2, 3, 5, 16 and k == C: the row blockings 2, 4 (one padding row), 8 (three), 16 (none; three).
CASES = {
    # ---- the plain search on flat decoders
    # <eos> first of the top level: slot 0 ends at every step, the hypotheses are "ended at step t", t = 0, 1, ...
    "flat_c13_k2_eos_first": dict(search="plain", decoder="flat", C=13, k=2, L=4, eos=0, top=[0, 3, 7, 11]),
    # <eos> in the middle of the top level
    "flat_c13_k3_eos_mid": dict(search="plain", decoder="flat", C=13, k=3, L=6, eos=5, top=[2, 5, 6, 9]),
    # <eos> never chosen: all k final scores are equal, both sorts of the back-tracking are decided by slot
    "flat_c13_k5_eos_low": dict(search="plain", decoder="flat", C=13, k=5, L=6, eos=0, top=[1, 4, 6, 8, 10, 12]),
    # k == C: step 0 takes every class, the levels in order and each level by index; step 1 ties lA + lB with lB + lA
    "flat_c13_k13": dict(search="plain", decoder="flat", C=13, k=13, L=3, eos=0, top=[1, 4, 7], second=[2, 9]),
    # two waves, tied classes either side of class 64
    "flat_c97_k16_two_waves": dict(search="plain", decoder="flat", C=97, k=16, L=3, eos=41, top=list(range(1, 97, 5))),
    # fewer top classes than k: step 0 fills the beam from the second level by index, step 1 cuts inside the cross-beam ties
    # lA + lB (beams 0, 1) = lB + lA (beams 2 ..); from step 2 on every selected beam descends from lA + lA again
    "flat_c97_k5_two_levels_l2": dict(search="plain", decoder="flat", C=97, k=5, L=2, eos=64, top=[10, 80], second=[5, 30, 64, 90]),
    "flat_c97_k5_two_levels_l6": dict(search="plain", decoder="flat", C=97, k=5, L=6, eos=64, top=[10, 80], second=[5, 30, 64, 90]),
    # one top class in each of the four waves and k = 3 tied beams: in round 1 of step 1 wave 0 nominates beam 1 (its class of
    # beam 0 is taken) and waves 1 - 3 hold lower flat indices than wave 0
    "flat_c256_k3_four_waves": dict(search="plain", decoder="flat", C=256, k=3, L=4, eos=255, top=[5, 70, 130, 200]),
    # only <eos> has a finite bias: after step 0 all k*C candidates are -inf and are taken in index order
    "flat_c13_k3_all_ended": dict(search="plain", decoder="flat", C=13, k=3, L=3, eos=0, only=0),
    # ---- the constrained searches on flat decoders: the allowed classes are the tied ones
    "flat_trie_k3": dict(search="lexicon", decoder="flat", C=13, k=3, L=4, eos=1, top=[1, 2, 3, 11, 12], chars=C13, ci=False,
                         lexicon=TRIE13),
    # six allowed classes under k = 5 (with k or fewer, either tie-break would keep the same set)
    "flat_star_k5": dict(search="dfa", decoder="flat", C=13, k=5, L=4, eos=1, top=[1, 2, 3, 4, 5, 11, 12], chars=C13, ci=False,
                         regex=r"[abc0AB]+", candidates=PC._product("abc0AB", 1, 3)),
    # equal weights on the tied transitions and a weight_scale that is not 1: the fused scores tie
    "flat_bonus_k3": dict(search="wdfa", decoder="flat", C=13, k=3, L=4, eos=1, top=[1, 2, 3, 11, 12], chars=C13, ci=False,
                          lexicon=TRIE13, bonus=0.5, scale=0.75),
    # two fold groups of two classes (a/A, b/B) that tie as groups: the lower representative's flat index wins
    "flat_merged_k3": dict(search="merged", decoder="flat", C=13, k=3, L=4, eos=1, top=[1, 2, 3, 11, 12], chars=C13, ci=True,
                           lexicon=AB3),
    "flat_merged_bonus_k3": dict(search="merged_w", decoder="flat", C=13, k=3, L=4, eos=1, top=[1, 2, 3, 11, 12], chars=C13, ci=True,
                                 lexicon=AB3, bonus=0.5, scale=0.75),
    # ---- twin decoders (97 shipped classes, eos = 1): `seed` = the first of SEEDS that meets `condition` with a decisive tie
    "twin_plain_k3": dict(search="plain", decoder="twin", C=97, k=3, L=6, eos=1, fc_scale=6.0, seed=101),
    "twin_plain_k5": dict(search="plain", decoder="twin", C=97, k=5, L=6, eos=1, fc_scale=2.0, seed=100),
    # case-insensitive and NOT merged: 'c' and 'C' are both allowed at every letter and k cuts between them
    "twin_trie_k3": dict(search="lexicon", decoder="twin", C=97, k=3, L=6, eos=1, fc_scale=1.0, seed=100, chars="shipped", ci=True,
                         lexicon=TWIN_WORDS),
    "twin_star_k5": dict(search="dfa", decoder="twin", C=97, k=5, L=5, eos=1, fc_scale=1.0, seed=100, chars="shipped", ci=True,
                         regex=r"[ab]+", candidates=PC._product("AB", 1, 4)),
    "twin_bonus_k3": dict(search="wdfa", decoder="twin", C=97, k=3, L=6, eos=1, fc_scale=1.0, seed=100, chars="shipped", ci=True,
                          lexicon=TWIN_WORDS, bonus=0.5, scale=0.75),
}
WEIGHTED = ("wdfa", "merged_w")
MERGED = ("merged", "merged_w")


# ------------------------------------------------------------------ the two decoders
def flat_sd(c):
    """decoder weights whose logits are a bias of levels: fc.weight = 0"""
    sd = BC.decoder_sd(c["C"], eos=c["eos"])
    sd[BC.Q + "fc.weight"] = torch.zeros_like(sd[BC.Q + "fc.weight"])
    if "only" in c:
        bias = torch.full((c["C"],), -math.inf)
        bias[c["only"]] = 0.0
    else:
        bias = torch.full((c["C"],), LOW)
        bias[c.get("second", [])] = SECOND
        bias[c["top"]] = TOP
    sd[BC.Q + "fc.bias"] = bias.to(sd[BC.Q + "fc.bias"].dtype)
    return sd


def flat_step(sd):
    """-> step(state, y_prev) of a flat decoder in float64: the bias (times the temperature), whatever the state"""
    temp = float(sd[BC.Q + "temperature"].reshape(-1)[0]) if (BC.Q + "temperature") in sd else 1.0
    row = sd[BC.Q + "fc.bias"].double() * temp
    return lambda state, y_prev: (row.expand(state.shape[0], -1), state)


def twin_pairs(chars):
    """(lower-case class, upper-case class) of every letter both of whose cases are classes"""
    return [(c, chars.index(ch.upper())) for c, ch in enumerate(chars)
            if len(ch) == 1 and ch.islower() and ch.upper() != ch and ch.upper() in chars]


def twin_sd(c, chars):
    sd = BC.decoder_sd(c["C"], fc_scale=c["fc_scale"], eos=c["eos"])
    for name in ("fc.weight", "fc.bias"):
        sd[BC.Q + name] = sd[BC.Q + name].clone()
    for lo, up in twin_pairs(chars):
        sd[BC.Q + "fc.weight"][lo] = sd[BC.Q + "fc.weight"][up]
        sd[BC.Q + "fc.bias"][lo] = sd[BC.Q + "fc.bias"][up]
    return sd


def twin_step(sd, x, k, chars):
    """-> step(state, y_prev) in float64 from the weights; the lower-case logits are COPIES of their twins', not recomputed"""
    f = BC.f64_step(sd, x, BC.xproj_f64(sd, x))
    item = torch.arange(x.shape[0]).repeat_interleave(k)
    lo = torch.tensor([p[0] for p in twin_pairs(chars)])
    up = torch.tensor([p[1] for p in twin_pairs(chars)])

    def step(state, y_prev):
        logits, state = f(state, y_prev, item)
        logits = logits.clone()
        logits[:, lo] = logits[:, up]
        return logits, state
    return step


# ------------------------------------------------------------------ the searches, restated with the accumulation in `dtype`
def restate(step, state, B, k, C, L, eos, dtype, keys=None, item_roots=None, item_weights=None, scale=0.0, merge=False):
    """keys None: the plain search (beam_cases); else the search under the dict tries `item_roots` (lexicon_beam_cases), with
    `item_weights` ranked by model + scale * weights (weighted_pattern_cases), with `merge` the classes of one fold key as one
    candidate at their arg-max class (merged_beam_cases).  The log-softmax is float64 rounded to `dtype`; running scores,
    weight sums, merged and fused scores are computed in `dtype`.
    -> dict: symbols, scores (fused), model_scores, lengths, words, pr, sy (decision tables [L,B,k]), step_pairs [(hi, lo, cut)]
    (neighbouring candidates in rule order, first selected .. best not selected; cut = lo is that one), final_pairs [(hi, lo)]"""
    plain, weighted = keys is None, item_weights is not None
    ninf = -math.inf
    run = torch.full((B, k), ninf, dtype=dtype)
    acc = torch.zeros((B, k), dtype=dtype)
    nodes = [[None] * k for _ in range(B)]
    prefixes = [[""] * k for _ in range(B)]
    groups = MC.groups_of(keys) if not plain else None
    for b in range(B):
        if plain or item_roots[b] is not None:
            run[b, 0] = 0.0
            nodes[b][0] = True if plain else item_roots[b]
            if weighted:
                acc[b, 0] = item_weights[b].start()
    y_prev = torch.zeros((B * k,), dtype=torch.long)
    sc = torch.zeros((L, B, k), dtype=dtype)
    wa = torch.zeros((L, B, k), dtype=dtype)
    fu = torch.zeros((L, B, k), dtype=dtype)
    pr = torch.zeros((L, B, k), dtype=torch.long)
    sy = torch.zeros((L, B, k), dtype=torch.long)
    term = [[[None] * k for _ in range(B)] for _ in range(L)]
    step_pairs, final_pairs = [], []
    for t in range(L):
        logits, state = step(state, y_prev)
        lsm = torch.log_softmax(logits.detach().cpu().double().view(B, k, C), dim=2).to(dtype)
        for b in range(B):
            model = torch.full((k, C), ninf, dtype=dtype)
            wsum = torch.zeros((k, C), dtype=dtype)
            for r in range(k):
                if nodes[b][r] is None or not float(run[b, r]) > ninf:
                    continue
                cand = run[b, r] + lsm[b, r]
                if plain:
                    model[r] = cand
                    continue
                node, w = nodes[b][r], item_weights[b] if weighted else None
                if node["word"] >= 0:
                    model[r, eos] = cand[eos]
                    if weighted:
                        wsum[r, eos] = acc[b, r] + torch.tensor(w.stop(prefixes[b][r]), dtype=dtype)
                for key in node["ch"]:
                    cls = groups[key]
                    wk = acc[b, r] + torch.tensor(w.symbol(prefixes[b][r], key), dtype=dtype) if weighted else 0.0
                    if merge and len(cls) > 1:
                        vals = cand[cls]
                        if not float(vals.max()) > ninf:
                            continue
                        rep = cls[int(torch.nonzero(vals == vals.max())[0])]
                        model[r, rep], wsum[r, rep] = torch.logsumexp(vals, 0), wk
                    else:
                        for c in cls:
                            model[r, c], wsum[r, c] = cand[c], wk
            model, wsum = model.view(-1), wsum.view(-1)
            # ONE rounding of model + scale * sum, as the device's fused multiply-add: the sum in float64, then to dtype
            fused = (model.double() + scale * wsum.double()).to(dtype) if weighted else model
            o = BC.order(fused)
            sel = o[:k]
            sc[t, b], wa[t, b], fu[t, b], pr[t, b], sy[t, b] = model[sel], wsum[sel], fused[sel], sel // C, sel % C
            for i in range(min(k, k * C - 1)):
                step_pairs.append((float(fused[o[i]]), float(fused[o[i + 1]]), i == k - 1))
            new, new_prefix = [], []
            for j in range(k):
                slot, c = int(pr[t, b, j]), int(sy[t, b, j])
                if not float(fu[t, b, j]) > ninf or c == eos:
                    if float(fu[t, b, j]) > ninf and not plain:
                        term[t][b][j] = nodes[b][slot]
                    new.append(None)
                    new_prefix.append("")
                elif plain:
                    new.append(True)
                    new_prefix.append("")
                else:
                    new.append(nodes[b][slot]["ch"][keys[c]])
                    new_prefix.append(prefixes[b][slot] + keys[c])
            nodes[b], prefixes[b] = new, new_prefix
            for j in range(k):
                run[b, j] = sc[t, b, j] if new[j] is not None else ninf
                acc[b, j] = wa[t, b, j] if new[j] is not None else 0.0
        flat = (pr[t] + torch.arange(B).view(B, 1) * k).view(-1)
        state = state.index_select(0, flat.to(state.device))
        y_prev = sy[t].reshape(-1).clone()
    out = {"pr": pr, "sy": sy, "step_pairs": step_pairs, "final_pairs": final_pairs}
    if plain:
        sym, scores, lengths, _ = BC.backtrack(sc.double(), pr, sy, eos)
        for b in range(B):
            final_pairs.extend((float(scores[b, i]), float(scores[b, i + 1])) for i in range(k - 1))
        out.update(symbols=sym, scores=scores, model_scores=scores, lengths=lengths, words=None)
        return out
    sym = torch.full((B, k, L), eos, dtype=torch.long)
    scores = torch.full((B, k), ninf, dtype=torch.float64)
    model_scores = torch.full((B, k), ninf, dtype=torch.float64)
    lengths = torch.zeros((B, k), dtype=torch.long)
    words = torch.full((B, k), -1, dtype=torch.long)
    for b in range(B):
        done = sorted((-float(fu[t, b, j]), t, j) for t in range(L) for j in range(k)
                      if int(sy[t, b, j]) == eos and math.isfinite(float(fu[t, b, j])))
        final_pairs.extend((-done[i][0], -done[i + 1][0]) for i in range(min(k, len(done) - 1)))
        for i, (neg, t, j) in enumerate(done[:k]):
            scores[b, i], model_scores[b, i], lengths[b, i], words[b, i] = -neg, sc[t, b, j], t + 1, term[t][b][j]["word"]
            slot = j
            for tt in range(t, -1, -1):
                sym[b, i, tt] = sy[tt, b, slot]
                slot = int(pr[tt, b, slot])
    out.update(symbols=sym, scores=scores, model_scores=model_scores, lengths=lengths, words=words)
    return out


def condition(r64, r32, margin):
    """the property every case must have (see the module's docstring).  -> dict of counts: ties (finite pairs that are exactly
    equal), decisive (of them: the k-th selected against the best one not selected), decisive_ninf (that cut between two -inf
    candidates), final_ties.  AssertionError where a pair is neither equal in both arithmetics nor more than `margin` apart,
    or where the two arithmetics decide differently."""
    for n in ("pr", "sy", "symbols", "lengths"):
        assert torch.equal(r64[n], r32[n]), f"float64 and float32 decide differently ({n})"
    assert (r64["words"] is None and r32["words"] is None) or torch.equal(r64["words"], r32["words"])
    count = dict(ties=0, decisive=0, decisive_ninf=0, final_ties=0)
    assert len(r64["step_pairs"]) == len(r32["step_pairs"]) and len(r64["final_pairs"]) == len(r32["final_pairs"])
    for (hi, lo, cut), (hi32, lo32, _) in zip(r64["step_pairs"], r32["step_pairs"]):
        assert (lo == -math.inf) == (lo32 == -math.inf) and (hi == -math.inf) == (hi32 == -math.inf)
        if lo == -math.inf:
            count["decisive_ninf"] += cut and hi == -math.inf
            continue
        assert (hi == lo and hi32 == lo32) or (hi - lo > margin and hi32 > lo32), ("a near-tie between candidates", hi, lo, hi32, lo32)
        count["ties"] += hi == lo
        count["decisive"] += cut and hi == lo
    for (hi, lo), (hi32, lo32) in zip(r64["final_pairs"], r32["final_pairs"]):
        if lo == -math.inf:
            continue
        assert (hi == lo and hi32 == lo32) or (hi - lo > margin and hi32 > lo32), ("a near-tie between final scores", hi, lo, hi32, lo32)
        count["final_ties"] += hi == lo
    return count


# ------------------------------------------------------------------ case data
_DATA = {}


def case_inputs(name, seed=None):
    """everything of a case but the replays: B k T L C eos search, sd, x [B,T,D] float32 (CPU), step (the float64 decoder step),
    state0, and for a constrained search characters, ci, lexicon (the word list the dict trie holds; for a regex its
    enumerated language), regex, keys, item_roots, item_weights, bonus, scale, margin"""
    c = CASES[name]
    k, L, C, eos = (c[n] for n in ("k", "L", "C", "eos"))
    x = BC.rand_x(B, T, c.get("seed", 100) if seed is None else seed)
    chars = LC.shipped_characters() if c.get("chars", "shipped") == "shipped" else list(c["chars"])
    if c["decoder"] == "flat":
        sd = flat_sd(c)
        step, state0 = flat_step(sd), torch.zeros((B * k, 1), dtype=torch.float64)
    else:
        assert len(chars) == C
        sd = twin_sd(c, chars)
        step, state0 = twin_step(sd, x, k, chars), torch.zeros((B * k, 256), dtype=torch.float64)
    d = dict(name=name, search=c["search"], B=B, k=k, T=T, L=L, C=C, eos=eos, sd=sd, x=x, step=step, state0=state0, keys=None,
             item_roots=None, item_weights=None, scale=0.0, bonus=0.0, margin=MARGIN, merge=c["search"] in MERGED)
    if c["search"] == "plain":
        return d
    assert len(chars) == C
    ci = c["ci"]
    words = list(c["lexicon"]) if "lexicon" in c else PC.language(c["regex"], c["candidates"](), L, ci)
    keys = LC.class_keys(chars, eos, ci)
    roots, skipped, _ = LC.dict_tries(words, chars, L, eos, ci)
    assert skipped == {"empty": 0, "too_long": 0, "no_class": 0}, skipped
    d.update(characters=chars, ci=ci, lexicon=c.get("lexicon"), regex=c.get("regex"), words=words, keys=keys, item_roots=[roots[0]] * B)
    if c["search"] in WEIGHTED:
        d.update(item_weights=[WC.SumWeights([WC.BonusWeights(c["bonus"])])] * B, scale=float(c["scale"]), bonus=float(c["bonus"]))
        # the fused score's own float32 bound (weighted_pattern_cases.weight_bound), W <= L * (|lsm| + scale * bonus) < 8 L
        d["margin"] = MARGIN + WC.weight_bound(L, 8.0 * L)
    return d


def _restate(d, dtype, step=None, state0=None):
    return restate(step or d["step"], d["state0"] if state0 is None else state0, d["B"], d["k"], d["C"], d["L"], d["eos"], dtype,
                   d["keys"], d["item_roots"], d["item_weights"], d["scale"], d["merge"])


def existing_replay(d, step=None, state0=None):
    """the float64 replay of the case's search from the neighbouring case modules: the reference of every comparison.
    step / state0: another decoder step (the GPU tests pass the step kernel's)"""
    step, state0 = step or d["step"], d["state0"] if state0 is None else state0
    a = (step, state0, d["B"], d["k"], d["C"], d["L"], d["eos"])
    if d["search"] == "plain":
        return BC.replay_with(*a)
    if d["search"] in ("lexicon", "dfa"):
        return LC.replay_with(*a, d["keys"], d["item_roots"])
    if d["search"] == "wdfa":
        return WC.replay_with(*a, d["keys"], d["item_roots"], d["item_weights"], d["scale"])
    return MC.replay_with(*a, d["keys"], d["item_roots"], d["item_weights"], d["scale"])


def check_inputs(d):
    """`condition` of a case's inputs -> (counts, the float64 restatement)"""
    r64, r32 = _restate(d, torch.float64), _restate(d, torch.float32)
    return condition(r64, r32, d["margin"]), r64


def find_seed(name):
    """the first of SEEDS whose inputs meet `condition` with at least one decisive finite tie"""
    for seed in SEEDS:
        try:
            count, _ = check_inputs(case_inputs(name, seed))
        except AssertionError:
            continue
        if count["decisive"] >= 1:
            return seed
    raise AssertionError(f"{name}: no seed of {list(SEEDS)} meets the condition with a decisive tie")


def case_data(name):
    """case_inputs + f64 (the existing float64 replay), r64 (the float64 restatement) and count (`condition`'s counts; it has
    raised if the case does not meet the condition).  Built once and shared; nothing in it is changed afterwards."""
    if name not in _DATA:
        d = case_inputs(name)
        d["count"], d["r64"] = check_inputs(d)
        d["f64"] = existing_replay(d)
        _DATA[name] = d
    return _DATA[name]


def model_scores_of(f64):
    """the model scores of an existing replay's result (the unweighted searches have one score)"""
    return f64.get("model_scores", f64["scores"])
