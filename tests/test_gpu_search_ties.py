"""GPU: the six decoder searches (glass_beam_search, _lexicon, _dfa, _wdfa, _merged_dfa, _merged_wdfa) on inputs whose
candidates tie EXACTLY (tests/search_tie_cases.py), where only the stated rule - score, then flat index beam*C + class; the
back-tracking by value, then slot; completed entries by score, then t*k + slot - decides what survives; and with a non-finite
feature in a neighbouring item.  The neighbouring suites keep every selection MARGIN away from a tie; a kernel that took the
higher index on a tie - inside a thread's beams, across lanes, across the four waves, in a later round - passes them all."""
import math

import numpy as np
import pytest
import torch

import beam_cases as BC
import lexicon_beam_cases as LC
import recognition_edge_cases as E
import search_tie_cases as S
import test_gpu_beam_search as G
import test_gpu_pattern_beam as GP
import weighted_pattern_cases as WC

pytestmark = pytest.mark.gpu

MARGIN, TOL = G.MARGIN, G.TOL
assert (MARGIN, TOL) == (S.MARGIN, S.TOL)
FIELDS = ("symbols", "scores", "lengths", "path_probs", "words", "model_scores")
_bits = GP._bits


def _same_bits(a, b, what, fields=FIELDS, rows=None):
    """fields of two results (BeamResult or dict of CPU tensors) bit for bit; rows: (rows of a, rows of b) to compare"""
    get = lambda r, n: r.get(n) if isinstance(r, dict) else getattr(r, n, None)
    for n in fields:
        u, v = get(a, n), get(b, n)
        assert (u is None) == (v is None), (what, n)
        if u is not None:
            u, v = _bits(u), _bits(v)
            if rows is not None:
                u, v = u[rows[0]], v[rows[1]]
            assert u.dtype == v.dtype and torch.equal(u, v), (what, n)


def _constraint(d):
    """the product's constraint of a case -> the keyword arguments of ASTER_V2.beam_decode"""
    from glass_amd.evaluation.lexicon import LexiconTrie
    from glass_amd.evaluation.pattern import DecodePattern
    if d["search"] == "plain":
        return {}
    a = (d["characters"], d["L"], d["eos"])
    if d["regex"] is not None:
        return dict(pattern=DecodePattern(d["regex"], *a, case_insensitive=d["ci"], device=G._dev()))
    trie = LexiconTrie(d["lexicon"], *a, case_insensitive=d["ci"], device=G._dev())
    if d["search"] == "lexicon":
        return dict(lexicon=trie)
    pat = DecodePattern.from_trie(trie)
    kw = dict(merge_case=True) if d["merge"] else {}
    if d["search"] in S.WEIGHTED:
        return dict(pattern=pat.weighted(length_bonus=d["bonus"]), weight_scale=d["scale"], **kw)
    return dict(pattern=pat, **kw)


def _kernel_step(dec, x, k, C):
    """the decoder step of the replays from the existing kernel on inflated inputs -> (step, state0)"""
    from glass_amd.ops import native as K
    B, T, D = x.shape
    xproj = K.linear(x.view(B * T, D), dec.w["xW"], dec.w["xB"]).view(B, T, D)
    xi = x.unsqueeze(1).expand(B, k, T, D).reshape(B * k, T, D).contiguous()
    xpi = xproj.unsqueeze(1).expand(B, k, T, D).reshape(B * k, T, D).contiguous()

    def step(state, y_prev):
        logits, _, state = K.attention_decode_step(xi, xpi, dec.w, state, y_prev.to(torch.int32).to(x.device), C)
        return logits, state
    return step, torch.zeros((B * k, D), dtype=torch.float32, device=x.device)


_RUNS = {}


def _run(name):
    """everything the tests of one case share, computed once: decoder, constraint, the device search"""
    if name not in _RUNS:
        d = S.case_data(name)                                       # raises if the inputs do not meet the condition
        dec = G._decoder(d["sd"], d["C"], d["L"])
        x = d["x"].to(G._dev())
        kw = _constraint(d)
        got = dec.beam_decode(x, d["k"], d["eos"], path_probs=True, **kw)
        _RUNS[name] = dict(d=d, dec=dec, x=x, kw=kw, got=got,
                           cpu={n: getattr(got, n).cpu() for n in FIELDS if getattr(got, n, None) is not None})
    return _RUNS[name]


def _against(name, d, got, ref, weighted):
    """all k hypotheses of every item against a replay's result -> (largest |d model score|, |d fused score|, |d path row|)"""
    B, k, L, C = d["B"], d["k"], d["L"], d["C"]
    assert got["symbols"].shape == (B, k, L) and got["scores"].shape == got["lengths"].shape == (B, k)
    assert torch.equal(got["symbols"].long(), ref["symbols"]), name
    assert torch.equal(got["lengths"].long(), ref["lengths"]), name
    fin = torch.isfinite(ref["scores"])
    model, ref_model = got.get("model_scores", got["scores"]), S.model_scores_of(ref)
    for t in (got["scores"], model):
        assert torch.equal(torch.isneginf(t), torch.isneginf(ref["scores"])) and not torch.isnan(t).any(), name
        assert not (t == math.inf).any()
    if d["search"] != "plain":
        assert got["words"].dtype == torch.int32
        want = torch.where(fin, 0, -1) if d["regex"] is not None else ref["words"]
        assert torch.equal(got["words"].long(), want), name
    dm = G._absdiff(model, ref_model)
    df = np.where(fin.numpy(), np.abs(got["scores"].double().numpy() - np.where(fin.numpy(), ref["scores"].numpy(), 0.0)), 0.0)
    bound = TOL + (WC.weight_bound(L, 1.0) * np.maximum(1.0, ref["W"].numpy()) if weighted else 0.0)
    assert dm < TOL, (name, dm)
    assert (df <= bound).all(), (name, float(df.max()))
    dp = 0.0
    for b in range(B):
        want = BC.path_rows(ref["symbols"][b, 0], ref["step_scores"][b, 0], ref["lengths"][b, 0], ref_model[b, 0], C)
        rows = got["path_probs"][b].double().numpy()
        assert ((rows != 0) == (want != 0)).all(), (name, b)
        dp = max(dp, float(np.abs(rows - want).max()))
    assert dp < TOL, (name, dp)
    # two final scores that are exactly equal in the replay are bit-equal on the device
    eq = (ref["scores"][:, :, None] == ref["scores"][:, None, :]) & fin[:, :, None]
    for n, t in (("scores", got["scores"]), ("model_scores", model)):
        bits = t.contiguous().view(torch.int32)
        assert ((bits[:, :, None] == bits[:, None, :]) | ~eq).all(), (name, n, "tied hypotheses differ in bits")
    return dm, float(df.max()), dp


@pytest.mark.parametrize("name", list(S.CASES))
def test_tie_cases_against_the_replays(name):
    """Every item, all k hypotheses: symbols, lengths, words / tags and the finite / -inf pattern EQUAL to the existing float64
    replay of the case's search and to the same replay driven by `K.attention_decode_step` (merged: its merge in float32);
    scores, model scores and path rows within TOL = 1e-4 (fused scores: plus the float32 bound of weighted_pattern_cases);
    hypotheses whose replay scores are exactly equal have bit-equal device scores.  The inputs' condition (every deciding pair
    exactly tied in float64 and float32, or more than MARGIN apart; a decisive tie present) is asserted first.
    Measured on an MI355X, largest |d model score| = |d fused score| | |d path row| of the device search vs the float64 replay
    || the same vs the kernel-driven replay:
      flat_c13_k2_eos_first      5.4e-8 | 1.1e-8 || 5.4e-8 | 1.1e-8     flat_c13_k3_eos_mid        5.4e-8 | 1.1e-8 || 5.4e-8 | 1.1e-8
      flat_c13_k5_eos_low        6.6e-7 | 4.6e-8 || 6.6e-7 | 4.6e-8     flat_c13_k13               2.2e-7 | 4.2e-9 || 2.2e-7 | 4.2e-9
      flat_c97_k16_two_waves     2.1e-7 | 5.5e-9 || 2.1e-7 | 5.5e-9     flat_c97_k5_two_levels_l2  2.5e-7 | 8.8e-9 || 2.5e-7 | 8.8e-9
      flat_c97_k5_two_levels_l6  7.5e-7 | 8.8e-9 || 7.5e-7 | 8.8e-9     flat_c256_k3_four_waves    1.8e-7 | 3.5e-8 || 1.8e-7 | 3.5e-8
      flat_c13_k3_all_ended      0      | 0      || 0      | 0          flat_trie_k3               3.7e-7 | 2.0e-8 || 3.7e-7 | 2.0e-8
      flat_star_k5               5.5e-7 | 1.9e-8 || 5.5e-7 | 1.9e-8     flat_bonus_k3              3.7e-7 | 2.0e-8 || 3.7e-7 | 2.0e-8
      flat_merged_k3             5.0e-7 | 4.0e-8 || 6.0e-7 | 8.5e-8     flat_merged_bonus_k3       5.0e-7 | 4.0e-8 || 6.0e-7 | 8.5e-8
      twin_plain_k3              1.8e-5 | 1.9e-6 || 3.0e-7 | 1.9e-7     twin_plain_k5              4.0e-6 | 2.2e-7 || 7.5e-7 | 1.0e-8
      twin_trie_k3               6.1e-6 | 2.3e-7 || 1.4e-6 | 1.7e-7     twin_star_k5               8.2e-6 | 3.8e-7 || 1.5e-6 | 3.3e-8
      twin_bonus_k3              6.1e-6 | 2.3e-7 || 1.4e-6 | 1.7e-7
    Every case passed with the kernels as they were: no search deviates from the stated rule on a tie."""
    r = _run(name)
    d, got = r["d"], r["cpu"]
    n = d["count"]
    assert n["decisive"] >= 1 or ("only" in S.CASES[name] and n["decisive_ninf"] >= 1), "no decisive tie: replace the case"
    weighted = d["search"] in S.WEIGHTED
    assert ("model_scores" in got) == weighted
    dm, df, dp = _against(name, d, got, d["f64"], weighted)
    step, state0 = _kernel_step(r["dec"], r["x"], d["k"], d["C"])
    if d["merge"]:
        import merged_beam_cases as MC
        drv = MC.replay_with(step, state0, d["B"], d["k"], d["C"], d["L"], d["eos"], d["keys"], d["item_roots"], d["item_weights"],
                             d["scale"], merge_dtype=torch.float32)
    else:
        drv = S.existing_replay(d, step, state0)
    km, kf, kp = _against(name + " (kernel-driven)", d, got, drv, weighted)
    print(f"[ties] {name}: {n['ties']} ties, {n['decisive']} decisive, {n['decisive_ninf']} -inf cuts, {n['final_ties']} final ties; "
          f"device vs float64 replay: model {dm:.3e}, fused {df:.3e}, path {dp:.3e}; vs kernel-driven replay: model {km:.3e}, "
          f"fused {kf:.3e}, path {kp:.3e}")


@pytest.mark.parametrize("name", list(S.CASES))
def test_two_runs_and_an_item_alone_are_bit_identical(name):
    """a second run gives the same bits; item 1 alone gives the bits it has in the batch of three"""
    r = _run(name)
    d = r["d"]
    again = r["dec"].beam_decode(r["x"], d["k"], d["eos"], path_probs=True, **r["kw"])
    _same_bits(again, r["got"], (name, "second run"))
    alone = r["dec"].beam_decode(r["x"][1:2].contiguous(), d["k"], d["eos"], path_probs=True, **r["kw"])
    _same_bits(alone, r["got"], (name, "alone"), rows=(slice(0, 1), slice(1, 2)))


def test_the_native_entry_point_gives_the_same_bits():
    """`K.beam_search` on the four-wave case: what `ASTER_V2.beam_decode` returned, bit for bit"""
    from glass_amd.ops import native as K
    r = _run("flat_c256_k3_four_waves")
    d, dec, x = r["d"], r["dec"], r["x"]
    xproj = K.linear(x.view(-1, 256), dec.w["xW"], dec.w["xB"]).view(x.shape)
    out = K.beam_search(x, xproj, dec.w, d["k"], d["C"], d["L"], d["eos"], path_probs=True)
    for a, n in zip(out, ("symbols", "scores", "lengths", "path_probs")):
        assert torch.equal(_bits(a), _bits(r["cpu"][n])), n


@pytest.mark.parametrize("name", [n for n, c in S.CASES.items() if c["search"] in ("lexicon", "dfa")])
def test_trie_as_dfa_and_zero_weights_are_bit_equal(name):
    """on ties too: the lexicon search = the DFA search of the trie turned into an automaton = the weighted search with
    all-zero weights (whose fused scores are its model scores)"""
    from glass_amd.evaluation.pattern import DecodePattern
    r = _run(name)
    d = r["d"]
    pat = DecodePattern.from_trie(r["kw"]["lexicon"]) if d["search"] == "lexicon" else r["kw"]["pattern"]
    plain = ("symbols", "scores", "lengths", "path_probs", "words")
    if d["search"] == "lexicon":
        dfa = r["dec"].beam_decode(r["x"], d["k"], d["eos"], path_probs=True, pattern=pat)
        _same_bits(dfa, r["got"], (name, "trie as DFA"), plain)
    zero = pat.weighted()
    assert not zero.weight64.any()
    w = r["dec"].beam_decode(r["x"], d["k"], d["eos"], path_probs=True, pattern=zero, weight_scale=0.75)
    _same_bits(w, r["got"], (name, "zero weights"), ("symbols", "lengths", "path_probs", "words"))
    assert torch.equal(_bits(w.model_scores), _bits(r["cpu"]["scores"])) and torch.equal(_bits(w.scores), _bits(w.model_scores))


# ------------------------------------------------------------------ a non-finite neighbour
POISON = dict(C=97, k=5, L=6, eos=1, item=1)


def _poison_searches(dec, chars):
    """name -> f(x) -> tuple of device tensors, for the plain, lexicon, DFA, weighted DFA and merged searches and forced decoding"""
    from glass_amd.evaluation.lexicon import LexiconTrie
    from glass_amd.evaluation.pattern import DecodePattern
    k, L, eos = POISON["k"], POISON["L"], POISON["eos"]
    trie = LexiconTrie(S.TWIN_WORDS, chars, L, eos, case_insensitive=True, device=G._dev())
    pat = DecodePattern(r"[a-c]+\d?", chars, L, eos, case_insensitive=True, device=G._dev())
    wpat = DecodePattern.from_trie(trie).weighted(length_bonus=0.5)
    g = torch.Generator().manual_seed(7)
    targets = torch.randint(2, POISON["C"], (S.B, 3, L), generator=g, dtype=torch.int32).to(G._dev())
    lengths = torch.tensor([[L, 3, 1]] * S.B, dtype=torch.int32).to(G._dev())

    def beam(**kw):
        def f(x):
            r = dec.beam_decode(x, k, eos, path_probs=True, **kw)
            return {n: getattr(r, n) for n in FIELDS if getattr(r, n, None) is not None}
        return f

    def forced(x):
        r = dec.score(x, targets, lengths, eos=eos, probs=True)
        return dict(step_logp=r.step_logp, scores=r.scores, lengths=r.lengths, probs=r.probs)
    return dict(plain=beam(), lexicon=beam(lexicon=trie), dfa=beam(pattern=pat), wdfa=beam(pattern=wpat, weight_scale=0.75),
                merged=beam(pattern=pat, merge_case=True), forced=forced), len(S.TWIN_WORDS)


@pytest.mark.parametrize("poison", list(E.POISONS))
def test_a_non_finite_neighbour_changes_no_other_item(poison):
    """a NaN / +inf / 1e30 feature in item 1 of three (C = 97: wave 0's 64 candidates are then all NaN, which is where the
    top-k's "no candidate" fallback is taken): every search completes, items 0 and 2 are bit-identical to the clean call and so
    is a following clean call; of item 1 only what the kernels promise is checked - symbols in [0, C), lengths in
    [0, max_len], words -1 or a word's index, no NaN among the search scores (the tables hold numbers the back-tracking sorts).
    Before the fallback also replaced the score (rows_topk: `gb = -INFINITY`), the NaN case of the plain search returned the
    scores [nan, 0, 0, 0, nan] for item 1 on an MI355X: the NaN maximum of wave 0 went into the score table, beam_rank gave
    every NaN rank 0 and the back-tracking read result slots no lane had assigned."""
    C, k, L, eos, bad_item = (POISON[n] for n in ("C", "k", "L", "eos", "item"))
    chars = LC.shipped_characters()
    dec = G._decoder(BC.decoder_sd(C, fc_scale=1.0, eos=eos), C, L)
    x = BC.rand_x(S.B, S.T, 321)
    bad = x.clone()
    bad[bad_item, 3, 11] = E.POISONS[poison]
    x, bad = x.to(G._dev()), bad.to(G._dev())
    others = [b for b in range(S.B) if b != bad_item]
    searches, n_words = _poison_searches(dec, chars)
    for what, f in searches.items():
        clean = {n: t.cpu() for n, t in f(x).items()}
        hit = {n: t.cpu() for n, t in f(bad).items()}
        torch.cuda.synchronize()
        again = {n: t.cpu() for n, t in f(x).items()}
        for n in clean:
            assert torch.equal(_bits(hit[n])[others], _bits(clean[n])[others]), (poison, what, n, "another item changed")
            assert torch.equal(_bits(again[n]), _bits(clean[n])), (poison, what, n, "a following clean call changed")
        ln = hit["lengths"][bad_item]
        assert int(ln.min()) >= 0 and int(ln.max()) <= L, (poison, what)
        if what != "forced":
            sym = hit["symbols"][bad_item]
            assert int(sym.min()) >= 0 and int(sym.max()) < C, (poison, what)
            assert not torch.isnan(hit["scores"][bad_item]).any(), (poison, what)
        if "words" in hit:
            w = hit["words"][bad_item]
            assert int(w.min()) >= -1 and int(w.max()) < n_words, (poison, what)
