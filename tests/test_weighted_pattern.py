"""CPU: the host side of weighted-pattern decoding (evaluation/weighted_pattern.py) - the character n-gram model against a
brute-force back-off, its estimate and its ARPA reader; the weighted automata (length bonus, pushed word priors, the product
with the model's contexts) against weights computed straight from their sources (tests/weighted_pattern_cases.py); the
tables, their reproducibility and limits; the seeds and gaps of the float64 replay's cases; the per-feature header and its
binding; what the model surface refuses."""
import ctypes
import itertools
import math
import os

import numpy as np
import pytest
import torch

import lexicon_beam_cases as LC
import weighted_pattern_cases as WC

ROOT = LC.ROOT
NAMES = ["glass_beam_search_wdfa_workspace_bytes", "glass_beam_search_wdfa"]
BOS, EOS = WC.BOS, WC.EOS


def _lm():
    from glass_amd.evaluation.weighted_pattern import CharNgramLM
    return CharNgramLM.estimate(WC.AB_WORDS + ["cab", "c"], order=3, alphabet="abcd")


# ------------------------------------------------------------------ the n-gram model
def test_score_against_a_brute_force_backoff():
    lm = _lm()
    symbols = ["a", "b", "c", "d", "z", EOS]
    n = 0
    for m in range(4):
        for h in itertools.product(["a", "b", "c", "z"], repeat=m):
            for hist in (h, (BOS,) + h):
                for c in symbols:
                    want = WC.lm_score(lm.logp, lm.backoff, lm.order, lm.unk_logp, hist, c)
                    assert lm.score(hist, c) == pytest.approx(want, abs=1e-12), (hist, c)
                    n += 1
    assert lm.score(("a", "b"), "z") == pytest.approx(lm.backoff[("a", "b")] + lm.backoff[("b",)] + lm.unk_logp, abs=1e-12)
    assert lm.score(("z", "z"), "a") == lm.logp[("a",)]                        # contexts without a back-off weigh 0
    assert lm.context((BOS, "a", "b", "a")) == ("b", "a") and lm.context((BOS,)) == (BOS,)
    assert lm.word_score("ab") == pytest.approx(lm.score((BOS,), "a") + lm.score((BOS, "a"), "b") + lm.score(("a", "b"), EOS), abs=1e-12)
    print(f"[weighted] {n} scores against the brute force; {len(lm.logp)} n-grams, {len(lm.backoff)} back-offs")


@pytest.mark.parametrize("order", [1, 2, 3, 4])
def test_estimate_is_a_distribution_in_every_seen_context(order):
    from glass_amd.evaluation.weighted_pattern import CharNgramLM
    words = WC.AB_WORDS + WC.MIX_WORDS
    lm = CharNgramLM.estimate(words, order=order, discount=0.75)
    alphabet = sorted({c for w in words for c in w}) + [EOS]
    contexts = {()} | set(lm.backoff)
    for w in words:
        s = (BOS,) + tuple(w)
        contexts |= {s[max(i - m, 0):i] for i in range(1, len(s) + 1) for m in range(order)}
    assert len(contexts) > 1 or order == 1
    for h in contexts:
        assert sum(math.exp(lm.score(h, c)) for c in alphabet) == pytest.approx(1.0, abs=1e-12), h
    # the definition, on one seen and one unseen trigram
    if order == 3:
        d, n_ab = 0.75, sum(1 for w in words for i in range(len(w) - 1) if w[i:i + 2] == "ab")
        nxt = [(w + "\n")[i + 2] for w in words for i in range(len(w) - 1) if w[i:i + 2] == "ab"]
        T = len(set(nxt))
        p_low = lambda c: math.exp(lm.score(("b",), c))
        assert math.exp(lm.score(("a", "b"), "a")) == pytest.approx((nxt.count("a") - d) / n_ab + d * T / n_ab * p_low("a"), abs=1e-12)
        assert ("a", "b", "3") not in lm.logp
        assert math.exp(lm.score(("a", "b"), "3")) == pytest.approx(d * T / n_ab * p_low("3"), abs=1e-12)
    for bad in (dict(order=0), dict(discount=1.0), dict(discount=0.0), dict(alphabet="a")):
        with pytest.raises(ValueError):
            CharNgramLM.estimate(words, **bad)


ARPA = """
\\data\\
ngram 1=4
ngram 2=3

\\1-grams:
-99\t<s>\t-0.30103
-0.60206\ta\t-0.1
-0.39794\tb
-1.0\t</s>

\\2-grams:
-0.2\t<s> a
-0.5\ta b
-0.7\tb </s>

\\end\\
"""


def test_from_arpa():
    from glass_amd.evaluation.weighted_pattern import CharNgramLM
    lm = CharNgramLM.from_arpa(ARPA)
    ln10 = math.log(10.0)
    assert lm.order == 2 and len(lm.logp) == 7 and set(lm.backoff) == {(BOS,), ("a",)}
    assert lm.score((BOS,), "a") == pytest.approx(-0.2 * ln10, abs=1e-12)
    assert lm.score((BOS,), "b") == pytest.approx((-0.30103 - 0.39794) * ln10, abs=1e-12)
    assert lm.score(("a",), EOS) == pytest.approx((-0.1 - 1.0) * ln10, abs=1e-12)
    assert lm.score(("b",), "a") == pytest.approx(-0.60206 * ln10, abs=1e-12)                # no back-off stored for b: 0
    assert lm.score(("a",), "q") == pytest.approx(-0.1 * ln10 - 23.0, abs=1e-12)
    assert lm.word_score("ab") == pytest.approx((-0.2 - 0.5 - 0.7) * ln10, abs=1e-12)
    for bad in ("", "\\data\\\nngram 1=1\n\\1-grams:\n-1.0\tab\n\\end\\", "\\data\\\nngram 1=1\n\\1-grams:\n-1.0\n\\end\\"):
        with pytest.raises(ValueError):
            CharNgramLM.from_arpa(bad)


# ------------------------------------------------------------------ the automata against weights from their sources
_BUILT = {}


def _built(name):
    if name not in _BUILT:
        d = WC.case_inputs(name)
        _BUILT[name] = (d,) + WC.build_pattern(d, "cpu")
    return _BUILT[name]


@pytest.mark.parametrize("name", list(WC.CASES))
def test_weights_of_every_short_string(name):
    """every string of up to 4 characters over the case's alphabet: accepted iff the base pattern accepts it, and its weight
    (start64 + the walked weight64 + final64) is the callbacks' total; the tables are the float32 roundings"""
    d, base, wp = _built(name)
    from glass_amd.evaluation.weighted_pattern import WeightedPattern
    assert isinstance(wp, WeightedPattern) and isinstance(wp, type(base)) and wp.keys == base.keys
    alphabet = WC.alphabet_of(d)
    accepted, worst = 0, 0.0
    for key in d["segment_names"]:
        for w in WC.strings_up_to(alphabet, 4):
            got = wp.weight_of(w, key)
            assert (got is not None) == base.accepts(w, key) == wp.accepts(w, key), (name, key, w)
            assert wp.tag(w, key) == base.tag(w, key)
            if got is not None:
                want = d["weights"][key].total(w)
                worst = max(worst, abs(got - want))
                assert got == pytest.approx(want, abs=1e-12), (name, key, w)
                accepted += 1
        for w in d["words"][key][:200]:                                            # and the language itself, whatever its lengths
            assert wp.weight_of(w, key) == pytest.approx(d["weights"][key].total(w), abs=1e-12), (name, key, w)
    assert accepted > 0 or name == "l64_a63"
    print(f"[weighted] {name}: {wp.num_states} states ({base.num_states} unweighted), {accepted} accepted strings, worst |dw| {worst:.2e}, "
          f"{wp.nbytes} bytes, built in {wp.build_seconds:.3f} s")
    # ---- tables
    N, F = wp.num_states, wp.num_fold
    assert wp.trans.shape == (N, F, 2) and wp.trans.dtype == np.int32 and wp.trans.flags["C_CONTIGUOUS"]
    assert np.array_equal(wp.trans[:, :, 0], wp.next)
    assert np.array_equal(wp.trans[:, :, 1].copy().view(np.float32), wp.weight64.astype(np.float32))
    assert np.array_equal(wp.final_w, wp.final64.astype(np.float32)) and np.array_equal(wp.start_w, wp.start64.astype(np.float32))
    assert wp.weight64.dtype == wp.final64.dtype == wp.start64.dtype == np.float64
    assert np.isfinite(wp.weight64).all() and not wp.weight64[wp.next < 0].any()
    assert np.array_equal(wp.accept, base.accept[wp.base_state]) and np.array_equal(wp.dist, base.dist[wp.base_state])
    assert np.array_equal(np.where(wp.start >= 0, wp.base_state[np.maximum(wp.start, 0)], -1), base.start)
    tgt = np.where(wp.next >= 0, wp.next & 0xFFFFFF, -1)
    assert np.array_equal(np.where(tgt >= 0, wp.next >> 24, -1), np.where(tgt >= 0, np.minimum(wp.dist[np.maximum(tgt, 0)], 127), -1))
    assert np.array_equal(np.where(tgt >= 0, wp.base_state[np.maximum(tgt, 0)], -1), np.where(base.next >= 0, base.next & 0xFFFFFF, -1)[wp.base_state])
    if d["lm"] is None:
        assert N == base.num_states and np.array_equal(wp.next, base.next)
    else:
        # breadth-first from the starts in segment order, fold symbols ascending: first visits are numbered in that order
        seen = head = 0
        for s in wp.start:
            if s >= seen:
                assert s == seen
                seen += 1
            while head < seen:
                for t in tgt[head][tgt[head] >= 0]:
                    if t >= seen:
                        assert t == seen, (name, head, t)
                        seen += 1
                head += 1
        assert seen == N
        assert len(set(zip(wp.base_state.tolist(), wp.contexts))) == N
    for n, t in wp.tensors.items():
        if n != "F":
            assert np.array_equal(t.numpy(), getattr(wp, n)), n
    # ---- two builds give identical arrays
    again = WC.build_pattern(d, "cpu")[1]
    for n in ("trans", "final_w", "start_w", "accept", "start", "fold", "weight64", "final64", "start64", "base_state"):
        assert np.array_equal(getattr(again, n), getattr(wp, n)), n


@pytest.mark.parametrize("name", ["priors_reverse_k3", "priors_twins_ci_k4", "two_segments_start_w"])
def test_priors_are_pushed_toward_the_root(name):
    """without the other sources: every prefix carries the best prior below it, a full word exactly its prior (the best of
    the words that end there), and start_w differs between the segments"""
    d, base, _ = _built(name)
    wp = base.weighted(word_logprior=d["priors"])
    priors = d["priors"] if isinstance(d["priors"], dict) else {None: d["priors"]}
    for key in d["segment_names"]:
        words, pri = d["words"][key], priors[key]
        for w in words:
            for n in range(len(w) + 1):
                q, total = int(wp.start[wp.segment(key)]), float(wp.start64[wp.segment(key)])
                for ch in w[:n]:
                    f = wp._sym_id[ch]
                    total += float(wp.weight64[q, f])
                    q = int(wp.next[q, f]) & 0xFFFFFF
                assert total == pytest.approx(max(p for v, p in zip(words, pri) if v.startswith(w[:n])), abs=1e-12), (key, w, n)
            assert wp.weight_of(w, key) == pytest.approx(max(p for v, p in zip(words, pri) if v == w), abs=1e-12), (key, w)
    if name == "priors_twins_ci_k4":
        assert wp.weight_of("ab") == wp.weight_of("AB") == pytest.approx(-0.25, abs=1e-12)           # three words at one node
    if name == "two_segments_start_w":
        assert wp.start64.tolist() == [-0.1, -0.5]
    assert wp.num_states == base.num_states


def test_a_trie_crossed_with_a_model_keeps_its_states():
    d, base, _ = _built("priors_reverse_k3")
    from glass_amd.evaluation.weighted_pattern import CharNgramLM
    lm = CharNgramLM.estimate(["ab", "abc", "cab", "0"], order=3)
    wp = base.weighted(lm=lm, word_logprior=d["priors"], length_bonus=0.5)
    assert wp.num_states == base.num_states and sorted(wp.base_state.tolist()) == list(range(base.num_states))
    for w, p in zip(d["words"]["p"], d["priors"]["p"]):
        assert wp.weight_of(w, "p") == pytest.approx(lm.word_score(w) + 0.5 * len(w) + p, abs=1e-12)    # the three sources add
        assert wp.tag(w, "p") == base.tag(w, "p")


def test_every_bad_argument_raises():
    from glass_amd.evaluation.lexicon import LexiconTrie
    from glass_amd.evaluation.pattern import DecodePattern
    regex = DecodePattern(r"[ab]+", WC.C13, 5, 1, device="cpu")
    trie = DecodePattern.from_trie(LexiconTrie(WC.LEX, WC.C13, 5, 1, case_insensitive=False, device="cpu"))
    for bonus in (math.inf, -math.inf, math.nan):
        with pytest.raises(ValueError, match="length_bonus"):
            regex.weighted(length_bonus=bonus)
    with pytest.raises(ValueError, match="not finite"):
        regex.weighted(length_bonus=1e39)                                        # finite in float64, not in float32
    with pytest.raises(ValueError, match="from_trie"):
        regex.weighted(word_logprior=[0.0])
    with pytest.raises(ValueError, match="entries"):
        trie.weighted(word_logprior=[0.0] * 10)
    with pytest.raises(ValueError, match="entries"):
        trie.weighted(word_logprior={"p": [0.0] * 7, "q": [0.0] * 3})
    with pytest.raises(ValueError, match="keys"):
        trie.weighted(word_logprior={"p": [0.0] * 7})
    with pytest.raises(ValueError, match="keys"):
        trie.weighted(word_logprior={"p": [0.0] * 7, "z": [0.0] * 4})
    for bad in (math.nan, math.inf, -math.inf):
        with pytest.raises(ValueError, match="not finite"):
            trie.weighted(word_logprior=[0.0] * 10 + [bad])
    with pytest.raises(ValueError, match="CharNgramLM"):
        regex.weighted(lm={"a": 0.0})
    with pytest.raises(ValueError, match="table limit"):
        regex.weighted(length_bonus=1.0, table_cap_bytes=regex.num_states * regex.num_fold * 8 - 1)
    regex.weighted(length_bonus=1.0, table_cap_bytes=regex.num_states * regex.num_fold * 8)       # the cap is on the 8-byte entries
    with pytest.raises(ValueError, match="states"):
        regex.weighted(lm=_lm(), table_cap_bytes=3 * regex.num_fold * 8)
    with pytest.raises(ValueError, match="weighted already"):
        regex.weighted(length_bonus=1.0).weighted(length_bonus=1.0)
    # a word the trie left out is ignored, whatever its prior
    lex = LexiconTrie(["ab", "", "abcdefgh", "b"], WC.C13, 5, 1, case_insensitive=False, device="cpu")
    assert lex.word_node.tolist()[1:3] == [-1, -1] and lex.segment_sizes == [4]
    wp = DecodePattern.from_trie(lex).weighted(word_logprior=[-1.0, math.nan, math.inf, -2.0])
    assert wp.weight_of("ab") == -1.0 and wp.weight_of("b") == -2.0 and wp.start64.tolist() == [-1.0]
    # zero weights: a weighted pattern of the same automaton
    z = regex.weighted()
    assert not z.weight64.any() and not z.final64.any() and not z.start64.any() and np.array_equal(z.next, regex.next)


# ------------------------------------------------------------------ the replay's cases: seeds, gaps, properties
@pytest.mark.parametrize("name", list(WC.CASES))
def test_case_seeds_and_gaps(name):
    """the seed is the first of 100.. for which every item's fused gaps exceed MARGIN + the weight bound and the case has the
    property it is named for - conditions on the float64 replay alone"""
    d = WC.case_data(name)
    f, k, L = d["f64"], d["k"], d["L"]

    def has_property(dd, ff):
        if name == WC.REVERSING:
            u = WC.unweighted_replay(dd)                 # (the GPU test compares the unweighted search with it: no near-tie there either)
            if not min(float(u["sel_gap"].min()), float(u["done_gap"].min())) > WC.MARGIN:
                return False
            return any(not torch.equal(u["symbols"][b, 0], ff["symbols"][b, 0]) for b in range(dd["B"]))
        if name == WC.LONGEST:
            return bool((ff["lengths"][:, 0] == L).all())
        return True
    fin = torch.isfinite(f["scores"])
    W = float(f["W"][fin].max()) if fin.any() else 0.0
    print(f"[weighted] {name}: seed {WC.CASES[name]['seed']}, smallest selection gap {float(f['sel_gap'].min()):.3e}, completion gap "
          f"{float(f['done_gap'].min()):.3e}, W {W:.2f}, weight bound {WC.weight_bound(L, W):.2e}, completed {f['completed'].tolist()[:6]}")
    assert WC.gaps_clear(d, f), "a near-tie: choose another seed for this case, do not relax the margin"
    assert has_property(d, f)
    for seed in range(100, WC.CASES[name]["seed"]):
        dd = WC.case_inputs(name, seed)
        ff = WC.replay(dd["sd"], dd["x"], dd["k"], dd["C"], dd["L"], dd["eos"], dd["keys"], dd["item_roots"], dd["item_weights"], dd["scale"])
        assert not (WC.gaps_clear(dd, ff) and has_property(dd, ff)), f"seed {seed} comes first"
    # every hypothesis is a word of the language, its fused score the model's plus scale * its weight
    for b, key in enumerate(d["item_keys"]):
        for i in range(k):
            if fin[b, i]:
                w = "".join(d["keys"][int(s)] for s in f["symbols"][b, i, :int(f["lengths"][b, i]) - 1])
                assert w in d["words"][key]
                want = float(f["model_scores"][b, i]) + d["scale"] * d["weights"][key].total(w)
                assert float(f["scores"][b, i]) == pytest.approx(want, abs=1e-9)
    if name == "k1_lm_c13_l4":
        assert k == 1
    if name == "two_segments_start_w":
        assert not fin[2].any() and not fin[3].any() and fin[[0, 1, 4]].all() and WC.item_segments(d) == [0, 1, -1, 2, 1]
        assert d["weights"]["p"].start() != d["weights"]["q"].start()
    if name == "l64_a63":
        assert (f["lengths"][:, 0] == 64).all()
    if name in WC.EXHAUSTIVE:
        assert len(d["words"][None]) <= k and all(len(w) < L - 1 for w in d["words"][None])
        assert (fin.sum(1) == len(d["words"][None])).all()
    if name == "priors_twins_ci_k4":
        assert d["words"][None].count("AB") == 3


# ------------------------------------------------------------------ the header and the model surface
def test_feature_header_and_binding():
    from glass_amd import _lib
    with open(os.path.join(ROOT, "include", "glass_hip_feature_wdfa.h")) as fh:
        text = fh.read()
    assert '#include "glass_hip.h"' in text
    assert list(_lib.signatures(text)) == NAMES
    for name in NAMES:
        assert _lib.FEATURE_EXPORTS.count(name) == 1 and name not in _lib.EXPORTS + _lib.EXT_EXPORTS + _lib.ADDON_EXPORTS, name
    for other in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if other != "glass_hip_feature_wdfa.h":
            with open(os.path.join(ROOT, "include", other)) as fh:
                assert "glass_beam_search_wdfa" not in fh.read(), other
    _lib.build_library()
    L = _lib.lib()
    p, i, l, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float
    assert L.glass_beam_search_wdfa_workspace_bytes.restype is l and L.glass_beam_search_wdfa_workspace_bytes.argtypes == [i] * 6
    assert L.glass_beam_search_wdfa.restype is i
    assert L.glass_beam_search_wdfa.argtypes == [p, p, p] + [i] * 7 + [p] * 6 + [i] * 3 + [p, f] + [p] * 6 + [p, l, p]
    assert L.glass_abi_version() == _lib.ABI_VERSION == 8
    B, k, Lm = 3, 5, 26
    assert (L.glass_beam_search_wdfa_workspace_bytes(B, k, 32, 256, 97, Lm)
            == L.glass_beam_search_dfa_workspace_bytes(B, k, 32, 256, 97, Lm) + 2 * B * Lm * k * 4)
    assert L.glass_beam_search_wdfa_workspace_bytes(0, k, 32, 256, 97, Lm) == 0


def test_every_bad_argument_is_refused_on_the_host():
    """no device needed: every refusal comes before the first runtime call; the pointers are never dereferenced"""
    from glass_amd import _lib
    _lib.build_library()
    L = _lib.lib()
    ptr = 4096

    def call(B=2, k=3, T=8, D=256, C=13, max_len=5, N=4, S=1, F=11, scale=1.0, **null):
        a = {n: (None if null.get(n) else ptr) for n in ("x", "trans", "final_w", "start_w", "accept", "start", "fold", "item", "model",
                                                         "tags", "ws")}
        return L.glass_beam_search_wdfa(a["x"], ptr, ptr, B, k, T, D, C, max_len, 1, a["trans"], a["final_w"], a["start_w"], a["accept"],
                                        a["start"], a["fold"], N, S, F, a["item"], scale, ptr, ptr, a["model"], ptr, a["tags"], None,
                                        a["ws"], 1 << 40, None)
    for kw, what in ((dict(k=17), "k=17"), (dict(k=14), "k=14"), (dict(max_len=65), "max_len=65"), (dict(T=65), "T=65"),
                     (dict(D=128), "D=128"), (dict(C=257), "C=257"), (dict(N=0), "N=0"), (dict(N=1 << 24), "N=16777216"),
                     (dict(S=0), "S=0"), (dict(F=0), "F=0"), (dict(F=257), "F=257"), (dict(scale=math.inf), "weight_scale"),
                     (dict(scale=math.nan), "weight_scale"), (dict(x=True), "null"), (dict(trans=True), "null"),
                     (dict(final_w=True), "null"), (dict(start_w=True), "null"), (dict(accept=True), "null"), (dict(start=True), "null"),
                     (dict(fold=True), "null"), (dict(item=True), "null"), (dict(model=True), "null"), (dict(tags=True), "null"),
                     (dict(ws=True), "null")):
        assert call(**kw) < 0, kw
        assert what in L.glass_last_error().decode(), (kw, L.glass_last_error().decode())
    assert L.glass_beam_search_wdfa(ptr, ptr, ptr, 2, 3, 8, 256, 13, 5, 1, 4100, ptr, ptr, ptr, ptr, ptr, 4, 1, 11, ptr, 1.0, ptr, ptr, ptr,
                                    ptr, ptr, None, ptr, 1 << 40, None) < 0 and "8-byte aligned" in L.glass_last_error().decode()
    assert L.glass_beam_search_wdfa(ptr, ptr, ptr, 2, 3, 8, 256, 13, 5, 1, ptr, ptr, ptr, ptr, ptr, ptr, 4, 1, 11, ptr, 1.0, ptr, ptr, ptr,
                                    ptr, ptr, None, ptr, 16, None) < 0 and "workspace too small" in L.glass_last_error().decode()
    assert call(B=0) == 0                                                       # nothing to do, nothing launched


def _cfg(opts=()):
    from glass_amd.config import get_glass_cfg
    return get_glass_cfg(os.path.join(ROOT, "configs", "glass_icdar15_mi355x.yaml"), ["MODEL.DEVICE", "cpu"] + list(opts))


def test_host_surface():
    from glass_amd.evaluation.lexicon import LexiconTrie
    from glass_amd.evaluation.pattern import DecodePattern
    from glass_amd.modeling.recognition.recognizer_decoder import ASTER_V2, BeamResult
    from glass_amd.modeling.recognition.recognizer_head_v2 import RecognizerRCNNHeadV3
    from glass_amd.structures.core import ShapeSpec
    chars = LC.shipped_characters()
    wp = DecodePattern(r"\d+", chars, 26, 1, device="cpu").weighted(length_bonus=0.5)
    trie = LexiconTrie(["car"], chars, 26, 1, device="cpu")
    dec = ASTER_V2(_cfg(), ShapeSpec(channels=256))
    x = torch.zeros((2, 8, 256))
    with pytest.raises(ValueError, match="lexicon and pattern"):
        dec.beam_decode(x, 3, 1, lexicon=trie, pattern=wp)
    with pytest.raises(ValueError, match="max_len"):
        dec.beam_decode(x, 3, 1, pattern=DecodePattern(r"\d+", chars, 25, 1, device="cpu").weighted(length_bonus=0.5))
    r = BeamResult(1, 2, 3)
    assert r.model_scores is None and tuple(r) == (1, 2, 3, None)
    assert BeamResult(1, 2, 3, model_scores=4).model_scores == 4
    assert _cfg().MODEL.ROI_RECOGNIZER_HEAD.DECODE_LENGTH_BONUS == 0.0
    with pytest.raises(ValueError, match="DECODE_PATTERN"):
        RecognizerRCNNHeadV3(_cfg(["MODEL.ROI_RECOGNIZER_HEAD.BEAM_WIDTH", 3, "MODEL.ROI_RECOGNIZER_HEAD.DECODE_LENGTH_BONUS", 0.5]),
                             ShapeSpec(channels=256))
    plain = RecognizerRCNNHeadV3(_cfg(["MODEL.ROI_RECOGNIZER_HEAD.BEAM_WIDTH", 3, "MODEL.ROI_RECOGNIZER_HEAD.DECODE_PATTERN", r"\d+"]),
                                 ShapeSpec(channels=256))
    assert type(plain.pattern) is DecodePattern and plain.weight_scale == 1.0                    # the default: nothing changes
    built = RecognizerRCNNHeadV3(_cfg(["MODEL.ROI_RECOGNIZER_HEAD.BEAM_WIDTH", 3, "MODEL.ROI_RECOGNIZER_HEAD.DECODE_PATTERN", r"\d+",
                                       "MODEL.ROI_RECOGNIZER_HEAD.DECODE_LENGTH_BONUS", 0.5]), ShapeSpec(channels=256))
    assert type(built.pattern).__name__ == "WeightedPattern" and built.pattern.weight_of("123") == 1.5
    head = RecognizerRCNNHeadV3(_cfg(["MODEL.ROI_RECOGNIZER_HEAD.BEAM_WIDTH", 3]), ShapeSpec(channels=256))
    head.set_pattern(wp, weight_scale=0.7)
    assert head.pattern is wp and head.weight_scale == 0.7
    head.set_pattern(None)
    assert head.pattern is None and head.weight_scale == 1.0
