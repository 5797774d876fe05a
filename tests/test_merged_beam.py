"""CPU: the host side of the fold-merged constrained beam searches - DecodePattern.fold_groups, the validation of hand-made
groups, every refusal of the surface, the feature header and its binding, the config key - and the float64 replay's cases
(tests/merged_beam_cases.py): their seeds and margins, the invariant, what each case is named for."""
import ctypes
import os

import numpy as np
import pytest
import torch

import lexicon_beam_cases as LC
import merged_beam_cases as MC

ROOT = LC.ROOT
NAMES = ["glass_beam_search_merged_dfa_workspace_bytes", "glass_beam_search_merged_dfa",
         "glass_beam_search_merged_wdfa_workspace_bytes", "glass_beam_search_merged_wdfa"]


def _cfg(opts=()):
    from glass_amd.config import get_glass_cfg
    return get_glass_cfg(os.path.join(ROOT, "configs", "glass_icdar15_mi355x.yaml"), ["MODEL.DEVICE", "cpu"] + list(opts))


# ------------------------------------------------------------------ fold_groups
def _brute_force_groups(fold, F):
    return [[c for c in range(len(fold)) if fold[c] == f] for f in range(F)]


@pytest.mark.parametrize("ci", [True, False])
def test_fold_groups_against_a_brute_force_grouping(ci):
    from glass_amd.evaluation.lexicon import LexiconTrie
    from glass_amd.evaluation.pattern import DecodePattern
    chars = LC.shipped_characters()
    eos = chars.index("[s]")
    p = DecodePattern(r"[a-z]+\d?", chars, 26, eos, case_insensitive=ci, device="cpu")
    gs, gc = p.fold_groups()
    want = _brute_force_groups(p.fold.tolist(), p.num_fold)
    assert gs.dtype == gc.dtype == np.int32 and gs.shape == (p.num_fold + 1,) and gs[0] == 0 and gs[-1] == len(gc)
    assert [gc[gs[f]:gs[f + 1]].tolist() for f in range(p.num_fold)] == want
    sizes = sorted({len(g) for g in want})
    assert sizes == ([1, 2] if ci else [1]) and (sum(len(g) == 2 for g in want) == 26) == ci
    in_groups = set(gc.tolist())
    assert eos not in in_groups and chars.index("[GO]") not in in_groups and len(in_groups) == len(gc) == 95
    for f, g in enumerate(want):                                  # a group is the casings of one character
        assert len({chars[c].upper() if ci else chars[c] for c in g}) == 1
    # deterministic, carried by `tensors`, inherited by the weighted pattern and by from_trie
    again = p.fold_groups()
    assert np.array_equal(again[0], gs) and np.array_equal(again[1], gc)
    assert np.array_equal(p.tensors["group_start"].numpy(), gs) and np.array_equal(p.tensors["group_cls"].numpy(), gc)
    assert p.tensors["group_start"].dtype == torch.int32
    wp = p.weighted(length_bonus=0.5)
    assert np.array_equal(wp.fold_groups()[1], gc) and np.array_equal(wp.tensors["group_cls"].numpy(), gc)
    assert np.array_equal(wp.tensors["group_start"].numpy(), gs)
    t = DecodePattern.from_trie(LexiconTrie(["car", "Card"], chars, 26, eos, case_insensitive=ci, device="cpu"))
    assert np.array_equal(t.fold_groups()[0], gs) and np.array_equal(t.tensors["group_cls"].numpy(), gc)
    # what the pattern pins about itself did not move
    assert p.nbytes == p.next.nbytes + p.accept.nbytes + p.start.nbytes + p.fold.nbytes


def test_hand_made_groups_are_validated():
    from glass_amd.ops.native import check_fold_groups
    t = MC.hand_inputs()["tables"]
    fold, gs, gc, C, F = t["fold"], t["group_start"], t["group_cls"], 13, t["F"]
    check_fold_groups(fold, gs, gc, C, F, 0)
    assert [gc[gs[f]:gs[f + 1]].tolist() for f in range(F)] == [[1, 5, 12], [2, 3, 7, 9], [4], [6], [8, 10]]

    def bad(match, fold=fold, gs=gs, gc=gc, C=C, F=F, eos=0):
        with pytest.raises(ValueError, match=match):
            check_fold_groups(np.asarray(fold), np.asarray(gs), np.asarray(gc), C, F, eos)
    bad("F \\+ 1", gs=gs[:-1])
    bad("rise from 0", gs=[1] + gs[1:].tolist())
    bad("rise from 0", gs=[0, 3, 2, 8, 9, 11])
    bad("rise from 0", gs=gs.tolist()[:-1] + [10])
    bad("outside", gc=[1, 5, 13] + gc[3:].tolist())
    bad("outside", gc=[-1] + gc[1:].tolist())
    bad("more than one group", gc=[1, 5, 12, 2, 3, 7, 9, 4, 6, 8, 8])
    bad("equal within a group", gc=[1, 5, 11] + gc[3:].tolist())
    bad("equal within a group", fold=[-1, 0, 1, 1, 2, 3, 3, 1, 4, 1, 4, -1, 0])
    bad("stop class", eos=5)
    bad("ascending", gc=[5, 1, 12] + gc[3:].tolist())
    bad("1..C", gc=np.zeros(0, dtype=np.int32), gs=np.zeros(F + 1, dtype=np.int32))
    bad("classes", C=12)
    bad("integer", gc=gc.astype(np.float32))


# ------------------------------------------------------------------ the header and the binding
def test_feature_header_and_binding():
    from glass_amd import _lib
    with open(os.path.join(ROOT, "include", "glass_hip_feature_merged.h")) as fh:
        text = fh.read()
    assert list(_lib.signatures(text)) == NAMES
    for name in NAMES:
        assert _lib.FEATURE_EXPORTS.count(name) == 1 and name not in _lib.EXPORTS + _lib.EXT_EXPORTS + _lib.ADDON_EXPORTS, name
    for other in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if other != "glass_hip_feature_merged.h":
            with open(os.path.join(ROOT, "include", other)) as fh:
                assert "glass_beam_search_merged" not in fh.read(), other
    assert "glass_hip_feature_merged.h" in [os.path.basename(p) for p in _lib.feature_headers()]
    for word in ("Invariant", "Approximation", "REPRESENTATIVE", "ascending class order", "never merged"):
        assert word in text, word                                   # the contract is stated where the entry points are declared
    _lib.build_library()
    L = _lib.lib()
    p, i, l, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float
    assert L.glass_beam_search_merged_dfa.restype is i and L.glass_beam_search_merged_wdfa.restype is i
    assert L.glass_beam_search_merged_dfa.argtypes == [p, p, p] + [i] * 7 + [p] * 4 + [i] * 3 + [p, p, p, i] + [p] * 5 + [p, l, p]
    assert L.glass_beam_search_merged_wdfa.argtypes == ([p, p, p] + [i] * 7 + [p] * 6 + [i] * 3 + [p, f] + [p, p, i] + [p] * 6 +
                                                        [p, l, p])
    assert L.glass_abi_version() == _lib.ABI_VERSION == 8
    for B, k, Lm in ((3, 5, 26), (1, 16, 64), (0, 5, 26)):
        assert (L.glass_beam_search_merged_dfa_workspace_bytes(B, k, 32, 256, 97, Lm)
                == L.glass_beam_search_dfa_workspace_bytes(B, k, 32, 256, 97, Lm))
        assert (L.glass_beam_search_merged_wdfa_workspace_bytes(B, k, 32, 256, 97, Lm)
                == L.glass_beam_search_wdfa_workspace_bytes(B, k, 32, 256, 97, Lm))


def test_every_bad_argument_is_refused_on_the_host():
    """no device needed: every refusal comes before the first runtime call; the pointers are never dereferenced"""
    from glass_amd import _lib
    _lib.build_library()
    L = _lib.lib()
    ptr = 4096

    def dfa(B=2, k=3, C=13, N=4, F=11, gs=ptr, gc=ptr, n=11, ws=1 << 40):
        return L.glass_beam_search_merged_dfa(ptr, ptr, ptr, B, k, 8, 256, C, 5, 1, ptr, ptr, ptr, ptr, N, 1, F, ptr, gs, gc, n, ptr, ptr,
                                              ptr, ptr, None, ptr, ws, None)

    def wdfa(B=2, k=3, C=13, N=4, F=11, gs=ptr, gc=ptr, n=11, ws=1 << 40, scale=1.0):
        return L.glass_beam_search_merged_wdfa(ptr, ptr, ptr, B, k, 8, 256, C, 5, 1, ptr, ptr, ptr, ptr, ptr, ptr, N, 1, F, ptr, scale,
                                               gs, gc, n, ptr, ptr, ptr, ptr, ptr, None, ptr, ws, None)
    for call, fn in ((dfa, "glass_beam_search_merged_dfa"), (wdfa, "glass_beam_search_merged_wdfa")):
        for kw, what in ((dict(k=17), "k=17"), (dict(k=14), "k=14"), (dict(N=0), "N=0"), (dict(F=257), "F=257"),
                         (dict(gs=None), "null group array"), (dict(gc=None), "null group array"), (dict(n=0), "n_group_cls=0"),
                         (dict(n=14), "n_group_cls=14"), (dict(ws=16), "workspace too small")):
            assert call(**kw) < 0, (fn, kw)
            msg = L.glass_last_error().decode()
            assert what in msg and msg.startswith(fn + ":"), (fn, kw, msg)
        assert call(B=0) == 0                                                   # nothing to do, nothing launched
    assert wdfa(scale=float("inf")) < 0 and "weight_scale" in L.glass_last_error().decode()


# ------------------------------------------------------------------ the surface: every ValueError, the config key
def test_host_surface():
    from glass_amd.evaluation import inference_on_dataset
    from glass_amd.evaluation.lexicon import LexiconTrie
    from glass_amd.evaluation.pattern import DecodePattern
    from glass_amd.modeling.recognition.recognizer_decoder import ASTER_V2
    from glass_amd.modeling.recognition.recognizer_head_v2 import RecognizerRCNNHeadV3
    from glass_amd.structures.core import ShapeSpec
    chars = LC.shipped_characters()
    pat = DecodePattern(r"[a-z]+", chars, 26, 1, case_insensitive=True, device="cpu")
    trie = LexiconTrie(["car", "Card"], chars, 26, 1, device="cpu")
    dec = ASTER_V2(_cfg(), ShapeSpec(channels=256))
    x = torch.zeros((2, 8, 256))
    with pytest.raises(ValueError, match="merge_case needs pattern"):
        dec.beam_decode(x, 3, 1, merge_case=True)
    with pytest.raises(ValueError, match="DecodePattern.from_trie"):
        dec.beam_decode(x, 3, 1, lexicon=trie, merge_case=True)
    with pytest.raises(ValueError, match="max_len"):
        dec.beam_decode(x, 3, 1, pattern=DecodePattern(r"\d+", chars, 25, 1, device="cpu"), merge_case=True)
    # ---- the config key: off by default, needs DECODE_PATTERN, builds a case-insensitive pattern and merges
    assert _cfg().MODEL.ROI_RECOGNIZER_HEAD.DECODE_MERGE_CASE is False
    beam = ["MODEL.ROI_RECOGNIZER_HEAD.BEAM_WIDTH", 3]
    with pytest.raises(ValueError, match="DECODE_MERGE_CASE needs MODEL.ROI_RECOGNIZER_HEAD.DECODE_PATTERN"):
        RecognizerRCNNHeadV3(_cfg(beam + ["MODEL.ROI_RECOGNIZER_HEAD.DECODE_MERGE_CASE", True]), ShapeSpec(channels=256))
    rx = ["MODEL.ROI_RECOGNIZER_HEAD.DECODE_PATTERN", r"[a-z]+\d?"]
    plain = RecognizerRCNNHeadV3(_cfg(beam + rx), ShapeSpec(channels=256))
    assert plain.merge_case is False and plain.pattern.case_insensitive is False                 # the default: nothing changes
    keyed = RecognizerRCNNHeadV3(_cfg(beam + rx + ["MODEL.ROI_RECOGNIZER_HEAD.DECODE_MERGE_CASE", True]), ShapeSpec(channels=256))
    assert keyed.merge_case is True and keyed.pattern.case_insensitive is True and type(keyed.pattern) is DecodePattern
    assert keyed.pattern.accepts("AbC1") and not plain.pattern.accepts("AbC1")
    both = RecognizerRCNNHeadV3(_cfg(beam + rx + ["MODEL.ROI_RECOGNIZER_HEAD.DECODE_MERGE_CASE", True,
                                                  "MODEL.ROI_RECOGNIZER_HEAD.DECODE_LENGTH_BONUS", 0.5]), ShapeSpec(channels=256))
    assert both.merge_case is True and type(both.pattern).__name__ == "WeightedPattern" and both.pattern.weight_of("Ab") == 1.0
    # ---- set_pattern / set_lexicon
    head = RecognizerRCNNHeadV3(_cfg(beam), ShapeSpec(channels=256))
    head.set_pattern(pat, merge_case=True)
    assert head.pattern is pat and head.merge_case is True
    head.set_pattern(pat)
    assert head.merge_case is False
    head.set_pattern(pat, merge_case=True)
    head.set_pattern(None)
    assert head.pattern is None and head.merge_case is False
    head.set_lexicon(trie, merge_case=True)                         # through DecodePattern.from_trie
    assert head.lexicon is None and head.merge_case is True and type(head.pattern) is DecodePattern
    assert head.pattern.num_states == trie.num_nodes and np.array_equal(head.pattern.accept, trie.node_word)
    with pytest.raises(ValueError, match="a pattern is set"):
        head.set_lexicon(trie)
    head.set_pattern(None)
    head.set_lexicon(trie)
    assert head.lexicon is trie and head.pattern is None and head.merge_case is False
    with pytest.raises(ValueError, match="a lexicon is set"):
        head.set_lexicon(trie, merge_case=True)
    greedy = RecognizerRCNNHeadV3(_cfg(), ShapeSpec(channels=256))
    with pytest.raises(ValueError, match="BEAM_WIDTH"):
        greedy.set_lexicon(trie, merge_case=True)
    # ---- the driver
    with pytest.raises(ValueError, match="merge_case without"):
        inference_on_dataset(None, [], None, merge_case=True)


def test_native_wrappers_refuse_before_any_device_call():
    """merge=True without the group arrays, and hand-made groups that are no groups of the fold"""
    from glass_amd._lib import GlassLibraryError
    from glass_amd.ops import native as K
    t = dict(MC.hand_inputs()["tables"])
    bad = dict(t, group_cls=t["group_cls"][::-1].copy())
    x = torch.zeros((1, 7, 256))
    for fn in (K.beam_search_dfa, K.beam_search_wdfa):
        with pytest.raises((ValueError, GlassLibraryError)):        # (x is on the CPU: the first check of every wrapper)
            fn(x, x, {}, 3, 13, 5, 0, t, torch.zeros(1, dtype=torch.int32), merge=True)
    with pytest.raises(GlassLibraryError, match="group_start and group_cls"):
        K._merge_arrays("beam_search_dfa", {"fold": t["fold"]}, {"fold": t["fold"]}, 13, 5, 0, torch.device("cpu"))
    with pytest.raises(ValueError, match="ascending|equal within"):
        K._merge_arrays("beam_search_dfa", bad, {"fold": bad["fold"]}, 13, 5, 0, torch.device("cpu"))
    arrays = {"fold": t["fold"]}
    gs, gc, n = K._merge_arrays("beam_search_dfa", t, arrays, 13, 5, 0, torch.device("cpu"))
    assert n == 11 and gs.dtype == gc.dtype == arrays["fold"].dtype == torch.int32 and gs.tolist() == t["group_start"].tolist()


# ------------------------------------------------------------------ the replay's cases
@pytest.mark.parametrize("name", list(MC.CASES))
def test_case_seeds_margins_and_invariant(name):
    """conditions on the float64 replay alone: the committed seed is the first whose smallest margin (rank gap at the k-th
    place, representative gap inside a selected group, final order) is at least MARGIN = 1e-3, at most half of the tried seeds
    were rejected, the k folded strings of every item are distinct, every hypothesis is a word of the language"""
    c = MC.CASES[name]
    seed, tried, f = MC.find_seed(name)
    assert (seed, tried) == (c["seed"], c["tried"]), (name, seed, tried)
    d = MC.case_data(name)
    assert torch.equal(d["f64"]["symbols"], f["symbols"])
    k, B = d["k"], d["B"]
    fin = torch.isfinite(f["scores"])
    print(f"[merged] {name}: seed {seed} ({tried} tried), smallest margin {float(f['margin'].min()):.3e}, completed "
          f"{f['completed'].tolist()[:6]}, finite {fin.sum(1).tolist()[:6]}")
    assert MC.MARGIN == 1e-3 == 10 * MC.TOL
    for b, key in enumerate(d["item_keys"]):
        texts = [f["folded"][b][i] for i in range(k) if fin[b, i]]
        assert len(set(texts)) == len(texts), (name, b, texts)
        for i, w in enumerate(texts):
            assert w in d["words"][key] and int(f["lengths"][b, i]) == len(w) + 1
            spelled = "".join(d["keys"][int(s)] for s in f["symbols"][b, i, :len(w)])
            assert spelled == w                                       # the representatives fold to the string
            want = float(f["model_scores"][b, i]) + d["scale"] * d["weights"][key].total(w)
            assert float(f["scores"][b, i]) == pytest.approx(want, abs=1e-9)
    if name == MC.EXHAUSTED:
        assert len(set(d["words"][None])) == 3 < k and (fin.sum(1) == 3).all()
    if name == MC.EMPTY:
        assert fin[[0, 3]].all() and not fin[1].any() and not fin[2].any() and MC.item_segments(d) == [0, 1, 5, 0]
    if name == "priors_twins_k4_c13":
        assert d["words"][None].count("AB") == 3 and all(f["folded"][b].count("AB") == 1 for b in range(B))
    if name == "trie_twins_k5_c97":
        assert len(d["words"][None]) > len(set(d["words"][None]))     # case twins in the lexicon
    if name == "sensitive_k5_c97":
        assert all(len(g) == 1 for g in MC.groups_of(d["keys"]).values())


def test_the_merged_score_is_the_summed_mass_of_the_casings():
    """the replay against plain enumeration on a one-step language: with L = 2 a hypothesis is one folded character and its
    score is log(sum of the softmax over the character's classes) + the stop's log-probability along the representative"""
    import beam_cases as BC
    chars, eos, C = MC.C13, 1, 13
    keys = LC.class_keys(chars, eos, True)
    roots, _, _ = LC.dict_tries(["a", "b", "1"], chars, 3, eos, True)
    sd = BC.decoder_sd(C, fc_scale=1.0, eos=eos)
    x = BC.rand_x(2, 7, 100)
    f = MC.replay(sd, x, 3, C, 3, eos, keys, [roots[0]] * 2)
    step = BC.f64_step(sd, x, BC.xproj_f64(sd, x))
    for b in range(2):
        item = torch.tensor([b])
        logits, h = step(torch.zeros((1, 256), dtype=torch.float64), torch.zeros(1, dtype=torch.long), item)
        p = torch.softmax(logits[0], 0)
        want = {}
        for key, cls in (("A", [2, 11]), ("B", [3, 12]), ("1", [6])):
            rep = max(cls, key=lambda c: (float(p[c]), -c))
            l2, _ = step(h, torch.tensor([rep]), item)
            want[key] = (float(torch.log(p[cls].sum())) + float(torch.log_softmax(l2[0], 0)[eos]), rep)
        got = {f["folded"][b][i]: (float(f["scores"][b, i]), int(f["symbols"][b, i, 0])) for i in range(3)}
        assert set(got) == set(want)
        for key in want:
            assert got[key][1] == want[key][1] and got[key][0] == pytest.approx(want[key][0], abs=1e-12)


def test_hand_made_case_and_known_answer_inputs():
    d = MC.hand_data()
    f = d["f64"]
    fin = torch.isfinite(f["scores"])
    assert fin.all(), "k = 5 hypotheses of the 5-symbol language for every item"
    dead = "PQRST"[MC.HAND["dead_symbol"]]
    assert all(dead not in w for b in range(d["B"]) for w in f["folded"][b]), "the all -inf group is never emitted"
    emitted = {int(s) for b in range(d["B"]) for i in range(d["k"]) for s in f["symbols"][b, i, :int(f["lengths"][b, i]) - 1]}
    assert emitted & {1, 5, 12} and emitted & {2, 3, 7, 9}, "the groups of three and of four are exercised"
    sd, chars = MC.known_sd()
    import beam_cases as BC
    for name in ("fc.weight", "fc.bias", "tgt_embedding.weight"):
        w = sd[BC.Q + name]
        assert torch.equal(w[chars.index("q")], w[chars.index("Q")]) and not torch.equal(w[chars.index("q")], w[chars.index("r")])
