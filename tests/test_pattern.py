"""CPU: the host side of pattern-constrained decoding - the regex compiler of evaluation/pattern.py against `re.fullmatch`,
its tables (dist, trimming, minimisation, reproducibility, limits, from_trie / from_charset), the float64 replay's cases of
tests/pattern_cases.py (their gaps against MARGIN), the per-feature header and its binding, and what the model surface
refuses."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import lexicon_beam_cases as LC
import pattern_cases as PC

ROOT = LC.ROOT
NAMES = ["glass_beam_search_dfa_workspace_bytes", "glass_beam_search_dfa"]


def _pattern(p, chars=PC.SMALL, L=8, eos=1, **kw):
    from glass_amd.evaluation.pattern import DecodePattern
    return DecodePattern(p, chars, L, eos, device="cpu", **kw)


# ------------------------------------------------------------------ the compiler
@pytest.mark.parametrize("ci", [False, True])
@pytest.mark.parametrize("regex", PC.REGEXES)
def test_compiler_against_re_fullmatch(regex, ci):
    """every string of up to 5 characters over the small set (the empty one included); minimize=True and False accept the
    same strings"""
    rx = re.compile(regex, re.IGNORECASE if ci else 0)
    p, q = _pattern(regex, case_insensitive=ci), _pattern(regex, case_insensitive=ci, minimize=False)
    assert p.num_states <= q.num_states and p.num_fold == (4 if ci else 6)
    accepted = 0
    for w in PC.strings_up_to(PC.SMALL_ALPHABET, 5):
        want = rx.fullmatch(w) is not None
        assert p.accepts(w) == want, (regex, ci, w)
        assert q.accepts(w) == want, (regex, ci, w, "minimize=False")
        accepted += want
    if regex in (r"[xyz]a?", r"[^\w\-]b"):
        assert accepted == 0 and p.num_states == 1 and p.start.tolist() == [-1], "an empty class is legal and matches nothing"
    assert not p.accepts("a[") and not p.accepts("Ā")                 # a character outside the set


@pytest.mark.parametrize("regex", PC.UNSUPPORTED)
def test_unsupported_constructs_raise(regex):
    with pytest.raises(ValueError, match="position"):
        _pattern(regex)


def test_the_regex_lists_cover_what_the_issue_names():
    assert len(PC.REGEXES) >= 30
    assert any("((" in r or "(a(b" in r for r in PC.REGEXES) and any("{0," in r for r in PC.REGEXES)
    assert r"ab|a" in PC.REGEXES and r"[xyz]a?" in PC.REGEXES
    for r in PC.REGEXES:
        re.compile(r)


# ------------------------------------------------------------------ the tables
@pytest.mark.parametrize("minimize", [True, False])
@pytest.mark.parametrize("regex", PC.REGEXES + [r"a{63}", r"(a|b){5}1{2,}"])
def test_tables(regex, minimize):
    """dist = an independent breadth-first search; no state without a path to acceptance; the packed field; states in
    breadth-first order; two builds give identical arrays"""
    p, again = _pattern(regex, L=64, minimize=minimize), _pattern(regex, L=64, minimize=minimize)
    for n in ("next", "accept", "start", "fold", "dist"):
        assert np.array_equal(getattr(p, n), getattr(again, n)) and getattr(p, n).dtype == np.int32, n
    N, F = p.next.shape
    assert (N, F) == (p.num_states, p.num_fold) and p.accept.shape == (N,) and p.start.shape == (1,) and len(p) == 1
    assert p.nbytes == p.next.nbytes + p.accept.nbytes + p.start.nbytes + p.fold.nbytes and p.build_seconds > 0
    assert p.fold.tolist() == [-1, -1, 0, 1, 2, 3, 4, 5]
    dist = PC.bfs_dist(p.next, p.accept)
    if p.start[0] < 0:
        assert N == 1 and dist == [None] and not (p.next >= 0).any()
        return
    assert None not in dist, "a state without a path to acceptance"
    assert p.dist.tolist() == dist
    live = p.next >= 0
    tgt = p.next & 0xFFFFFF
    assert (tgt[live] < N).all() and ((p.next[live] >> 24) == np.minimum(p.dist[tgt[live]], 127)).all()
    assert (p.next[~live] == -1).all() and set(np.unique(p.accept)) <= {-1, 0}
    # breadth-first numbering from the start state, symbols ascending: first visits come in increasing order
    assert p.start[0] == 0
    seen, order = {0}, [0]
    for q in order:
        for f in range(F):
            if live[q, f] and int(tgt[q, f]) not in seen:
                seen.add(int(tgt[q, f]))
                order.append(int(tgt[q, f]))
    assert order == list(range(N))
    for n, t in p.tensors.items():
        assert t == F if n == "F" else np.array_equal(t.numpy(), getattr(p, n)), n


def test_a63_fills_the_distance_field_and_minimisation_shrinks():
    p = _pattern(r"a{63}", L=64)
    assert p.num_states == 64 and p.dist[0] == 63 and p.start[0] == 0 and (p.next[0, 0] >> 24) == 62
    assert _pattern(r"a{63}", L=63).start.tolist() == [-1], "63 characters need 64 steps"
    assert _pattern(r"a{200}b", L=64).dist.max() == 201                       # stored as min(dist, 127)
    assert (_pattern(r"a{200}b", L=64).next[0, 0] >> 24) == 127
    assert _pattern(r"(a|b)*1|(b|a)*1", minimize=True).num_states == 2 < _pattern(r"(ab|a1|b1)", minimize=False).num_states


def test_limits_raise():
    from glass_amd.evaluation import pattern as P
    with pytest.raises(ValueError, match="NFA"):
        _pattern(r"(a{1000}){1000}")
    with pytest.raises(ValueError, match="NFA"):
        _pattern(r"a{40}", nfa_cap=64)
    with pytest.raises(ValueError, match="table"):
        _pattern(r"a{40}", table_cap_bytes=6 * 4 * 8)
    trie = _trie(["abab", "b1"], PC.SMALL, 8, 1)
    with pytest.raises(ValueError, match="table"):
        P.DecodePattern.from_trie(trie, table_cap_bytes=64)
    old = P.MAX_STATES
    P.MAX_STATES = 5
    try:
        with pytest.raises(ValueError, match="2\\^24"):
            _pattern(r"a{40}")
        with pytest.raises(ValueError, match="2\\^24"):
            P.DecodePattern.from_trie(trie)
    finally:
        P.MAX_STATES = old
    with pytest.raises(ValueError, match="eos"):
        _pattern(r"a", eos=9)
    with pytest.raises(TypeError):
        _pattern(["a"])


def _trie(lexicon, chars, L, eos, ci=True):
    from glass_amd.evaluation.lexicon import LexiconTrie
    return LexiconTrie(lexicon, chars, L, eos, case_insensitive=ci, device="cpu")


def test_segments_keys_and_charset():
    from glass_amd.evaluation.pattern import DecodePattern
    p = _pattern({"d": r"1+", 7: r"[ab]+", "none": r"[xyz]", "d2": r"1+"})
    assert p.keys == ["d", 7, "none", "d2"] and len(p) == 4 and [p.segment(k) for k in p.keys] == [0, 1, 2, 3]
    with pytest.raises(KeyError):
        p.segment("e")
    assert p.start.tolist()[2] == -1 and p.start[0] == 0 and p.start[0] == p.start[3], "equal languages share their states"
    assert p.accepts("11", "d") and not p.accepts("11", 7) and p.accepts("ab", 7) and not p.accepts("a", "none")
    c = DecodePattern.from_charset("a1-", PC.SMALL, 8, 1, device="cpu")
    r = _pattern(r"[a1\-]+")
    for n in ("next", "accept", "start", "fold"):
        assert np.array_equal(getattr(c, n), getattr(r, n)), n
    assert c.accepts("a-1") and not c.accepts("") and not c.accepts("ab") and c.tag("a") == 0 and c.tag("b") == -1
    with pytest.raises(ValueError):
        DecodePattern.from_charset("", PC.SMALL, 8, 1, device="cpu")


@pytest.mark.parametrize("name", list(LC.CASES))
def test_from_trie_accepts_exactly_the_kept_words(name):
    """the trie as a DFA: one state per node, the same fold and keys, accept = node_word, start = seg_root; the transitions
    are the trie's children and dist an independent breadth-first search"""
    from glass_amd.evaluation.pattern import DecodePattern
    d = LC.case_data(name)
    trie = _trie(d["lexicon"], d["characters"], d["L"], d["eos"], d["case_insensitive"])
    p = DecodePattern.from_trie(trie)
    assert p.num_states == trie.num_nodes and p.keys == trie.keys and p.num_fold == trie.num_fold
    assert np.array_equal(p.fold, trie.fold) and np.array_equal(p.accept, trie.node_word) and np.array_equal(p.start, trie.seg_root)
    assert (p.num_classes, p.max_len, p.eos) == (trie.num_classes, trie.max_len, trie.eos)
    dist = PC.bfs_dist(p.next, p.accept)
    if any(s >= 0 for s in trie.seg_root):
        assert p.dist.tolist() == dist
    known = {k for k in d["keys"] if k is not None}
    pos = 0
    for key in (d["lexicon"] if isinstance(d["lexicon"], dict) else [None]):
        words = d["lexicon"][key] if isinstance(d["lexicon"], dict) else d["lexicon"]
        for j, w in enumerate(words):
            text = w.upper() if d["case_insensitive"] else w
            kept = bool(text) and len(text) <= d["L"] - 1 and all(ch in known for ch in text)
            assert p.accepts(w, key) == kept, (name, key, w)
            if kept:
                first = min(pos + i for i, v in enumerate(words) if (v.upper() if d["case_insensitive"] else v) == text)
                assert p.tag(w, key) == first
                assert not p.accepts(w + w[-1] * 70, key)
        pos += len(words)
        for w in LC.random_words(np.random.default_rng(5), [c for c in d["characters"] if len(c) == 1], 200, 1, 4):
            text = w.upper() if d["case_insensitive"] else w
            assert p.accepts(w, key) == (text in {(v.upper() if d["case_insensitive"] else v) for v in words}
                                         and len(text) <= d["L"] - 1 and all(ch in known for ch in text)), (name, key, w)


# ------------------------------------------------------------------ the search cases
@pytest.mark.parametrize("name", list(PC.CASES))
def test_cases_have_their_gaps_and_properties(name):
    """no selection and no pair of neighbouring completions of any item is a near-tie (the GPU test compares symbols
    exactly); every hypothesis of the replay is a word of the enumerated language and the pattern built by the product
    accepts exactly that language; every case exercises what it is named for"""
    d = PC.case_data(name)
    f, k, L, eos = d["f64"], d["k"], d["L"], d["eos"]
    fin = torch.isfinite(f["scores"])
    print(f"[pattern] {name}: smallest selection gap {float(f['sel_gap'].min()):.3e}, smallest completion gap "
          f"{float(f['done_gap'].min()):.3e}, completed {f['completed'].tolist()[:8]}, words {[len(w) for w in d['words'].values()]}, "
          f"lowest score {float(f['scores'][fin].min()) if fin.any() else None}")
    assert min(float(f["sel_gap"].min()), float(f["done_gap"].min())) > PC.MARGIN, \
        "a near-tie: choose another seed for this case, do not relax the margin"
    p = _pattern(d["patterns"], d["characters"], L, eos, case_insensitive=d["ci"])
    for key, words in d["words"].items():
        assert all(p.accepts(w, key) for w in words[:2000]) and (bool(words) == (p.start[p.segment(key)] >= 0))
    for b, key in enumerate(d["item_keys"]):
        for i in range(k):
            n = int(f["lengths"][b, i])
            assert (n > 0) == bool(fin[b, i])
            if n:
                text = PC.text_of(f["symbols"][b, i], n, d["characters"])
                assert (text.upper() if d["ci"] else text) in set(d["words"][key]) and p.accepts(text, key)
    if name == "too_long_for_l4":
        assert not fin.any() and d["words"] == {None: []}
    if name == "digits_l4_k5":
        assert len(d["words"][None]) == 5 + 25 + 125 and (f["completed"] > k).all() and fin.all()
    if name == "plates_c97_l26_t32_k3":
        assert len(d["words"][None]) == 26 * 26 * 1100 and p.num_fold < 95 and fin.all()
    if name == "shared_prefix_k4":
        assert sorted(d["words"][None]) == ["a", "ab", "abc", "ac"] and (f["completed"] == k).all()      # all four complete
    if name == "star_k4":
        assert (f["completed"] > k).all()
    if name == "rows512_b32_k16":
        assert d["B"] * k == 512 and fin.all()
    if name == "c256_identity":
        assert p.num_fold == 254 and p.next.shape[1] == 254 and int(p.fold.max()) == 253 and fin.all()
    if name == "l64_a63":
        assert d["words"] == {None: ["a" * 63]} and p.dist[p.start[0]] == 63 and (f["lengths"][:, 0] == 64).all() and not fin[:, 1].any()
    if name == "two_segments":
        assert not fin[2].any() and not fin[3].any() and fin[[0, 1, 4]].all() and PC.item_segments(d) == [0, 1, -1, 2, 1]
    if name in PC.EXHAUSTIVE:
        assert len(d["words"][None]) <= k and all(len(w) < L - 1 for w in d["words"][None])
        assert (fin.sum(1) == len(d["words"][None])).all()


# ------------------------------------------------------------------ the header and the model surface
def test_feature_header_and_binding():
    from glass_amd import _lib
    with open(os.path.join(ROOT, "include", "glass_hip_feature_dfa.h")) as fh:
        text = fh.read()
    assert '#include "glass_hip.h"' in text
    assert list(_lib.signatures(text)) == NAMES
    for name in NAMES:
        assert _lib.FEATURE_EXPORTS.count(name) == 1 and name not in _lib.EXPORTS + _lib.EXT_EXPORTS + _lib.ADDON_EXPORTS, name
    for other in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if other != "glass_hip_feature_dfa.h":
            with open(os.path.join(ROOT, "include", other)) as fh:
                assert "glass_beam_search_dfa" not in fh.read(), other
    assert "glass_hip_feature_dfa.h" in [os.path.basename(p) for p in _lib.feature_headers()]
    _lib.build_library()
    L = _lib.lib()
    p, i, l = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    assert L.glass_beam_search_dfa_workspace_bytes.restype is l and L.glass_beam_search_dfa_workspace_bytes.argtypes == [i] * 6
    assert L.glass_beam_search_dfa.restype is i
    assert L.glass_beam_search_dfa.argtypes == [p, p, p] + [i] * 7 + [p] * 4 + [i] * 3 + [p] * 6 + [p, l, p]
    assert L.glass_abi_version() == _lib.ABI_VERSION == 8
    assert (L.glass_beam_search_dfa_workspace_bytes(3, 5, 32, 256, 97, 26)
            == L.glass_beam_search_lexicon_workspace_bytes(3, 5, 32, 256, 97, 26))


def test_every_bad_argument_is_refused_on_the_host():
    """no device needed: every refusal comes before the first runtime call; the pointers are never dereferenced"""
    from glass_amd import _lib
    _lib.build_library()
    L = _lib.lib()
    ptr = 4096

    def call(B=2, k=3, T=8, D=256, C=13, max_len=5, N=4, S=1, F=11, **null):
        a = {n: (None if null.get(n) else ptr) for n in ("x", "next", "accept", "start", "fold", "item", "tags", "ws")}
        return L.glass_beam_search_dfa(a["x"], ptr, ptr, B, k, T, D, C, max_len, 1, a["next"], a["accept"], a["start"], a["fold"],
                                       N, S, F, a["item"], ptr, ptr, ptr, a["tags"], None, a["ws"], 1 << 40, None)
    for kw, what in ((dict(k=17), "k=17"), (dict(k=14), "k=14"), (dict(max_len=65), "max_len=65"), (dict(T=65), "T=65"),
                     (dict(D=128), "D=128"), (dict(C=257), "C=257"), (dict(N=0), "N=0"), (dict(N=1 << 24), "N=16777216"),
                     (dict(S=0), "S=0"), (dict(F=0), "F=0"), (dict(F=257), "F=257"), (dict(x=True), "null"), (dict(next=True), "null"),
                     (dict(accept=True), "null"), (dict(start=True), "null"), (dict(fold=True), "null"), (dict(item=True), "null"),
                     (dict(tags=True), "null"), (dict(ws=True), "null")):
        assert call(**kw) < 0, kw
        assert what in L.glass_last_error().decode(), (kw, L.glass_last_error().decode())
    assert L.glass_beam_search_dfa(ptr, ptr, ptr, 2, 3, 8, 256, 13, 5, 1, ptr, ptr, ptr, ptr, 4, 1, 11, ptr, ptr, ptr, ptr, ptr, None,
                                   ptr, 16, None) < 0 and "workspace too small" in L.glass_last_error().decode()
    assert call(B=0) == 0                                                       # nothing to do, nothing launched


def _cfg(opts=()):
    from glass_amd.config import get_glass_cfg
    return get_glass_cfg(os.path.join(ROOT, "configs", "glass_icdar15_mi355x.yaml"), ["MODEL.DEVICE", "cpu"] + list(opts))


def test_host_surface_refuses_mismatches():
    from glass_amd.evaluation import inference_on_dataset
    from glass_amd.modeling.recognition.recognizer_decoder import ASTER_V2
    from glass_amd.modeling.recognition.recognizer_head_v2 import RecognizerRCNNHeadV3
    from glass_amd.structures.core import ShapeSpec
    chars = LC.shipped_characters()
    pat = _pattern(r"\d+", chars, 26, 1)
    two = _pattern({"a": r"\d+", "b": r"[a-z]+"}, chars, 26, 1)
    trie = _trie(["car"], chars, 26, 1)
    dec = ASTER_V2(_cfg(), ShapeSpec(channels=256))
    x = torch.zeros((2, 8, 256))
    with pytest.raises(ValueError, match="lexicon and pattern"):
        dec.beam_decode(x, 3, 1, lexicon=trie, pattern=pat)
    for bad, what in ((_pattern(r"\d+", chars[:-1], 26, 1), "classes"), (_pattern(r"\d+", chars, 25, 1), "max_len"),
                      (_pattern(r"\d+", chars, 26, 0), "eos")):
        with pytest.raises(ValueError, match=what):
            dec.beam_decode(x, 3, 1, pattern=bad)
    with pytest.raises(ValueError, match="one-segment"):
        dec.beam_decode(x, 3, 1, pattern=two)
    for seg in ([0, 2], [0, -1], [0], [0.0, 1.0]):
        with pytest.raises(ValueError, match="segments"):
            dec.beam_decode(x, 3, 1, pattern=two, segments=seg)
    assert _cfg().MODEL.ROI_RECOGNIZER_HEAD.DECODE_PATTERN == ""
    head = RecognizerRCNNHeadV3(_cfg(["MODEL.ROI_RECOGNIZER_HEAD.BEAM_WIDTH", 0]), ShapeSpec(channels=256))
    assert head.pattern is None
    with pytest.raises(ValueError, match="BEAM_WIDTH"):
        head.set_pattern(pat)
    head.set_pattern(None)
    with pytest.raises(ValueError, match="BEAM_WIDTH"):
        RecognizerRCNNHeadV3(_cfg(["MODEL.ROI_RECOGNIZER_HEAD.DECODE_PATTERN", r"\d+"]), ShapeSpec(channels=256))
    with pytest.raises(ValueError, match="position"):
        RecognizerRCNNHeadV3(_cfg(["MODEL.ROI_RECOGNIZER_HEAD.BEAM_WIDTH", 3, "MODEL.ROI_RECOGNIZER_HEAD.DECODE_PATTERN", r"^\d+$"]),
                             ShapeSpec(channels=256))
    head = RecognizerRCNNHeadV3(_cfg(["MODEL.ROI_RECOGNIZER_HEAD.BEAM_WIDTH", 3]), ShapeSpec(channels=256))
    with pytest.raises(ValueError, match="eos"):
        head.set_pattern(_pattern(r"\d+", chars, 26, 0))
    with pytest.raises(ValueError, match="image_segments"):
        head.set_pattern(pat, torch.zeros((2,), dtype=torch.int32))             # a host tensor
    head.set_pattern(pat)
    assert head.pattern is pat and head.image_segments is None and head.lexicon is None
    with pytest.raises(ValueError, match="pattern is set"):
        head.set_lexicon(trie)
    head.set_lexicon(None)
    assert head.pattern is pat
    head.set_pattern(None)
    head.set_lexicon(trie)
    with pytest.raises(ValueError, match="lexicon is set"):
        head.set_pattern(pat)
    head.set_lexicon(None)
    built = RecognizerRCNNHeadV3(_cfg(["MODEL.ROI_RECOGNIZER_HEAD.BEAM_WIDTH", 3, "MODEL.ROI_RECOGNIZER_HEAD.DECODE_PATTERN", r"[A-Z]{2}\d+"]),
                                 ShapeSpec(channels=256))
    assert built.pattern is not None and built.pattern.keys == [None] and not built.pattern.case_insensitive
    assert built.pattern.accepts("AB12") and not built.pattern.accepts("ab12")
    with pytest.raises(ValueError, match="pattern_key"):
        inference_on_dataset(None, [], lambda d: d, pattern_key=lambda inp: 0)
    with pytest.raises(ValueError, match="together"):
        inference_on_dataset(None, [], lambda d: d, lexicon=trie, pattern=pat)
