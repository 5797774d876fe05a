"""CPU: the lexicon trie (`LexiconTrie`) against a dict-of-dicts trie, the fold tables, the float64 constrained search of
tests/lexicon_beam_cases.py against plain enumeration, the properties its cases must have (gaps, dead slots, more completions
than k, ...), the extension header, and the argument checks of the host surface."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import beam_cases as BC
import forced_cases as FC
import lexicon_beam_cases as LC

ROOT = LC.ROOT


def _trie(lexicon, chars, max_len, eos, ci=True):
    from glass_amd.evaluation.lexicon import LexiconTrie
    return LexiconTrie(lexicon, chars, max_len, eos, case_insensitive=ci, device="cpu")


def _mask_ints(trie):
    """every node's mask words as one Python int (bit f = fold symbol f)"""
    out = [0] * trie.num_nodes
    for q in range(trie.mask_words):
        for n, w in enumerate(trie.child_mask[:, q].tolist()):
            out[n] |= w << (32 * q)
    return out


def _child(trie, masks, node, f):
    """the lookup of the ABI: child_base + popcount(mask bits below f), or -1"""
    if not (masks[node] >> f) & 1:
        return -1
    return int(trie.child_base[node]) + bin(masks[node] & ((1 << f) - 1)).count("1")


def _compare(trie, roots, keys, every_symbol=True):
    """walk the arrays and the dict tries together -> number of nodes seen.  Every node: its word; every (node, fold symbol):
    the child by mask and popcount exists exactly where the dict has one; children contiguous, ordered by fold symbol and
    numbered after every node of the level above (breadth-first order)."""
    sym_of = {}
    for c, key in enumerate(keys):
        if key is not None:
            sym_of.setdefault(key, int(trie.fold[c]))
            assert sym_of[key] == int(trie.fold[c]) >= 0
        else:
            assert int(trie.fold[c]) == -1
    assert sorted(sym_of.values()) == list(range(trie.num_fold))
    masks = _mask_ints(trie)
    assert len(roots) == len(trie.seg_root)
    level = []
    for root, r in zip(roots, trie.seg_root.tolist()):
        assert (root is None) == (r == -1)
        if root is not None:
            level.append((r, root))
    assert [n for n, _ in level] == list(range(len(level)))
    seen = 0
    while level:
        nxt = []
        for node, d in level:
            seen += 1
            assert int(trie.node_word[node]) == d["word"]
            want = sorted((sym_of[key], key) for key in d["ch"])
            if every_symbol:
                assert [f for f in range(trie.num_fold) if _child(trie, masks, node, f) >= 0] == [f for f, _ in want]
            else:
                assert bin(masks[node]).count("1") == len(want)
            kids = [_child(trie, masks, node, f) for f, _ in want]
            assert kids == list(range(int(trie.child_base[node]), int(trie.child_base[node]) + len(kids))) or not kids
            nxt += [(kid, d["ch"][key]) for kid, (_, key) in zip(kids, want)]
        assert [n for n, _ in nxt] == list(range(level[-1][0] + 1, level[-1][0] + 1 + len(nxt)))      # breadth-first numbering
        level = nxt
    return seen


@pytest.mark.parametrize("seed, ci, C", [(1, True, 97), (2, False, 97), (3, True, 13), (4, False, 256)])
def test_trie_against_dict_trie(seed, ci, C):
    """seeded random lexicons of several segments (one of them empty), with duplicates, empty words, words that are too
    long and words with a character the set does not have"""
    rng = np.random.default_rng(seed)
    chars = LC.shipped_characters() if C == 97 else LC.generic_characters(C)
    eos, L = (1, 9) if C == 97 else (0, 6)
    al = chars[2:] if C != 97 else [c for c in chars[2:] if c.isalnum()]
    lex = {}
    for s in range(4):
        words = LC.random_words(rng, al[:12], 40, 1, L + 1) + LC.random_words(rng, al, 25, 1, 4)
        words += ["", words[3], words[5].swapcase(), al[0] + "中", words[0]]
        lex[f"s{s}"] = words
    lex["empty"] = []
    lex["only_bad"] = ["", "中" * 2]
    trie = _trie(lex, chars, L, eos, ci)
    roots, skipped, upper = LC.dict_tries(lex, chars, L, eos, ci)
    keys = LC.class_keys(chars, eos, ci)
    assert trie.skipped == skipped and min(skipped.values()) > 0
    assert trie.upper == upper and len(trie) == len(upper)
    assert trie.mask_words == math.ceil(trie.num_fold / 32) and trie.child_mask.shape == (trie.num_nodes, trie.mask_words)
    assert trie.child_mask.dtype == np.uint32 and trie.child_base.dtype == trie.node_word.dtype == trie.seg_root.dtype == np.int32
    assert _compare(trie, roots, keys) == trie.num_nodes
    assert trie.segment("s2") == 2 and trie.seg_root[trie.segment("empty")] == trie.seg_root[trie.segment("only_bad")] == -1
    with pytest.raises(KeyError):
        trie.segment("nope")
    for name, t in trie.tensors.items():
        if name != "F":
            assert t.dtype == torch.int32 and t.is_contiguous()
    assert trie.tensors["F"] == trie.num_fold
    assert np.array_equal(trie.tensors["child_mask"].numpy().view(np.uint32), trie.child_mask)


def test_trie_length_limit_terminal_with_children_and_duplicates():
    chars = LC.shipped_characters()
    trie = _trie(["car", "Card", "CAR", "x" * 25, "y" * 26, "cards"], chars, 26, 1)
    assert trie.skipped == {"empty": 0, "too_long": 1, "no_class": 0}
    masks = _mask_ints(trie)

    def walk(text):
        node = int(trie.seg_root[0])
        for ch in text:
            node = _child(trie, masks, node, int(trie.fold[chars.index(ch)]))
            if node < 0:
                return None
        return node
    assert trie.node_word[walk("CAR")] == 0 and trie.node_word[walk("car")] == 0          # "CAR" (index 2) is a duplicate
    assert trie.node_word[walk("cArD")] == 1 and trie.node_word[walk("CARDS")] == 5
    assert trie.node_word[walk("CA")] == -1 and masks[walk("CAR")] != 0                  # a terminal with children
    assert trie.node_word[walk("x" * 25)] == 3 and walk("y") is None
    assert trie.upper[1] == "CARD"
    one = _trie({"a": [], "b": [""]}, chars, 26, 1)                                       # no word at all: still no empty array
    assert one.num_nodes == 1 and one.seg_root.tolist() == [-1, -1] and one.node_word.tolist() == [-1]
    exact = _trie(["ab"], chars, 3, 1)
    assert exact.skipped["too_long"] == 0 and _trie(["abc"], chars, 3, 1).skipped["too_long"] == 1


def test_trie_with_more_than_65536_nodes():
    rng = np.random.default_rng(5)
    chars = LC.shipped_characters()
    al = [c for c in chars if len(c) == 1 and c.islower()]
    words = LC.random_words(rng, al, 30000, 5, 7)
    trie = _trie(words, chars, 26, 1)
    roots, skipped, _ = LC.dict_tries(words, chars, 26, 1)
    assert trie.num_nodes > 65536 and trie.skipped == skipped
    assert _compare(trie, roots, LC.class_keys(chars, 1), every_symbol=False) == trie.num_nodes


def test_fold_tables():
    chars = LC.shipped_characters()
    trie = _trie(["a"], chars, 26, 1)
    F = trie.num_fold
    assert trie.mask_words == math.ceil(F / 32) and 1 <= trie.mask_words <= 8
    assert trie.fold[chars.index("a")] == trie.fold[chars.index("A")] >= 0
    assert trie.fold[chars.index("[GO]")] == trie.fold[chars.index("[s]")] == -1
    assert sorted(set(trie.fold.tolist()) - {-1}) == list(range(F))
    assert F == len({c.upper() for c in chars if len(c) == 1})
    ident = _trie(["a"], chars, 26, 1, ci=False)
    assert ident.num_fold == len([c for c in chars if len(c) == 1]) and len(set(ident.fold.tolist()) - {-1}) == ident.num_fold
    wide = _trie([], LC.generic_characters(256), 26, 0, ci=False)
    assert wide.num_fold == 254 and wide.mask_words == 8 and wide.fold[:2].tolist() == [-1, -1]
    assert wide.fold[2:].tolist() == list(range(254))
    folded = _trie([], LC.generic_characters(256), 26, 0, ci=True)
    assert folded.num_fold < 254                                        # Latin Extended-A folds in pairs
    with pytest.raises(ValueError):
        _trie([], ["[GO]", "[s]"] + [chr(0x4e00 + i) for i in range(300)], 26, 0)


@pytest.mark.parametrize("name", LC.EXHAUSTIVE)
def test_replay_is_exhaustive_on_small_segments(name):
    """identity fold, at most k words per segment, every word shorter than max_len - 1: nothing is ever pruned, so the finite
    hypotheses are exactly the segment's words and their scores the float64 teacher-forced scores of word + eos"""
    d = LC.case_data(name)
    f, k, L, eos, chars = d["f64"], d["k"], d["L"], d["eos"], d["characters"]
    assert not d["case_insensitive"]
    all_words = [w for key in d["lexicon"] for w in d["lexicon"][key]]
    targets = torch.full((d["B"], k, L), eos, dtype=torch.long)
    for b, key in enumerate(d["item_keys"]):
        words = d["lexicon"][key]
        assert len(words) == len(set(words)) <= k and all(0 < len(w) < L - 1 for w in words)
        n = int(torch.isfinite(f["scores"][b]).sum())
        got = [all_words[int(i)] for i in f["words"][b, :n]]
        assert sorted(got) == sorted(words) and (f["words"][b, n:] == -1).all() and (f["lengths"][b, n:] == 0).all()
        for i, w in enumerate(got):
            assert f["symbols"][b, i].tolist() == [chars.index(ch) for ch in w] + [eos] * (L - len(w))
            assert int(f["lengths"][b, i]) == len(w) + 1
        targets[b] = f["symbols"][b]
    forced = FC.forced_f64(d["sd"], d["x"], targets, f["lengths"], eos)
    fin = torch.isfinite(f["scores"])
    assert float((forced["scores"][fin] - f["scores"][fin]).abs().max()) < 1e-9
    assert (f["scores"][:, :-1] >= f["scores"][:, 1:]).all()


@pytest.mark.parametrize("name", list(LC.CASES))
def test_cases_have_their_gaps_and_properties(name):
    """no selection and no pair of neighbouring completions of any item is a near-tie (the GPU test compares symbols
    exactly), and every case exercises what it is named for"""
    d = LC.case_data(name)
    f, k, eos = d["f64"], d["k"], d["eos"]
    gap = min(float(f["sel_gap"].min()), float(f["done_gap"].min()))
    print(f"[lexbeam] {name}: smallest selection gap {float(f['sel_gap'].min()):.3e}, smallest completion gap "
          f"{float(f['done_gap'].min()):.3e}, completed {f['completed'].tolist()}, scores {float(f['scores'][torch.isfinite(f['scores'])].min()) if torch.isfinite(f['scores']).any() else None}")
    assert gap > LC.MARGIN, "a near-tie: choose another seed for this case, do not relax the margin"
    fin = torch.isfinite(f["scores"])
    assert ((f["lengths"] > 0) == fin).all() and ((f["words"] >= 0) == fin).all()
    for b in range(d["B"]):
        for i in range(k):
            n = int(f["lengths"][b, i])
            assert (f["symbols"][b, i, n:] == eos).all() and (n == 0 or int(f["symbols"][b, i, n - 1]) == eos)
            if n:
                text = "".join(d["characters"][int(c)] for c in f["symbols"][b, i, :n - 1])
                assert text.upper() == d["upper"][int(f["words"][b, i])]
    if name == "k1_c5_l1":
        assert not fin.any() and sum(d["skipped"].values()) == 2
    if name == "k3_c97_l26_shipped":
        assert not fin[2].any() and not fin[3].any(), "the item out of range and the item of the empty segment"
        assert int(f["lengths"][4, 0]) == 26 and int(fin[4].sum()) == 3, "the 25-character word ends at the last step"
        assert len({int(w) for w in f["words"][4]}) == 1, "three case variants of one word"
        assert any(len(set(f["words"][b, :2].tolist())) == 1 for b in (0, 1)), "two case variants alive at once"
    if name == "k4_many_completions":
        assert (f["completed"] > k).all()
    if name == "k5_dead_slots":
        assert (fin.sum(1) < k).all()
    if name == "k16_b32_l6_rows512":
        assert d["B"] * k == 512 and fin.all()


def test_extension_header_and_binding():
    from glass_amd import _lib
    with open(os.path.join(ROOT, "include", "glass_hip_ext.h")) as fh:
        text = fh.read()
    assert '#include "glass_hip.h"' in text
    sigs = _lib.signatures(text)
    names = ["glass_beam_search_lexicon_workspace_bytes", "glass_beam_search_lexicon"]
    assert list(sigs) == names == _lib.EXT_EXPORTS
    assert len(_lib.EXPORTS) == 105 and not set(names) & set(_lib.EXPORTS)
    with open(os.path.join(ROOT, "include", "glass_hip.h")) as fh:
        assert "glass_beam_search_lexicon" not in fh.read()
    _lib.build_library()
    L = _lib.lib()
    for n in names:
        assert hasattr(L, n)
    p, i, l = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    assert L.glass_beam_search_lexicon_workspace_bytes.restype is ctypes.c_int64
    assert L.glass_beam_search_lexicon_workspace_bytes.argtypes == [i] * 6
    assert L.glass_beam_search_lexicon.restype is ctypes.c_int
    assert L.glass_beam_search_lexicon.argtypes == [p, p, p] + [i] * 7 + [p] * 5 + [i] * 3 + [p] * 6 + [p, l, p]
    assert L.glass_abi_version() == _lib.ABI_VERSION == 8
    # the tables of the unconstrained search, plus one int per table entry
    assert (L.glass_beam_search_lexicon_workspace_bytes(3, 5, 32, 256, 97, 26)
            == L.glass_beam_search_workspace_bytes(3, 5, 32, 256, 97, 26) + 3 * 26 * 5 * 4)


def _cfg(opts=()):
    from glass_amd.config import get_glass_cfg
    return get_glass_cfg(os.path.join(ROOT, "configs", "glass_icdar15_mi355x.yaml"), ["MODEL.DEVICE", "cpu"] + list(opts))


def test_host_surface_refuses_mismatches():
    from glass_amd.modeling.recognition.recognizer_decoder import ASTER_V2, BeamResult
    from glass_amd.modeling.recognition.recognizer_head_v2 import RecognizerRCNNHeadV3
    from glass_amd.structures.core import ShapeSpec
    chars = LC.shipped_characters()
    trie = _trie(["car"], chars, 26, 1)
    two = _trie({"a": ["car"], "b": ["dog"]}, chars, 26, 1)
    dec = ASTER_V2(_cfg(), ShapeSpec(channels=256))
    x = torch.zeros((2, 8, 256))
    for bad, what in ((_trie(["car"], chars[:-1], 26, 1), "classes"), (_trie(["car"], chars, 25, 1), "max_len"),
                      (_trie(["car"], chars, 26, 0), "eos")):
        with pytest.raises(ValueError, match=what):
            dec.beam_decode(x, 3, 1, lexicon=bad)
    with pytest.raises(ValueError, match="one-segment"):
        dec.beam_decode(x, 3, 1, lexicon=two)
    for seg in ([0, 2], [0, -1], [0], [0.0, 1.0]):
        with pytest.raises(ValueError, match="segments"):
            dec.beam_decode(x, 3, 1, lexicon=two, segments=seg)
    with pytest.raises(ValueError, match="segments without a lexicon"):
        dec.beam_decode(x, 3, 1, segments=[0, 0])
    r = BeamResult(1, 2, 3)
    assert r.words is None and r.distributions is None and tuple(r) == (1, 2, 3, None)
    head = RecognizerRCNNHeadV3(_cfg(["MODEL.ROI_RECOGNIZER_HEAD.BEAM_WIDTH", 0]), ShapeSpec(channels=256))
    with pytest.raises(ValueError, match="BEAM_WIDTH"):
        head.set_lexicon(trie)
    head.set_lexicon(None)
    head = RecognizerRCNNHeadV3(_cfg(["MODEL.ROI_RECOGNIZER_HEAD.BEAM_WIDTH", 3]), ShapeSpec(channels=256))
    assert head.lexicon is None
    with pytest.raises(ValueError, match="eos"):
        head.set_lexicon(_trie(["car"], chars, 26, 0))
    with pytest.raises(ValueError, match="image_segments"):
        head.set_lexicon(trie, torch.zeros((2,), dtype=torch.int32))            # a host tensor
    head.set_lexicon(trie)
    assert head.lexicon is trie and head.image_segments is None
    head.set_lexicon(None)
    assert head.lexicon is None


def test_driver_refuses_a_key_without_a_lexicon():
    from glass_amd.evaluation import inference_on_dataset
    with pytest.raises(ValueError, match="lexicon_key"):
        inference_on_dataset(None, [], lambda d: d, lexicon_key=lambda inp: 0)
