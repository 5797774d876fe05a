"""CPU: lexicon loading (reference glass/evaluation/lexicon_utils.py get_lexicon, over a tmp-dir copy of the
MaskTextSpotterV3 directory layout), the host encoding of the device lexicon matcher, and its library entry."""
import os
import random

import pytest
import torch

import lexicon_cases as C


def _write(path, lines):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w", encoding="utf-8") as f:
        f.write("".join(l + "\n" for l in lines))


@pytest.fixture(scope="module")
def mtsv3(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("MaskTextSpotterV3"))
    lex = os.path.join(root, "evaluation", "lexicons")
    _write(os.path.join(lex, "totaltext", "weak_voc_new.txt"), ["Weak", "total", "  padded  "])
    _write(os.path.join(lex, "totaltext", "weak_voc_pair_list.txt"), ["WEAK Weak", "TOTAL total"])
    _write(os.path.join(lex, "ic15", "GenericVocabulary_new.txt"), ["generic", "Words"])
    # the pair-list quirk: the value starts len(key upper-cased) + 1 characters in, 'straße' -> 'STRASSE' is one longer
    _write(os.path.join(lex, "ic15", "GenericVocabulary_pair_list.txt"), ["generic Generic", "words two words", "straße Straße!"])
    _write(os.path.join(lex, "ic15", "ch4_test_vocabulary_new.txt"), ["ch4", "VOCAB"])
    _write(os.path.join(lex, "ic15", "ch4_test_vocabulary_pair_list.txt"), ["CH4 ch4", "VOCAB vocab"])
    for i in range(1, 501):
        _write(os.path.join(lex, "ic15", "new_strong_lexicon", f"new_voc_img_{i}.txt"), [f"img{i}", "shared"])
        _write(os.path.join(lex, "ic15", "new_strong_lexicon", f"pair_voc_img_{i}.txt"), [f"IMG{i} img{i}", "SHARED shared"])
    return root


def test_library_exports_lexicon_entry_and_keeps_abi_8():
    from glass_amd import _lib
    assert "glass_lexicon_match" in _lib.EXPORTS and "glass_lexicon_match_workspace_bytes" in _lib.EXPORTS
    _lib.build_library()
    L = _lib.lib()
    assert hasattr(L, "glass_lexicon_match") and L.glass_abi_version() == _lib.ABI_VERSION == 8
    assert L.glass_lexicon_match_workspace_bytes(15000) == 15000 * 8 and L.glass_lexicon_match_workspace_bytes(0) == 0


def test_load_lexicon_type_mapping_and_quirks(mtsv3):
    from glass_amd.evaluation import load_lexicon
    assert load_lexicon(mtsv3, "icdar15", 0) == (None, None)
    assert load_lexicon("/nonexistent", "anything", 0) == (None, None)           # type 0 is checked first
    weak = load_lexicon(mtsv3, "totaltext", 2)
    assert weak == (["Weak", "total", "padded"], {"WEAK": "Weak", "TOTAL": "total"})
    for t in (1, 3, 7, -1):                                                      # totaltext: the weak lexicon for any non-zero type
        assert load_lexicon(mtsv3, "totaltext", t) == weak
    lex, pairs = load_lexicon(mtsv3, "icdar15", 1)
    assert lex == ["generic", "Words"]
    assert pairs == {"GENERIC": "Generic", "WORDS": "two words", "STRASSE": "traße!"}
    assert load_lexicon(mtsv3, "icdar15", 2) == (["ch4", "VOCAB"], {"CH4": "ch4", "VOCAB": "vocab"})
    lex3, pairs3 = load_lexicon(mtsv3, "icdar15", 3)
    assert list(lex3) == list(range(1, 501)) and list(pairs3) == list(range(1, 501))
    assert lex3[1] == ["img1", "shared"] and lex3[500] == ["img500", "shared"] and pairs3[42] == {"IMG42": "img42", "SHARED": "shared"}
    for ds, t in (("icdar15", 4), ("icdar13", 1), ("textocr", 2), ("ctw1500", 3)):
        with pytest.raises(ValueError, match="No lexicon for dataset"):
            load_lexicon(mtsv3, ds, t)


def test_weighted_edit_distance_is_refused():
    from glass_amd.evaluation import LexiconMatcher
    with pytest.raises(NotImplementedError, match="lexicon_utils.py:174-180"):
        LexiconMatcher(["word"], {"WORD": "word"}, weighted_ed=True)


def test_lexicon_match_refuses_cpu_tensors():
    from glass_amd._lib import GlassLibraryError
    from glass_amd.evaluation import lexicon_layout
    from glass_amd.ops import native as K
    lay = lexicon_layout([["APPLE", "MAPLE"]])
    t = {k: torch.from_numpy(v) for k, v in lay.items() if k != "max_segment_words"}
    with pytest.raises(GlassLibraryError):
        K.lexicon_match([b"APPEL"], [0], t["word_off"], t["word_len"], t["word_sym"], t["word_index"], t["seg_off"], 2)


def test_host_encoding_upper_length_change_and_sentinel():
    from glass_amd.evaluation import encode_query, encode_word, lexicon_layout
    from glass_amd.evaluation.lexicon import SENTINEL
    assert encode_word("straße".upper()) == b"STRASSE"                           # upper() changes the length: 6 -> 7
    assert encode_word("ﬁx".upper()) == b"FIX"
    assert encode_word("café".upper()) == b"CAF" + bytes([SENTINEL])
    assert encode_word("Ωİ".upper()) == bytes([SENTINEL, SENTINEL])
    assert encode_query("Hello-1") == b"HELLO-1" and encode_query("") == b"" and encode_query("a" * 64) == b"A" * 64
    with pytest.raises(ValueError):
        encode_query("café")                                                     # non-ASCII query
    with pytest.raises(ValueError):
        encode_query("a" * 65)
    # layout: length-sorted inside each segment (stable), 16-byte aligned starts, original positions kept
    segs = [["CCC", "A", "BB", "DD", ""], [], ["straße".upper(), "X"]]
    lay = lexicon_layout(segs)
    assert lay["seg_off"].tolist() == [0, 5, 5, 7] and lay["max_segment_words"] == 5
    assert lay["word_index"].tolist() == [4, 1, 2, 3, 0, 6, 5]
    assert lay["word_len"].tolist() == [0, 1, 2, 2, 3, 1, 7]
    assert all(o % 16 == 0 for o in lay["word_off"].tolist()) and lay["word_sym"].size % 16 == 0
    sym = lay["word_sym"].tobytes()
    got = [sym[o:o + n] for o, n in zip(lay["word_off"].tolist(), lay["word_len"].tolist())]
    assert got == [b"", b"A", b"BB", b"DD", b"CCC", b"X", b"STRASSE"]


def test_sentinel_gives_the_code_point_distance():
    """only query-to-word equality enters the edit distance, so mapping every non-ASCII code point to one symbol that no
    ASCII query has changes no distance (host levenshtein on both forms)"""
    from glass_amd.evaluation import encode_word, levenshtein
    r = random.Random(3)
    for _ in range(400):
        q = "".join(r.choice("abcAB-") for _ in range(r.randint(0, 12))).upper()
        w = "".join(r.choice("abcéßΩİ") for _ in range(r.randint(0, 12))).upper()
        assert levenshtein(q, encode_word(w).decode("latin-1")) == levenshtein(q, w)


def test_random_case_golden_is_find_match_word():
    """the recorded answers of the GPU random case are what find_match_word returns (a sample re-derived here)"""
    from glass_amd.evaluation import find_match_word
    lexicon, pairs, queries = C.random_case()
    digest, expected = C.load_random_golden()
    assert digest == C.case_digest(lexicon, queries), "tests/lexicon_cases.py no longer generates the recorded case"
    assert len(expected) == len(queries) == 512 and len(lexicon) == 5000
    assert max(len(q) for q in queries) == 64 and min(len(q) for q in queries) == 0 and max(len(w) for w in lexicon) >= 65
    for i in list(range(4)) + random.Random(5).sample(range(4, 512), 8):       # "", "A" * 64, 64 random, "b", 8 more
        assert find_match_word(queries[i], lexicon, pairs) == expected[i], i
