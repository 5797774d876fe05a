"""CPU: the weighted lexicon match (reference glass/evaluation/lexicon_utils.py:26-48, :136-182) on the host -
`find_match_word_weighted` against the reference's recorded answers, the cost tables the device path uploads, its
pre-launch errors, the library entry and the writer's `weighted_ed` switch."""
import os
import random
import re

import numpy as np
import pytest

import lexicon_weighted_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_weighted_entry_and_keeps_abi_8():
    from glass_amd import _lib
    names = ("glass_lexicon_match_weighted", "glass_lexicon_match_weighted_workspace_bytes")
    assert all(n in _lib.EXPORTS for n in names)
    with open(os.path.join(ROOT, "include", "glass_hip.h")) as f:
        header = f.read()
    for n in names:
        assert re.search(r"\b" + n + r"\(", header), n
    _lib.build_library()
    L = _lib.lib()
    assert all(hasattr(L, n) for n in names) and L.glass_abi_version() == _lib.ABI_VERSION == 8
    ws = L.glass_lexicon_match_weighted_workspace_bytes
    assert ws(0, 90_000) == 0
    assert ws(15_000, 90_000) == 15_000 * (8 + 8 + 4)              # one slice per query: unit key + (distance, index) partial
    assert ws(5, 12_000) == 5 * 8 + 5 * 12 * 8 + 5 * 12 * 4        # few queries: one slice per 1,024-word chunk
    assert ws(3, 0) == 3 * 8 and ws(3, 100) % 8 == 0


def test_golden_digest_matches_the_generated_cases():
    golden = C.load_golden()
    for name, make in C.GOLDEN_CASES.items():
        lexicon, pairs, queries, scores, _ = make()
        assert golden[name][0] == C.case_digest(lexicon, queries, scores), f"{name}_case no longer generates the recorded inputs"
        assert len(golden[name][1]) == len(queries)
    lexicon, _, queries, scores, _ = C.random_case()
    assert len(lexicon) == 4000 and len(queries) == 256
    assert min(map(len, queries)) == 0 and max(map(len, queries)) == 64 and max(map(len, scores)) == 65
    assert any(not w.isascii() for w in lexicon) and len(set(w.upper() for w in lexicon)) < len(lexicon)


def test_find_match_word_weighted_equals_the_reference_on_a_sample():
    """12 queries: the empty one, 64-symbol ones, the three planted ties, both far_case queries and 4 more random ones"""
    from glass_amd.evaluation import find_match_word_weighted
    golden = C.load_golden()
    sample = [("random", i) for i in [0, 1, 3] + random.Random(5).sample(range(4, 256), 4)]
    sample += [("ties", 0), ("ties", 1), ("ties", 2), ("far", 0), ("far", 1)]
    assert len(sample) == 12
    for name, i in sample:
        case = C.GOLDEN_CASES[name]()
        rec, lexicon, pairs, scores = C.host_queries(case)[i]
        got = C.as_hex(find_match_word_weighted(rec, lexicon, pairs, scores, case[4]))
        assert got == golden[name][1][i], (name, i, rec)
    ties = dict(zip(C.ties_case()[2], golden["ties"][1]))
    assert {q: ties[q][0] for q in C.TIES_WINNERS} == C.TIES_WINNERS
    assert ties["tiger"][1] == (1.0).hex() and ties["world"][1] == (0.0).hex()
    assert golden["far"][1][0][0] != "" and float.fromhex(golden["far"][1][0][1]) < 100 and golden["far"][1][1] == ("", (100.0).hex())


def _dp_from_tables(rec, word, dele, ins, rep, sym_class):
    """what the kernel computes: the DP over the uploaded tables, adding and taking minima only"""
    from glass_amd.evaluation import encode_word
    q, w = rec.upper().encode("ascii"), encode_word(word)
    prev = [float(j) for j in range(len(q) + 1)]
    for i in range(1, len(w) + 1):
        cur = [float(i)]
        for j in range(1, len(q) + 1):
            r = 0.0 if q[j - 1] == w[i - 1] else float(rep[j - 1][sym_class[w[i - 1]]])
            cur.append(min(min(prev[j] + float(ins[j - 1]), cur[j - 1] + float(dele[j - 1])), prev[j - 1] + r))
        prev = cur
    return prev[len(q)]


def test_cost_tables_reproduce_weighted_edit_distance_exactly():
    from glass_amd.evaluation import symbol_classes, weighted_cost_tables, weighted_edit_distance
    lexicon, _, queries, scores, enc = C.random_case()
    sym_class, classes = symbol_classes(enc)
    assert sym_class.dtype == np.uint8 and sym_class.shape == (256,) and len(classes) == 96      # 95 characters + [UNK]
    assert sym_class[0x80] == classes.index(enc.dict["[UNK]"]) and sym_class[ord("\t")] == sym_class[0x80]
    r = random.Random(29)
    for _ in range(200):
        k = r.randrange(len(queries))
        rec, word = queries[k], r.choice(lexicon).upper()
        dele, ins, rep = weighted_cost_tables(rec, scores[k], enc, classes)
        assert dele.dtype == ins.dtype == rep.dtype == np.float64 and rep.shape == (len(rec), 96)
        want = weighted_edit_distance(rec, word, scores[k], enc)
        assert float(_dp_from_tables(rec, word, dele, ins, rep, sym_class)).hex() == float(want).hex(), (rec, word)


class _NoLaunch:
    """a WeightedLexiconMatcher without a device: the pre-launch checks must raise before `tensors` is touched"""

    def __new__(cls, enc):
        from glass_amd.evaluation import WeightedLexiconMatcher, symbol_classes

        class Lexicon:
            device = "cpu"
            upper = ["WORD"]
            max_segment_words = 1

            def segment(self, key):
                return {None: 0}[key]

            @property
            def tensors(self):
                raise AssertionError("a launch was prepared")

        m = object.__new__(WeightedLexiconMatcher)
        m.lexicon, m.pairs, m.text_encoder, m.table_cap_bytes = Lexicon(), {"WORD": "word"}, enc, 1 << 20
        m.classes = symbol_classes(enc)[1]
        return m


def test_pre_launch_errors():
    enc = C.Encoder()
    m = _NoLaunch(enc)
    good = C.score_table(random.Random(1), "word", enc, 26)
    with pytest.raises(ValueError, match="score tables"):
        m.match(["word", "ward"], scores=[good])
    with pytest.raises(IndexError):
        m.match(["word"], scores=[good[:3]])                         # 4 characters, 3 score rows
    for bad in (float("nan"), float("inf"), -0.25):
        t = [list(row) for row in good]
        t[2][5] = bad
        with pytest.raises(ValueError, match="negative or non-finite"):
            m.match(["word"], scores=[t])
    t = [list(row) for row in good]
    t[1][enc.char_encode("o")] = 0.0
    with pytest.raises(ZeroDivisionError):
        m.match(["word"], scores=[t])
    with pytest.raises(ValueError, match="ASCII"):
        m.match(["wörd"], scores=[good])
    with pytest.raises(ValueError):
        m.match(["w" * 65], scores=[C.score_table(random.Random(1), "w" * 65, enc, 66)])
    with pytest.raises(KeyError):
        _NoLaunch(C.Encoder(unk=False)).match(["wo\trd"], scores=[good + good])    # a query character without a class
    with pytest.raises(TypeError):
        m.match(["word"])
    with pytest.raises(AssertionError, match="a launch was prepared"):
        m.match(["word"], scores=[good])                             # valid input does reach the launch


def test_character_set_must_be_ascii():
    from glass_amd.evaluation import symbol_classes
    with pytest.raises(ValueError, match="ASCII"):
        symbol_classes(C.Encoder(C.CHARSET + "é"))
    table, classes = symbol_classes(C.Encoder(unk=False))
    assert len(classes) == 95 and table[0x80] == 0xFF and table[ord("\t")] == 0xFF and table[ord("a")] != 0xFF


def test_unit_cost_matcher_still_refuses_weighted_ed():
    from glass_amd.evaluation import LexiconMatcher
    with pytest.raises(NotImplementedError, match="lexicon_utils.py:174-180") as e:
        LexiconMatcher(["word"], {"WORD": "word"}, weighted_ed=True)
    assert "WeightedLexiconMatcher" in str(e.value) and "no return" not in str(e.value)


def _records(r, enc, lexicon_words, n=60, n_images=6):
    recs = []
    for _ in range(n):
        img = r.randint(1, n_images)
        w = r.choice(lexicon_words[img] if isinstance(lexicon_words, dict) else lexicon_words)
        u = r.random()
        if u < 0.35:
            rec = w
        elif u < 0.7:
            rec = "".join(c if r.random() > 0.2 else r.choice("xyzé") for c in w.lower())
        else:
            rec = "".join(r.choice("abcdefghijklmnop'!") for _ in range(r.randint(1, 12)))
        ascii_rec = "".join(c for c in rec if ord(c) < 128)
        x, y = r.randint(0, 600), r.randint(0, 400)
        recs.append({"image_id": img, "polys": [[x, y], [x + 30, y], [x + 30, y + 10], [x, y + 10]], "rec": rec,
                     "score_text": r.choice([0.0005, r.random()]), "score_detection": r.random(),
                     "character_probs": C.score_table(r, ascii_rec, enc, 26, zero=0.6)})
    return recs


def test_host_writer_with_weighted_ed_drops_and_replaces_by_the_rule():
    from glass_amd.evaluation import TextResultWriter, find_match_word_weighted, match_transcript
    r = random.Random(31)
    enc = C.Encoder()
    words = ["".join(r.choice("abcdefghijklmnop") for _ in range(r.randint(2, 9))).capitalize() for _ in range(120)]
    pairs = {w.upper(): w for w in words}
    recs = _records(r, enc, words)
    for lexicon_type in (1, 2):
        kw = dict(dataset="icdar15", lexicon=words, pairs=pairs, lexicon_type=lexicon_type, edit_distance_thr=1.5)
        files = TextResultWriter(enc, weighted_ed=True, **kw).to_eval_format(recs, 0.0, 0.0)
        want = {}
        for d in recs:
            if not d["score_text"] > 0.001:
                continue
            ass = "".join(c for c in d["rec"] if ord(c) < 128)
            word, dist = find_match_word_weighted(ass, words, pairs, d["character_probs"], enc)
            want.setdefault(f"{d['image_id']}.txt", [])
            if dist < 1.5 or lexicon_type == 1:
                cors = ",".join(f"{p[0]},{p[1]}" for p in d["polys"])
                want[f"{d['image_id']}.txt"].append(cors + ",####" + match_transcript(word, False))
        assert files == want
        plain = TextResultWriter(enc, **kw).to_eval_format(recs, 0.0, 0.0)
        if lexicon_type == 2:
            assert files != plain                                    # the weighted rule keeps other words than the unit rule
            assert 0 < sum(map(len, files.values())) < sum(d["score_text"] > 0.001 for d in recs)
    with pytest.raises(ValueError):
        TextResultWriter(enc, weighted_ed=True, matcher=object(), lexicon=words, pairs=pairs, lexicon_type=2)
