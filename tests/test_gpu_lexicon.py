"""GPU: glass_lexicon_match (csrc/lexicon.hip) through LexiconMatcher / TextResultWriter, compared exactly, as
(word, distance), with the host `find_match_word` (reference lexicon_utils.py:4-28)."""
import io
import random
import zipfile
from unittest import mock

import pytest
import torch

import lexicon_cases as C

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def test_random_lexicon_matches_find_match_word():
    from glass_amd.evaluation import LexiconMatcher
    lexicon, pairs, queries = C.random_case()
    digest, expected = C.load_random_golden()                  # find_match_word's answers (tests/test_lexicon.py re-derives a sample)
    assert digest == C.case_digest(lexicon, queries)
    got = LexiconMatcher(lexicon, pairs, device=_dev()).match(queries)
    bad = [(i, queries[i], got[i], expected[i]) for i in range(len(queries)) if got[i] != expected[i]]
    assert not bad, f"{len(bad)} of {len(queries)} differ, first: {bad[:3]}"


def test_ties_first_in_file_order_wins_across_workgroups():
    from glass_amd.evaluation import LexiconMatcher, find_match_word
    lexicon, pairs, queries = C.ties_case()
    got = LexiconMatcher(lexicon, pairs, device=_dev()).match(queries)
    for q, g in zip(queries, got):
        assert g == find_match_word(q, lexicon, pairs), q
    assert got[0] == ("helloq", 1) and got[1] == ("helloq", 1)   # planted at 60 123, longer than the later ties


def test_per_image_segments_empty_and_far():
    from glass_amd.evaluation import LexiconMatcher, find_match_word
    lexicons, pairs, queries = C.segments_case()
    m = LexiconMatcher(lexicons, pairs, device=_dev())
    got = m.match([q for q, _ in queries], [img for _, img in queries])
    for (q, img), g in zip(queries, got):
        assert g == find_match_word(q, lexicons[img], pairs[img]), (q, img)
    assert got[0] == ("", 100) and got[1] == ("", 100) and got[2] == ("", 100)
    assert sum(d == 0 for _, d in got) > 50
    with pytest.raises(KeyError):
        m.match(["word"], [51])                                  # no such image, as lexicon[51] in the reference


def _records(seed, n_images, lexicon_words):
    r = random.Random(seed)
    recs = []
    for k in range(160):
        img = r.randint(1, n_images)
        w = r.choice(lexicon_words[img] if isinstance(lexicon_words, dict) else lexicon_words)
        u = r.random()
        if u < 0.35:
            rec = w
        elif u < 0.7:
            rec = "".join(c if r.random() > 0.15 else r.choice("xyzé") for c in w.lower())   # near hit, non-ASCII stripped
        else:
            rec = "".join(r.choice("abcdefghijklmnop'!") for _ in range(r.randint(1, 12)))
        x, y, bw, bh = r.randint(0, 600), r.randint(0, 400), r.randint(5, 80), r.randint(5, 30)
        recs.append({"image_id": img, "polys": [[x, y], [x + bw, y], [x + bw, y + bh], [x, y + bh]], "rec": rec,
                     "score_text": r.choice([0.0005, r.random()]), "score_detection": r.random()})
    return recs


def test_writer_with_matcher_is_byte_identical_to_host_writer():
    from glass_amd.evaluation import LexiconMatcher, TextResultWriter
    r = random.Random(23)
    words = lambda n: ["".join(r.choice("abcdefghijklmnopéß'") for _ in range(r.randint(2, 10))).capitalize() for _ in range(n)]
    generic, weak = words(1500), words(200)
    strong = {i: words(40) for i in range(1, 21)}
    cases = ((1, generic, {w.upper(): w for w in generic}), (2, weak, {w.upper(): w for w in weak}),
             (3, strong, {i: {w.upper(): w for w in ws} for i, ws in strong.items()}))
    for lexicon_type, lexicon, pairs in cases:
        recs = _records(lexicon_type, 20, lexicon)
        kw = dict(dataset="icdar15", lexicon=lexicon, pairs=pairs, lexicon_type=lexicon_type, edit_distance_thr=1.5)
        host = TextResultWriter(None, **kw)
        dev = TextResultWriter(None, matcher=LexiconMatcher(lexicon, pairs, device=_dev()), **kw)
        for th in ((0.5, 0.0), (0.2, 0.4)):
            fh, fd = host.to_eval_format(recs, *th), dev.to_eval_format(recs, *th)
            assert fd == fh, (lexicon_type, th)
            with mock.patch("time.time", return_value=1_700_000_000.0):          # zip member timestamps
                zh, zd = host.det_zip(fh), dev.det_zip(fd)
            assert zd == zh, (lexicon_type, th)
        lines = [l for ls in fh.values() for l in ls]
        assert lines and zipfile.ZipFile(io.BytesIO(zh)).namelist()
        if lexicon_type != 1:
            assert len(lines) < sum(r["score_text"] > 0.001 for r in recs)       # some words had no lexicon match


def test_queries_longer_than_64_raise():
    from glass_amd.evaluation import LexiconMatcher
    from glass_amd.evaluation.lexicon import DeviceLexicon
    from glass_amd.ops import native as K
    m = LexiconMatcher(["word"], {"WORD": "word"}, device=_dev())
    assert m.match(["w" * 64]) == [("word", 63)]              # one W kept, 63 substituted or deleted
    with pytest.raises(ValueError):
        m.match(["w" * 65])
    with pytest.raises(ValueError):
        m.match(["wörd"])
    t = DeviceLexicon(["word"], _dev()).tensors
    with pytest.raises(ValueError):
        K.lexicon_match([b"W" * 65], [0], t["word_off"], t["word_len"], t["word_sym"], t["word_index"], t["seg_off"], 1)
