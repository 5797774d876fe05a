"""GPU: glass_lexicon_match_weighted (csrc/lexicon_weighted.hip) through WeightedLexiconMatcher / TextResultWriter, compared
exactly - the word with ==, the distance through float.hex() - with the reference's recorded answers
(tests/golden/lexicon_weighted.json) where there are any, otherwise with the host `find_match_word_weighted`."""
import io
import random
import zipfile
from unittest import mock

import pytest
import torch

import lexicon_cases
import lexicon_weighted_cases as C

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _device_answers(case, **kw):
    from glass_amd.evaluation import WeightedLexiconMatcher
    lexicon, pairs, queries, scores, enc = case
    m = WeightedLexiconMatcher(lexicon, pairs, enc, device=_dev(), **kw)
    if isinstance(lexicon, dict):
        got = m.match([q for q, _ in queries], [img for _, img in queries], scores=scores)
    else:
        got = m.match(queries, scores=scores)
    return [C.as_hex(g) for g in got]


def _host_answers(case):
    from glass_amd.evaluation import find_match_word_weighted
    return [C.as_hex(find_match_word_weighted(rec, lex, pairs, sc, case[4])) for rec, lex, pairs, sc in C.host_queries(case)]


def _assert_same(case, got, want):
    bad = [(i, case[2][i], got[i], want[i]) for i in range(len(want)) if got[i] != want[i]]
    assert len(got) == len(want) and not bad, f"{len(bad)} of {len(want)} differ, first: {bad[:3]}"


@pytest.mark.parametrize("name", sorted(C.GOLDEN_CASES))
def test_recorded_cases_equal_the_reference(name):
    case = C.GOLDEN_CASES[name]()
    digest, expected = C.load_golden()[name]
    assert digest == C.case_digest(case[0], case[2], case[3])
    got = _device_answers(case)
    _assert_same(case, got, expected)
    if name == "ties":
        by_query = dict(zip(case[2], got))
        assert {q: by_query[q][0] for q in C.TIES_WINNERS} == C.TIES_WINNERS      # first in file order, across workgroups
        assert by_query["tiger"][1] == (1.0).hex() and by_query["world"][1] == (0.0).hex()
    if name == "far":
        assert got[0][0] != "" and float.fromhex(got[0][1]) < 100.0               # dist_min_pre stayed 100, a match was found
        assert got[1] == ("", (100.0).hex())                                      # the "none found" segment


@pytest.mark.parametrize("name", ["crowd", "segments", "wide"])
def test_other_cases_equal_the_host_path(name):
    case = {"crowd": C.crowd_case, "segments": C.segments_case, "wide": C.wide_case}[name]()
    got = _device_answers(case)
    _assert_same(case, got, _host_answers(case))
    if name == "segments":
        queries = case[2]
        assert queries[0][1] == 7 and got[0] == ("", (100.0).hex())               # the empty segment
        assert got[1] == ("9:", (3.0).hex()) and got[2] == ("9:", (0.0).hex())    # only the empty word
        assert got[3][0].startswith("21:") and got[4] == ("", (100.0).hex())
    if name == "crowd":
        from glass_amd.evaluation import levenshtein
        units = [levenshtein("A", w.upper()) for w in case[0]]
        assert sum(u <= min(units) + 2 for u in units) > 1024                     # candidates of the query 'a'


def test_small_table_cap_chunks_the_queries_and_changes_nothing():
    case = C.crowd_case()
    assert _device_answers(case, table_cap_bytes=4096) == _device_answers(case)   # 1-2 queries per launch


def test_two_runs_are_bit_identical():
    case = C.random_case()
    assert _device_answers(case) == _device_answers(case)


def test_status_word_raises_key_error_only_for_a_candidate():
    from glass_amd.evaluation import WeightedLexiconMatcher, find_match_word_weighted
    lexicon, pairs, queries, scores, enc = C.no_unk_case()
    m = WeightedLexiconMatcher(lexicon, pairs, enc, device=_dev())
    with pytest.raises(KeyError):
        find_match_word_weighted(queries[0], lexicon, pairs, scores[0], enc)
    with pytest.raises(KeyError):
        m.match(queries[:1], scores=scores[:1])
    with pytest.raises(KeyError):
        m.match(queries, scores=scores)
    got = m.match(queries[1:], scores=scores[1:])                                 # 'CAFÉ' is in the lexicon but no candidate
    assert got == [find_match_word_weighted(queries[1], lexicon, pairs, scores[1], enc)] and got[0][0] == "orange"
    assert m.match([""], scores=[scores[0]]) == [find_match_word_weighted("", lexicon, pairs, scores[0], enc)]


def _records(seed, enc, n_images, lexicon_words):
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
        ascii_rec = "".join(c for c in rec if ord(c) < 128)
        x, y, bw, bh = r.randint(0, 600), r.randint(0, 400), r.randint(5, 80), r.randint(5, 30)
        recs.append({"image_id": img, "polys": [[x, y], [x + bw, y], [x + bw, y + bh], [x, y + bh]], "rec": rec,
                     "score_text": r.choice([0.0005, r.random()]), "score_detection": r.random(),
                     "character_probs": C.score_table(r, ascii_rec, enc, 26, zero=0.6)})
    return recs


def test_writer_with_weighted_matcher_is_byte_identical_to_host_writer():
    from glass_amd.evaluation import TextResultWriter, WeightedLexiconMatcher
    r = random.Random(23)
    enc = C.Encoder()
    words = lambda n: ["".join(r.choice("abcdefghijklmnopéß'") for _ in range(r.randint(2, 10))).capitalize() for _ in range(n)]
    generic, weak = words(1500), words(200)
    strong = {i: words(40) for i in range(1, 21)}
    cases = ((1, generic, {w.upper(): w for w in generic}), (2, weak, {w.upper(): w for w in weak}),
             (3, strong, {i: {w.upper(): w for w in ws} for i, ws in strong.items()}))
    for lexicon_type, lexicon, pairs in cases:
        recs = _records(lexicon_type, enc, 20, lexicon)
        kw = dict(dataset="icdar15", lexicon=lexicon, pairs=pairs, lexicon_type=lexicon_type, edit_distance_thr=1.5, weighted_ed=True)
        host = TextResultWriter(enc, **kw)
        dev = TextResultWriter(enc, matcher=WeightedLexiconMatcher(lexicon, pairs, enc, device=_dev()), **kw)
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


def test_unit_cost_matcher_is_unchanged_by_the_shared_header():
    from glass_amd.evaluation import LexiconMatcher
    lexicon, pairs, queries = lexicon_cases.random_case()
    digest, expected = lexicon_cases.load_random_golden()
    assert digest == lexicon_cases.case_digest(lexicon, queries)
    assert LexiconMatcher(lexicon, pairs, device=_dev()).match(queries) == expected
