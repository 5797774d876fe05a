"""CPU: the host side of the threshold sweep (RRCScorer.sweep / TextResultWriter.sweep): transcription ids against
`pair_correct`, `scored_lines` against `to_eval_format`, the exports, the grid checks, and `ThresholdSweep` against the
result lines of `method_strings`.  The device side is tests/test_gpu_rrc_sweep.py."""
import itertools
import random
from collections import OrderedDict
from unittest import mock

import numpy as np
import pytest


def test_transcription_ids_equal_pair_correct_on_every_pair():
    """every string of length 0..4 over {a, A, !, ., #, -} on both sides, plus ground truths holding '####'"""
    from glass_amd.evaluation import rrc_score as R
    alphabet = "aA!.#-"
    assert sum(c in R.SPECIAL_CHARACTERS for c in alphabet) == 2
    strings = ["".join(t) for n in range(5) for t in itertools.product(alphabet, repeat=n)]
    assert "" in strings and "####" in strings and len(strings) == sum(6 ** n for n in range(5))
    gts = strings + ["####", "a####", "####!", "!####a.", "!a####", "a####A", "##a##", "!", "!.", ".a."]
    dets = strings
    for ws in (False, True):
        sample = R.GroundTruthSample([[0, 0, 1, 0, 1, 1]] * len(gts), list(gts), list(gts), [False] * len(gts), [False] * len(gts))
        half = len(dets) // 2
        gt_accept, det_word = R.transcription_ids([sample, R.GroundTruthSample([], [], [], [], [])], [dets[:half], dets[half:]], ws)
        assert gt_accept.dtype == np.int32 and gt_accept.shape == (len(gts), 4) and det_word.dtype == np.int32
        assert det_word.shape == (len(dets),) and int(gt_accept.min()) == -1 and (det_word != -1).all()
        got = (det_word[None, :, None] == gt_accept[:, None, :]).any(axis=2)
        d_upper = [d.upper() for d in dets]
        for g, gs in enumerate(gts):
            gu = gs.upper().replace("####", "")
            want = np.array([(gu == du) if ws else R.transcription_match(gu, du) for du in d_upper])
            assert (got[g] == want).all(), (ws, gs, [dets[i] for i in np.nonzero(got[g] != want)[0][:5]])
        # the definition itself on a sample of pairs (the loop above inlines pair_correct to stay quick)
        r = random.Random(5)
        for _ in range(20000):
            g, d = r.randrange(len(gts)), r.randrange(len(dets))
            assert bool(got[g, d]) == R.pair_correct(gts[g], dets[d], ws), (ws, gts[g], dets[d])
        assert bool(got[gts.index(""), dets.index("")]) and not got[gts.index("")].sum() > 1      # empty accepts only empty
    g, d = R.transcription_ids([], [], False)
    assert g.shape == (0, 4) and d.shape == (0,)


class _Encoder:
    character = []


def _records(seed, n_images=9):
    r = random.Random(seed)
    words = ["hello", "World!", "(STOP)", "café", "it's", "John's", "-dash-", "exit", "x", "strüeet", "OPEN", "sale."]
    scores = [0.2995, 0.3, 0.3004, 0.2994, 0.6495, 0.65, 0.6494, 0.649, 0.001, 0.0005, 0.0011, 0.9, 0.5, 1.0, 0.12345]
    out = []
    for image_id in range(1, n_images + 1):
        for _ in range(r.randint(0, 7)):
            x, y = r.randint(0, 500), r.randint(0, 400)
            out.append({"image_id": image_id, "category_id": 1, "polys": [[x, y], [x + 40.7, y], [x + 40, y + 12.2], [x, y + 12]],
                        "rec": r.choice(words), "score_text": r.choice(scores), "score_detection": r.choice(scores)})
    out.append({"image_id": n_images + 1, "category_id": 1, "polys": [[1, 1], [9, 1], [9, 5]], "rec": "low", "score_text": 0.2,
                "score_detection": 0.1})                                   # a file whose only line every threshold below rejects
    return out


def test_scored_lines_filtered_equal_to_eval_format():
    from glass_amd.evaluation import TextResultWriter
    lexicon = ["hello", "world", "stop", "cafe", "exit", "open", "sale", "john", "street"]
    pairs = {w.upper(): w for w in lexicon}
    records = _records(3)
    assert any(d["score_text"] <= 0.001 for d in records) and any(d["score_text"] == 0.2995 for d in records)
    assert any(d["score_detection"] == 0.6495 for d in records) and any(ord(c) > 127 for d in records for c in d["rec"])
    seen_empty = seen_dropped = False
    for dataset in ("icdar15", "totaltext"):
        for kw in ({}, {"word_spotting": True}, {"lexicon": lexicon, "pairs": pairs, "lexicon_type": 1},
                   {"lexicon": lexicon, "pairs": pairs, "lexicon_type": 2, "word_spotting": True}):
            w = TextResultWriter(_Encoder(), dataset=dataset, **kw)
            scored = w.scored_lines(records)
            assert all(isinstance(l, str) and isinstance(a, float) and isinstance(b, float) for ls in scored.values() for l, a, b in ls)
            n_lines = sum(len(v) for v in scored.values())
            seen_dropped |= n_lines < sum(d["score_text"] > 0.001 for d in records)              # the lexicon dropped a word
            for t, d in ((0.3, 0.65), (0.0, 0.0), (0.5, 0.0), (0.3, 0.0), (0.0, 0.65), (0.301, 0.649), (2.0, 2.0)):
                want = w.to_eval_format(records, t, d)
                got = OrderedDict((name, [l for l, st, sd in ls if not (st < t or sd < d)]) for name, ls in scored.items())
                assert list(got) == list(want) and got == want, (dataset, kw, t, d)
                seen_empty |= any(len(v) == 0 for v in want.values()) and t < 2.0
            assert w.to_eval_format(records, 0.0, 0.0) == {k: [l for l, _, _ in v] for k, v in scored.items()}
            assert any(st == 0.3 for ls in scored.values() for _, st, _ in ls)                    # 0.2995 rounded onto the threshold
    assert seen_empty and seen_dropped


def test_new_symbols_exported_and_abi_unchanged():
    from glass_amd import _lib
    from glass_amd import evaluation
    for name in ("glass_rrc_sweep", "glass_rrc_sweep_workspace_bytes"):
        assert name in _lib.EXPORTS
    assert _lib.ABI_VERSION == 8
    assert evaluation.ThresholdSweep is evaluation.rrc_score.ThresholdSweep


def test_bad_grids_raise_before_anything_is_launched():
    """`sweep` checks the grid first: the scorer here was never initialised, so touching anything else would fail too"""
    from glass_amd.evaluation import RRCScorer
    from glass_amd.evaluation.rrc_score import threshold_grid
    from glass_amd.ops import native as K
    scorer = RRCScorer.__new__(RRCScorer)
    files = {"1.txt": [("0,10,10,10,10,0,0,0,####a", 0.9, 0.9)]}
    with mock.patch.object(K, "rrc_sweep", side_effect=AssertionError("launched")), \
            mock.patch.object(K, "rrc_pair_areas", side_effect=AssertionError("launched")), \
            mock.patch.object(K, "rrc_match", side_effect=AssertionError("launched")), \
            mock.patch.object(K, "upload", side_effect=AssertionError("uploaded")):
        for ts, ds in (([], [0.5]), ([0.5], []), ([float("nan")], [0.5]), ([0.5], [0.1, float("inf")]), ([0.5, float("-inf")], [0.5]),
                       (np.linspace(0, 1, 1025), np.linspace(0, 1, 1025)), (np.zeros(2 ** 20 + 1), [0.5])):
            with pytest.raises(ValueError):
                scorer.sweep(files, ts, ds)
    t, d = threshold_grid(np.linspace(0, 1, 1024), np.linspace(0, 1, 1024))                      # exactly 2^20 is allowed
    assert t.size * d.size == 2 ** 20 and t.dtype == np.float64


def test_threshold_sweep_cells_equal_the_result_lines():
    from glass_amd.evaluation import ThresholdSweep
    from glass_amd.evaluation.rrc_score import SampleCounts, method_strings, parse_method_string
    r = random.Random(9)
    cells = [(0, 0, 0, 0, 0, 0), (0, 5, 0, 0, 5, 0), (0, 0, 4, 0, 0, 4), (3, 7, 9, 5, 7, 11), (1, 3, 3, 2, 3, 3), (0, 3, 3, 0, 2, 2)]
    cells += [(lambda m, g, d: (r.randint(0, m), g, d, m, g + r.randint(0, 3), d + r.randint(0, 3)))(r.randint(0, 40), r.randint(40, 99),
                                                                                                     r.randint(40, 99)) for _ in range(18)]
    counts = np.array(cells, dtype=np.int64).reshape(4, 6, 6)
    ts, ds = [0.1, 0.2, 0.3, 0.4], [0.0, 0.2, 0.4, 0.6, 0.8, 1.0]
    sw = ThresholdSweep(ts, ds, counts)
    for i in range(4):
        for j in range(6):
            want = OrderedDict(parse_method_string(l) for l in method_strings([SampleCounts(*counts[i, j].tolist())]))
            assert sw.results(i, j) == want and list(sw.results(i, j)) == ["E2E_RESULTS", "DETECTION_ONLY_RESULTS"]
            for task, rates in (("E2E_RESULTS", sw.e2e), ("DETECTION_ONLY_RESULTS", sw.det_only)):
                assert {k: float(v[i, j]) for k, v in rates.items()} == want[task]
    for task, rates in (("E2E_RESULTS", sw.e2e), ("DETECTION_ONLY_RESULTS", sw.det_only)):
        i, j = divmod(int(np.argmax(rates["hmean"])), 6)
        assert sw.best(task) == (ts[i], ds[j], sw.results(i, j))
    dup = ThresholdSweep([0.1, 0.1], [0.5], np.array([cells[3], cells[3]]))                       # a tie: the first cell wins
    assert dup.best()[0] == 0.1 and np.argmax(dup.e2e["hmean"]) == 0
    empty = ThresholdSweep.empty()
    assert empty.counts.shape == (0, 0, 6) and empty.e2e["hmean"].shape == (0, 0) and empty.text_thresholds.size == 0
    with pytest.raises(ValueError):
        empty.best()
    with pytest.raises(ValueError):
        sw.best("OTHER")
