"""GPU: glass_rrc_sweep (csrc/rrc_sweep.hip) through RRCScorer.sweep and TextResultWriter.sweep.  Expected values come from
the exact rational checker of tests/rrc_cases.py run on each cell's thresholded submission, or, where the point is
consistency with the shipped path, from `scorer.score` / `writer.evaluate` per cell (pinned to the checker by
tests/test_gpu_rrc_score.py)."""
import random
from collections import OrderedDict

import numpy as np
import pytest
import torch

import rrc_cases as C

pytestmark = pytest.mark.gpu

SCORES = (0.1, 0.3, 0.5, 0.65, 0.9)


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _scored(sub, draw):
    """{key: lines} -> {key.txt: [(line, score_text, score_detection)]} with scores from draw()"""
    return OrderedDict((k + ".txt", [(l, draw(), draw()) for l in lines]) for k, lines in sub.items())


def _cell(scored, t, d):
    """the submission of one cell, as `to_eval_format` thresholds it: {key: lines}"""
    return OrderedDict((name[:-4], [l for l, st, sd in ls if not (st < t or sd < d)]) for name, ls in scored.items())


def _parsed(result):
    from glass_amd.evaluation.rrc_score import parse_method_string
    return OrderedDict(parse_method_string(result[k]) for k in ("e2e_method", "det_only_method"))


def _assert_cell(sw, i, j, want, what):
    assert sw.results(i, j) == want, (what, i, j, sw.counts[i, j].tolist(), sw.results(i, j), want)
    for task, rates in (("E2E_RESULTS", sw.e2e), ("DETECTION_ONLY_RESULTS", sw.det_only)):
        assert {k: float(v[i, j]) for k, v in rates.items()} == want[task], (what, task, i, j)


def test_tie_case_every_cell_equals_the_exact_checker_and_runs_are_identical():
    """IoU and don't-care ratios exactly on 0.5, scores exactly on the thresholds"""
    from glass_amd.evaluation import RRCScorer
    gt, sub, _ = C.tie_case()
    r = random.Random(41)
    scored = _scored(sub, lambda: r.choice(SCORES))
    ts, ds = [0.1, 0.3, 0.5, 0.65, 0.9], [0.0, 0.3, 0.65, 0.9]
    assert any(st in ts and sd in ds for ls in scored.values() for _, st, sd in ls)
    for ws in (False, True):
        scorer = RRCScorer(gt, ws, _dev())
        sw = scorer.sweep(scored, ts, ds)
        assert sw.counts.shape == (5, 4, 6) and sw.counts.dtype == np.int64
        for i, t in enumerate(ts):
            for j, d in enumerate(ds):
                _assert_cell(sw, i, j, _parsed(C.check_score(gt, _cell(scored, t, d), ws)), ("tie", ws))
        assert len({tuple(c) for c in sw.counts.reshape(-1, 6).tolist()}) > 3                      # the thresholds matter
        assert np.array_equal(scorer.sweep(scored, ts, ds).counts, sw.counts)


def _single_image(G, D, seed):
    """one image: G ground-truth rectangles on a lattice, D detections that are copies (shifted by a pixel at most) of the
    first few ground truths with varied transcriptions and scores, so several detections compete for one ground truth and
    some fall on a don't-care one"""
    r = random.Random(seed)
    rect = lambda x, y, w, h: [x, y, x + w, y, x + w, y + h, x, y + h]
    texts = ["word", "###", "Word!", "ab", "(stop)"]
    boxes = [((g % 50) * 30, (g // 50) * 20, 24, 12) for g in range(max(G, 5))]
    gt = OrderedDict([("1", ([rect(*boxes[g]) for g in range(G)], [texts[g % len(texts)] for g in range(G)]))])
    lines = []
    for d in range(D):
        x, y, w, h = boxes[r.randrange(5)]
        P = C._clockwise(C.ring(rect(x + r.randint(0, 1), y + r.randint(0, 1), w, h)))
        lines.append((C._line(P, r.choice(["word", "WORD", "other", "Word", "stop", "STOP)"])), r.choice(SCORES), r.choice(SCORES)))
    return gt, OrderedDict([("1.txt", lines)])


def _assert_equals_score_per_cell(scorer, scored, ts, ds, what):
    sw = scorer.sweep(scored, ts, ds, validate=False)
    assert sw.counts.shape == (len(ts), len(ds), 6)
    seen = {}
    for i, t in enumerate(ts):
        for j, d in enumerate(ds):
            cell = _cell(scored, t, d)
            key = tuple(tuple(v) for v in cell.values())
            if key not in seen:                                                                  # few distinct scores: few distinct cells
                seen[key] = _parsed(scorer.score({k + ".txt": v for k, v in cell.items()}, validate=False))
            _assert_cell(sw, i, j, seen[key], what)
    return sw, len(seen)


GRID_35 = ([0.0, 0.1, 0.3, 0.5, 0.65, 0.9, 0.95], [0.05, 0.3, 0.5, 0.9, 1.0])
GRID_143 = ([round(0.08 * k, 2) for k in range(13)], [round(0.1 * k, 1) for k in range(11)])


@pytest.mark.parametrize("G,D", [(5, 0), (5, 64), (5, 65), (5, 130), (0, 7), (7, 300), (4, 600)])
def test_word_widths_and_odd_combination_counts(G, D):
    """D = 0, one full word, one bit into the second word, three words (the 4-word register tier), 300 (the 8-word tier),
    600 (masks in the workspace); G = 0; grids of 35 and 143 combinations (no multiple of the wave or of the slice of 256)"""
    from glass_amd.evaluation import RRCScorer
    gt, scored = _single_image(G, D, 100 + D)
    for ws in (False, True):
        scorer = RRCScorer(gt, ws, _dev())
        sw, n35 = _assert_equals_score_per_cell(scorer, scored, *GRID_35, (G, D, ws, 35))
        if G == 0:                               # the result lines cannot tell 0 / n from 0 / 0: without ground truth nothing
            for i, t in enumerate(GRID_35[0]):   # is don't-care, so every present detection is a care detection of both sets
                for j, d in enumerate(GRID_35[1]):
                    n = len(_cell(scored, t, d)["1"])
                    assert sw.counts[i, j].tolist() == [0, 0, n, 0, 0, n], (i, j, n, sw.counts[i, j].tolist())
        if not ws:
            _assert_equals_score_per_cell(scorer, scored, *GRID_143, (G, D, ws, 143))
        assert n35 > 5 or D == 0


def test_rows_above_the_lds_capacity_are_read_from_the_workspace():
    """G * ceil(D / 64) = 1366 * 3 = 4098 row words, two more than GLASS_RRC_SWEEP_LDS_WORDS = 4096: the image's rows are
    read from global memory; one image below the boundary shares the chunk"""
    from glass_amd.evaluation import RRCScorer
    from glass_amd.ops import native as K
    assert K.RRC_SWEEP_LDS_WORDS == 4096
    gt, scored = _single_image(1366, 130, 77)
    gt2, scored2 = _single_image(1365, 130, 78)
    gt["2"], scored["2.txt"] = gt2["1"], scored2["1.txt"]
    scorer = RRCScorer(gt, False, _dev())
    _assert_equals_score_per_cell(scorer, scored, [0.1, 0.5, 0.9], [0.3, 0.65], "spill")


def test_many_images_chunking_and_threshold_order():
    from glass_amd.evaluation import RRCScorer
    from glass_amd.evaluation.rrc_score import parse_detection_line
    gold = C.load_decisions_golden()
    gt_all, sub_all, planted, _ = C.decisions_case(redraws=gold["redraws"])
    keys = planted + [k for k in gt_all if k not in planted][::11]
    gt = OrderedDict((k, gt_all[k]) for k in keys)
    sub = OrderedDict((k, sub_all[k]) for k in keys if k in sub_all)
    assert max(len(v) for v in sub.values()) == 101 and len(keys) > 20
    r = random.Random(2026)
    scored = _scored(sub, lambda: round(r.random(), 3))
    ts, ds = [0.2, 0.4, 0.6, 0.8], [0.1, 0.3, 0.5, 0.7]
    # the exact areas once; a cell's geometry is a selection of detection columns
    full = {}
    for k, lines in sub.items():
        full[k] = C.exact_image([C.ring(p) for p in gt[k][0]], [C.ring(parse_detection_line(l)[0]) for l in lines])
    for ws in (False, True):
        scorer = RRCScorer(gt, ws, _dev())
        sw = scorer.sweep(scored, ts, ds)
        for i, t in enumerate(ts):
            for j, d in enumerate(ds):
                geometry = {}
                for k, ls in scored.items():
                    sel = [n for n, (_, st, sd) in enumerate(ls) if not (st < t or sd < d)]
                    ag, ad, inter = full[k[:-4]]
                    geometry[k[:-4]] = (ag, [ad[n] for n in sel], [[row[n] for n in sel] for row in inter])
                _assert_cell(sw, i, j, _parsed(C.check_score(gt, _cell(scored, t, d), ws, geometry)), ("many", ws))
        assert np.array_equal(RRCScorer(gt, ws, _dev(), chunk_images=1).sweep(scored, ts, ds).counts, sw.counts)
        assert np.array_equal(RRCScorer(gt, ws, _dev(), workspace_cap_bytes=8 * 150).sweep(scored, ts, ds).counts, sw.counts)
        ts2, ds2 = [0.6, 0.2, 0.6], [0.7, 0.7, 0.3, 0.1]                                        # unsorted, duplicated
        sw2 = scorer.sweep(scored, ts2, ds2)
        for i, t in enumerate(ts2):
            for j, d in enumerate(ds2):
                assert np.array_equal(sw2.counts[i, j], sw.counts[ts.index(t), ds.index(d)])
    assert sw.counts[0, 0, 2] > sw.counts[3, 3, 2] > 0                                            # fewer detections stay


# ------------------------------------------------------------------------------------------------ through the writer

def _encoder():
    from glass_amd.config import get_glass_cfg
    from glass_amd.modeling.recognition.text_encoder import TextEncoder
    cfg = get_glass_cfg()
    cfg.MODEL.ROI_RECOGNIZER_HEAD.NAME = "RecognizerRCNNHeadV3"
    cfg.MODEL.ROI_RECOGNIZER_HEAD.MAX_WORD_LENGTH = 25
    return TextEncoder(cfg)


def _instances(enc, boxes, words, scores, peaks, masks=None):
    """synthetic model output: rotated boxes, text probabilities that decode to `words` with confidence set by `peaks`"""
    from glass_amd.structures.core import Instances, RotatedBoxes
    inst = Instances((480, 640))
    b = torch.tensor(boxes, dtype=torch.float32).reshape(-1, 5)
    inst.pred_boxes, inst.pred_rboxes = RotatedBoxes(b.clone()), RotatedBoxes(b.clone())
    inst.scores = torch.tensor(scores, dtype=torch.float32)
    inst.pred_classes = torch.zeros(len(b), dtype=torch.int64)
    labels = enc.encode(words)[:, 1:]
    prob = torch.full((len(words), labels.shape[1], len(enc.character)), 0.001)
    prob.scatter_(2, labels.unsqueeze(-1), torch.tensor(peaks, dtype=torch.float32).reshape(-1, 1, 1).expand(-1, labels.shape[1], 1).clone())
    inst.pred_text_prob = prob
    if masks is not None:
        inst.pred_masks = torch.from_numpy(masks)
    return inst


_WORDS = ["hello", "World", "STOP", "cafe", "exit", "street", "OPEN", "sale", "John", "market"]


def _writer_case(dataset, seed, n_images, with_masks):
    """(encoder, inputs, outputs, gt): images named so that the writer's sort gives ids 1..n (icdar) / 0..n-1 (totaltext)"""
    from glass_amd.evaluation import rotated_boxes_to_polygons
    r = random.Random(seed)
    enc = _encoder()
    inputs, outputs, gt = [], [], OrderedDict()
    for i in range(n_images):
        n = r.randint(0, 6)
        boxes = [[r.randint(80, 560), r.randint(60, 420), r.randint(30, 120), r.randint(12, 40), r.choice([0, 0, 15, -30, 90])] for _ in range(n)]
        words = [r.choice(_WORDS) for _ in range(n)]
        masks = None
        if with_masks:
            masks = np.zeros((n, 480, 640), dtype=bool)
            for k, (cx, cy, w, h, _) in enumerate(boxes):                       # an L-shaped region with a staircase edge
                masks[k, cy - h // 2:cy + h // 2, cx - w // 2:cx + w // 2] = True
                masks[k, cy - h // 2:cy, cx:cx + w // 2] = False
                for t in range(0, w // 2 - 2, 4):
                    masks[k, cy + h // 2:cy + h // 2 + 1 + t // 4, cx - w // 2 + t:cx - w // 2 + t + 2] = True
        inputs.append({"file_name": f"img_{i + 1}.jpg" if dataset.startswith("icdar") else f"{i:07d}.jpg"})
        outputs.append({"instances": _instances(enc, boxes, [w if r.random() < 0.8 else w + "x" for w in words],
                                                [r.choice([0.9, 0.7, 0.45]) for _ in range(n)],
                                                [r.choice([0.95, 0.8, 0.6]) for _ in range(n)], masks)})
        rings, texts = [], []
        for (cx, cy, w, h, a), word in zip(boxes, words):
            if r.random() < 0.15:
                continue
            q = rotated_boxes_to_polygons(np.array([[cx + r.randint(-3, 3), cy + r.randint(-2, 2), w, h, a]], dtype=np.float64))[0]
            rings.append([int(v) for p in q for v in p])
            texts.append(r.choice(["###", word + "!", word + "'s", word, word, word]))
        if r.random() < 0.3:
            rings.append([5, 5, 60, 5, 60, 25, 5, 25])
            texts.append(r.choice(["ab", "missed", "###"]))
        gt[str(i + 1) if dataset.startswith("icdar") else f"{i:07d}"] = (rings, texts)
    return enc, inputs, outputs, gt


def _sweep_equals_evaluate(writer, scorer, ts, ds):
    sw = writer.sweep(scorer, ts, ds)
    cells = [[writer.evaluate(scorer, t, d) for d in ds] for t in ts]
    for i in range(len(ts)):
        for j in range(len(ds)):
            assert sw.results(i, j) == cells[i][j], (i, j, sw.results(i, j), cells[i][j])
    for task in ("E2E_RESULTS", "DETECTION_ONLY_RESULTS"):
        flat = [cells[i][j][task]["hmean"] for i in range(len(ts)) for j in range(len(ds))]
        i, j = divmod(flat.index(max(flat)), len(ds))                                            # index(): the first maximum
        assert sw.best(task) == (ts[i], ds[j], cells[i][j])
    assert len({tuple(c) for c in sw.counts.reshape(-1, 6).tolist()}) > 2                          # the cells differ
    return sw


def test_writer_sweep_equals_evaluate_icdar15_with_device_lexicon():
    from glass_amd.evaluation import LexiconMatcher, RRCScorer, ThresholdSweep, TextResultWriter
    dev = _dev()
    enc, inputs, outputs, gt = _writer_case("icdar15", 11, 24, False)
    lexicon = _WORDS + ["hallo", "exits"]
    pairs = {w.upper(): w for w in lexicon}
    ts, ds = [0.0, 0.3, 0.6], [0.0, 0.5, 0.8]
    for ws in (False, True):
        w = TextResultWriter(enc, dataset="icdar15", word_spotting=ws, lexicon=lexicon, pairs=pairs, lexicon_type=1,
                             matcher=LexiconMatcher(lexicon, pairs, device=dev))
        empty = w.sweep(None, ts, ds)                                                             # no predictions: the empty sweep
        assert isinstance(empty, ThresholdSweep) and empty.counts.shape == (0, 0, 6) and empty.e2e["hmean"].size == 0
        with pytest.raises(ValueError):
            empty.best()
        w.process(inputs, outputs)
        sw = _sweep_equals_evaluate(w, RRCScorer(gt, ws, dev), ts, ds)
        assert 0 < sw.e2e["hmean"].max() < 1


def test_writer_sweep_equals_evaluate_totaltext_many_point_rings():
    from glass_amd.evaluation import RRCScorer, TextResultWriter, masks_to_polygons
    dev = _dev()
    enc, inputs, outputs, gt = _writer_case("totaltext", 12, 10, True)
    w = TextResultWriter(enc, dataset="totaltext", masks_to_polygons=masks_to_polygons)
    w.process(inputs, outputs)
    assert max(l.count(",") for ls in w.scored_lines(w.coco_results()).values() for l, _, _ in ls) > 40   # rings of > 20 points
    sw = _sweep_equals_evaluate(w, RRCScorer(gt, False, dev), [0.0, 0.3, 0.6], [0.0, 0.5, 0.8])
    assert sw.det_only["hmean"].max() > 0
