"""GPU: glass_rrc_pair_areas / glass_rrc_match (csrc/rrc_score.hip) through ops.native, RRCScorer and
TextResultWriter.evaluate, against the exact checker of tests/rrc_cases.py (rational arithmetic, slab decomposition).
The reference scorer is never run: its Polygon / Levenshtein C packages are absent."""
import io
import zipfile
from collections import OrderedDict
from unittest import mock

import numpy as np
import pytest
import torch

import rrc_cases as C

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _pairs_layout(pairs):
    """each (A, B) as one image with one GT ring and one detection ring"""
    from glass_amd.ops import native as K
    dev = _dev()
    rings = [A for _, A, _ in pairs] + [B for _, _, B in pairs]
    pts = np.array([p for r in rings for p in r], dtype=np.int32).reshape(-1, 2)
    off = np.concatenate([[0], np.cumsum([len(r) for r in rings])])
    n = len(pairs)
    up = lambda a, t: K.upload(np.asarray(a), t, dev)
    return (up(pts, torch.int32), up(off, torch.int32), up(np.arange(n + 1), torch.int32), up(n + np.arange(n + 1), torch.int32),
            up(np.arange(n + 1), torch.int64), n)


def test_areas_exact_and_intersections_within_the_derived_bound(capsys):
    """area == |shoelace| / 2 exactly; |inter - exact| <= BOUND_C * 2^-53 * ne * nf * W * H (derivation: tests/rrc_cases.py,
    'error bound').  Prints the largest error / bound ratio."""
    from glass_amd.ops import native as K
    pairs = C.area_pairs()
    assert len(pairs) > 200 and max(len(A) for _, A, _ in pairs) >= 64
    layout = _pairs_layout(pairs)
    area, inter = K.rrc_pair_areas(*layout)
    area2, inter2 = K.rrc_pair_areas(*layout)
    assert torch.equal(inter, inter2) and torch.equal(area, area2)           # bit-identical runs
    area, inter = area.cpu().numpy(), inter.cpu().numpy()
    n, worst = len(pairs), (0.0, "")
    for k, (name, A, B) in enumerate(pairs):
        assert area[k] == float(C.exact_area(A)) and area[n + k] == float(C.exact_area(B)), name   # halves of integers < 2^53: exact
        exact = C.exact_intersection(A, B)
        err, bound = abs(float(inter[k] - exact)) if inter[k] != exact else 0.0, C.inter_bound(A, B)
        worst = max(worst, (err / bound, name))
        assert err <= bound, (name, float(exact), inter[k], err, bound)
        if exact == 0 and name in ("disjoint", "touching boxes"):
            assert inter[k] == 0.0                                           # bounding boxes do not overlap: exactly 0
    with capsys.disabled():
        print(f"\nrrc_pair_areas: {n} pairs, largest |error| / bound = {worst[0]:.3e} ({worst[1]})")


def test_pair_order_and_grid_do_not_change_a_result():
    """the same pair gives the same bits wherever it sits in the wave and whoever its neighbours are"""
    from glass_amd.ops import native as K
    pairs = C.area_pairs()
    _, inter = K.rrc_pair_areas(*_pairs_layout(pairs))
    perm = list(range(len(pairs)))[::-1]
    _, inter_r = K.rrc_pair_areas(*_pairs_layout([pairs[i] for i in perm]))
    assert torch.equal(inter.cpu()[perm], inter_r.cpu())
    _, inter_1 = K.rrc_pair_areas(*_pairs_layout(pairs[40:41] * 3))
    assert inter_1.cpu().tolist() == [float(inter[40])] * 3


def _files(sub):
    """{sample key: lines} -> the {file name: lines} dictionary a writer hands over"""
    return {k + ".txt": v for k, v in sub.items()}


def test_exact_ties_do_not_match_and_just_above_does():
    from glass_amd.evaluation import RRCScorer
    gt, sub, want = C.tie_case()
    for ws in (False, True):
        scorer = RRCScorer(gt, ws, _dev())
        got = scorer.score(_files(sub))
        exp = C.check_score(gt, sub, ws)
        assert got["e2e_method"] == exp["e2e_method"] and got["det_only_method"] == exp["det_only_method"]
        assert got["per_sample"]["1"]["iouMat"] == [[0.5]] and got["per_sample"]["2"]["iouMat"] == [[0.55]]
        assert got["per_sample"]["4"]["detDontCare"] == [0] and got["per_sample"]["3"]["detDontCare"] == []
        assert got["per_sample"]["6"]["iouMat"] == [[0.0]]
    # the device decisions themselves
    from glass_amd.ops import native as K
    scorer = RRCScorer(gt, False, _dev())
    enc = scorer.encode_submission(_files(sub))
    G, D = enc.n_gt_per_image, enc.n_det_per_image
    pair_off = K.upload(np.concatenate([[0], np.cumsum(G * D)]), torch.int64, _dev())
    area, inter = K.rrc_pair_areas(enc.pts, enc.poly_off, enc.gt_off, enc.det_off, pair_off, int((G * D).sum()))
    dc_e, dc_d, m_e, m_d = (t.cpu().tolist() for t in K.rrc_match(area, inter, pair_off, enc.gt_off, enc.det_off, scorer._gt_dc_e2e,
                                                                    scorer._gt_dc_det, int(D.sum())))
    assert dc_e == sum((list(w[0]) for w in want.values()), []) and dc_d == sum((list(w[1]) for w in want.values()), [])
    assert m_e == sum((list(w[2]) for w in want.values()), []) and m_d == sum((list(w[3]) for w in want.values()), [])


def _same_sample(got, exp, key, gt, sub):
    for f in ("precision", "recall", "hmean", "gtPolPoints", "detPolPoints", "gtTrans", "detTrans", "gtDontCare", "detDontCare"):
        assert got[f] == exp[f], (key, f, got[f], exp[f])


def test_decisions_on_the_multi_image_case_equal_the_exact_checker():
    """match_*, det_dontcare_*, every per-sample field and the two method lines against the recorded answers of the exact
    checker (tests/golden/rrc_decisions.json; tests/test_rrc_score.py re-derives a sample and checks the bands).  iouMat is
    a float field: it is compared with the exact rational value within the propagated bound, 2 * bound / union + 4 * 2^-53,
    on a sample of images."""
    from glass_amd.evaluation import RRCScorer
    from glass_amd.evaluation.rrc_score import parse_detection_line
    gold = C.load_decisions_golden()
    gt, sub, planted, _ = C.decisions_case(redraws=gold["redraws"])
    assert C.case_digest(gt, sub) == gold["digest"] and len(gt) >= 200
    for ws, name in ((False, "e2e"), (True, "word_spotting")):
        scorer = RRCScorer(gt, ws, _dev())
        got = scorer.score(_files(sub))
        want = gold[name]
        assert got["e2e_method"] == want["e2e_method"] and got["det_only_method"] == want["det_only_method"]
        assert list(got["per_sample"]) == list(gt)
        bad = []
        for key, w in want["per_sample"].items():
            g = got["per_sample"][key]
            for f in ("precision", "recall", "hmean", "gtDontCare", "detDontCare"):
                if g[f] != w[f]:
                    bad.append((key, f, g[f], w[f]))
        assert not bad, bad[:5]
        # the raw decisions of the device, image by image
        scorer1 = RRCScorer(gt, ws, _dev(), chunk_images=1)
        assert scorer1.score(_files(sub)) == got                                       # a chunk boundary changes nothing
        dec = _device_decisions(scorer, sub)
        for key, w in want["per_sample"].items():
            assert dec[key] == [list(x) for x in w["decisions"]], key
    keys = planted + [k for k in gt if k not in planted][::11]
    exact = C.check_score({k: gt[k] for k in keys}, {k: sub[k] for k in keys if k in sub}, False)
    got = RRCScorer(gt, False, _dev()).score(_files(sub))
    for key in keys:
        e, g = exact["per_sample"][key], got["per_sample"][key]
        _same_sample(g, e, key, gt, sub)
        assert (g["iouMat"] == []) == (e["iouMat"] == []), key
        rings = [C.ring(parse_detection_line(l)[0]) for l in sub.get(key, [])]
        for gi, row in enumerate(e["iouMat"]):
            for di, v in enumerate(row):
                Gr = C.ring(gt[key][0][gi])
                union = C.exact_area(Gr) + C.exact_area(rings[di]) - C.exact_intersection(Gr, rings[di])
                tol = (2 * C.inter_bound(Gr, rings[di]) / float(union) if union else 0.0) + 4 * 2.0 ** -53
                assert abs(g["iouMat"][gi][di] - float(v)) <= tol, (key, gi, di)
    assert got["per_sample"][planted[-1]]["iouMat"] == [] and len(got["per_sample"][planted[-1]]["detTrans"]) == 101


def _device_decisions(scorer, sub):
    from glass_amd.ops import native as K
    enc = scorer.encode_submission(_files(sub))
    G, D = enc.n_gt_per_image, enc.n_det_per_image
    pair_off = K.upload(np.concatenate([[0], np.cumsum(G * D)]), torch.int64, _dev())
    area, inter = K.rrc_pair_areas(enc.pts, enc.poly_off, enc.gt_off, enc.det_off, pair_off, int((G * D).sum()))
    dc_e, dc_d, m_e, m_d = (t.cpu().tolist() for t in K.rrc_match(area, inter, pair_off, enc.gt_off, enc.det_off, scorer._gt_dc_e2e,
                                                                    scorer._gt_dc_det, int(D.sum())))
    out, g0, d0 = {}, 0, 0
    for key, g, d in zip(scorer.keys, G.tolist(), D.tolist()):
        out[key] = [dc_e[d0:d0 + d], dc_d[d0:d0 + d], m_e[g0:g0 + g], m_d[g0:g0 + g]]
        g0, d0 = g0 + g, d0 + d
    return out


# ------------------------------------------------------------------------------------------------------ end to end

def _encoder():
    from glass_amd.config import get_glass_cfg
    from glass_amd.modeling.recognition.text_encoder import TextEncoder
    cfg = get_glass_cfg()
    cfg.MODEL.ROI_RECOGNIZER_HEAD.NAME = "RecognizerRCNNHeadV3"
    cfg.MODEL.ROI_RECOGNIZER_HEAD.MAX_WORD_LENGTH = 25
    return TextEncoder(cfg)


def _instances(enc, boxes, words, scores, masks=None):
    """synthetic model output: rotated boxes, one-hot-ish text probabilities that decode to `words`"""
    from glass_amd.structures.core import Instances, RotatedBoxes
    inst = Instances((480, 640))
    b = torch.tensor(boxes, dtype=torch.float32).reshape(-1, 5)
    inst.pred_boxes, inst.pred_rboxes = RotatedBoxes(b.clone()), RotatedBoxes(b.clone())
    inst.scores = torch.tensor(scores, dtype=torch.float32)
    inst.pred_classes = torch.zeros(len(b), dtype=torch.int64)
    labels = enc.encode(words)[:, 1:]
    prob = torch.full((len(words), labels.shape[1], len(enc.character)), 0.001)
    prob.scatter_(2, labels.unsqueeze(-1), 0.9)
    inst.pred_text_prob = prob
    if masks is not None:
        inst.pred_masks = torch.from_numpy(masks)
    return inst


_E2E_WORDS = ["hello", "World", "STOP", "cafe", "exit", "street", "OPEN", "sale", "John", "market"]


def _writer_case(dataset, seed, n_images, with_masks):
    """(inputs, outputs, gt): images named so that the writer's sort gives ids 1..n (icdar) / 0..n-1 (totaltext)"""
    import random
    r = random.Random(seed)
    enc = _encoder()
    inputs, outputs, gt = [], [], OrderedDict()
    for i in range(n_images):
        n = r.randint(0, 6)
        boxes = [[r.randint(80, 560), r.randint(60, 420), r.randint(30, 120), r.randint(12, 40), r.choice([0, 0, 15, -30, 90])] for _ in range(n)]
        words = [r.choice(_E2E_WORDS) for _ in range(n)]
        masks = None
        if with_masks:
            masks = np.zeros((n, 480, 640), dtype=bool)
            for k, (cx, cy, w, h, _) in enumerate(boxes):                       # an L-shaped region: a many-point ring
                masks[k, cy - h // 2:cy + h // 2, cx - w // 2:cx + w // 2] = True
                masks[k, cy - h // 2:cy, cx:cx + w // 2] = False
                for t in range(0, w // 2 - 2, 4):                               # a staircase edge adds vertices
                    masks[k, cy + h // 2:cy + h // 2 + 1 + t // 4, cx - w // 2 + t:cx - w // 2 + t + 2] = True
        inputs.append({"file_name": f"img_{i + 1}.jpg" if dataset.startswith("icdar") else f"{i:07d}.jpg"})
        outputs.append({"instances": _instances(enc, boxes, [w if r.random() < 0.8 else w + "x" for w in words],
                                                [r.choice([0.9, 0.7, 0.45]) for _ in range(n)], masks)})
        # ground truth: the same boxes, jittered, as rings; some don't-care, some decorated
        rings, texts = [], []
        from glass_amd.evaluation import rotated_boxes_to_polygons
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


def _evaluate_and_check(writer, gt, ws, dev):
    from glass_amd.evaluation import RRCScorer
    from glass_amd.evaluation.rrc_score import load_submission, parse_method_string
    scorer = RRCScorer(gt, ws, dev)
    got = writer.evaluate(scorer, 0.5, 0.4)
    with mock.patch("time.time", return_value=1_700_000_000.0):
        det_zip = writer.det_zip(writer.to_eval_format(writer.coco_results(), 0.5, 0.4))
    exp = C.check_score(gt, load_submission(det_zip), ws)
    want = OrderedDict(parse_method_string(exp[k]) for k in ("e2e_method", "det_only_method"))
    assert got == want and list(got) == ["E2E_RESULTS", "DETECTION_ONLY_RESULTS"], (got, want)
    assert RRCScorer(gt, ws, dev, chunk_images=1).score(det_zip) == scorer.score(det_zip)     # chunking; zip input
    assert writer.evaluate(RRCScorer(gt, ws, dev, chunk_images=1), 0.5, 0.4) == got
    full = scorer.score(det_zip)
    assert full["e2e_method"] == exp["e2e_method"] and full["det_only_method"] == exp["det_only_method"]
    for key, e in exp["per_sample"].items():
        _same_sample(full["per_sample"][key], e, key, None, None)
    return got, exp


def test_writer_evaluate_icdar15_quads_with_and_without_word_spotting_and_lexicon():
    from glass_amd.evaluation import LexiconMatcher, TextResultWriter
    dev = _dev()
    enc, inputs, outputs, gt = _writer_case("icdar15", 11, 24, False)
    lexicon = _E2E_WORDS + ["hallo", "exits"]
    pairs = {w.upper(): w for w in lexicon}
    seen = set()
    for ws in (False, True):
        for matcher in (None, "device"):
            kw = dict(dataset="icdar15", word_spotting=ws)
            if matcher:
                kw.update(lexicon=lexicon, pairs=pairs, lexicon_type=1, matcher=LexiconMatcher(lexicon, pairs, device=dev))
            w = TextResultWriter(enc, **kw)
            assert w.evaluate(None) == OrderedDict()                                            # no predictions: {} as the reference
            w.process(inputs, outputs)
            got, exp = _evaluate_and_check(w, gt, ws, dev)
            assert 0 < got["E2E_RESULTS"]["hmean"] < 1 and 0 < got["DETECTION_ONLY_RESULTS"]["hmean"] < 1
            seen.add((ws, bool(matcher), got["E2E_RESULTS"]["hmean"]))
    assert len({h for _, _, h in seen}) > 1                                                     # the settings change the score


def test_writer_evaluate_totaltext_many_point_rings():
    from glass_amd.evaluation import TextResultWriter, masks_to_polygons
    dev = _dev()
    enc, inputs, outputs, gt = _writer_case("totaltext", 12, 10, True)
    w = TextResultWriter(enc, dataset="totaltext", masks_to_polygons=masks_to_polygons)
    w.process(inputs, outputs)
    files = w.to_eval_format(w.coco_results(), 0.5, 0.4)
    assert max(l.count(",") for ls in files.values() for l in ls) > 40                           # rings of > 20 points
    got, exp = _evaluate_and_check(w, gt, False, dev)
    assert got["DETECTION_ONLY_RESULTS"]["hmean"] > 0


def test_bad_input_raises_before_anything_is_launched():
    from glass_amd.evaluation import RRCScorer
    from glass_amd.ops import native as K
    gt = OrderedDict([("1", ([[0, 0, 10, 0, 10, 10, 0, 10]], ["a"]))])
    ok = "0,10,10,10,10,0,0,0,####a"
    scorer = RRCScorer(gt, False, _dev())
    assert scorer.score({"1.txt": [ok]})["e2e_method"] == "E2E_RESULTS: precision: 1.0, recall: 1.0, hmean: 1.0"
    with mock.patch.object(K, "rrc_pair_areas", side_effect=AssertionError("launched")), \
            mock.patch.object(K, "rrc_match", side_effect=AssertionError("launched")):
        for files in ({"1.txt": ["0,10,10,10,10,0.5,0,0,####a"]}, {"1.txt": ["0,10,10,10,10,0,0,2000000,####a"]},
                      {"1.txt": ["0,0,10,0,10,10,0,10,####counter-clockwise"]}, {"1.txt": ["0,20,10,0,10,10,0,0,####bowtie"]},
                      {"2.txt": [ok]}, {"res_1.txt": [ok]}):
            with pytest.raises(ValueError):
                scorer.score(files)
        buf = io.BytesIO()
        with zipfile.ZipFile(buf, "w") as z:
            z.writestr("2.txt", ok + "\n")
        with pytest.raises(ValueError):
            scorer.score(buf.getvalue())
    with pytest.raises(ValueError):
        RRCScorer(OrderedDict([("1", ([[0, 0, 3000000, 0, 10, 10]], ["a"]))]), False, _dev())
    with pytest.raises(K.GlassLibraryError):
        K.rrc_pair_areas(torch.zeros((4, 2), dtype=torch.int32), *[torch.zeros(2, dtype=torch.int32)] * 3, torch.zeros(2, dtype=torch.int64), 0)
