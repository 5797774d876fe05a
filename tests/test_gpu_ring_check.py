"""GPU: the detection ring check (csrc/ring_check.hip) through ops.native.ring_check, RingChecker, TextResultWriter and
RRCScorer.  Expected verdicts come from the rational checker of tests/ring_check_cases.py (pinned to
`normalize_detection_line` by tests/test_ring_check.py), expected strings and errors from the host path itself."""
import functools
from collections import OrderedDict

import numpy as np
import pytest
import torch

import ring_check_cases as C

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _run(rings):
    """(verdict, area2) device tensors of one native call on a list of point lists"""
    from glass_amd.ops import native as K
    flat = np.array([v for r in rings for p in r for v in p], dtype=np.int32).reshape(-1, 2)
    off = np.concatenate([[0], np.cumsum([len(r) for r in rings])]).astype(np.int64)
    return K.ring_check(K.upload(flat, torch.int32, _dev()), off)


@functools.lru_cache(maxsize=None)
def _case_lines():
    """(lines, what the host function makes of them): every case with a point, odd spellings, and one line for the fallback"""
    from glass_amd.evaluation import normalize_detection_line
    lines = [C.to_line(p, f"w{k}") for k, (_, p, _) in enumerate(C.all_cases()) if len(p) >= 1]
    lines += [" 1,1, 5,1,+5,4,1,4,####sp aced ", "0,0,4,0,4,3,0,3,####a,####b", "0,0,0,3,4,3,4,0,####",
              f"0,0,{(1 << 20) + 1},0,4,3,####far", f"0,0,0,3,{-(1 << 20) - 1},3,####far", f"0,0,{1 << 70},0,4,3,####huge"]
    return tuple(lines), tuple(normalize_detection_line(l) for l in lines)


def test_every_case_verdict_and_area():
    rings = [p for _, p, _ in C.all_cases()]
    verdict, area2 = _run(rings)
    assert verdict.dtype == torch.int32 and area2.dtype == torch.int64 and verdict.shape == area2.shape == (len(rings),)
    verdict, area2 = verdict.cpu().tolist(), area2.cpu().tolist()
    for (name, points, _), v, a in zip(C.all_cases(), verdict, area2):
        assert a == C.shoelace2(points), (name, a, C.shoelace2(points))
        assert v == C.expected_verdict(points), (name, v)


def test_mixed_batch_is_deterministic_and_independent_of_neighbours_and_order():
    rings, index = C.mixed_batch()
    v1, a1 = _run(rings)
    v2, a2 = _run(rings)
    assert torch.equal(v1, v2) and torch.equal(a1, a2)                                  # two runs: bit-identical
    got = v1.cpu().tolist()
    assert got == [C.expected_verdict(r) for r in rings]
    assert a1.cpu().tolist() == [C.shoelace2(r) for r in rings]
    for k, c in enumerate(index):                                                       # every case ring alone: same verdict
        if c >= 0:
            alone = _run([rings[k]])[0].cpu().tolist()
            assert alone == [got[k]], (C.all_cases()[c][0], alone, got[k])
    order = np.random.RandomState(5).permutation(len(rings))
    v3, a3 = _run([rings[k] for k in order])
    assert v3.cpu().tolist() == [got[k] for k in order] and torch.equal(a3.cpu(), a1.cpu()[torch.from_numpy(order)])


def test_checker_check_and_normalize_lines_equal_the_host_function():
    from glass_amd.evaluation import RingChecker, normalize_detection_line
    rc = RingChecker(_dev())
    rings = [p for _, p, _ in C.all_cases()] + [[(0, 0), ((1 << 20) + 1, 0), (4, 3)], [(0, 0), (4, 3), (1 << 70, 0)]]
    got = rc.check(rings)
    assert got.dtype == np.int32 and got.tolist() == [C.expected_verdict(r) for r in rings]
    lines, want = _case_lines()
    assert rc.normalize_lines(list(lines)) == list(want)
    assert sum(w is None for w in want) > 20 and sum(w is not None and w != l.strip() for w, l in zip(want, lines)) > 10
    assert rc.normalize_lines([]) == []
    for bad, exc in (("1,2,3,####x", AssertionError), ("1,2,3,4", IndexError), ("1,2,a,4,####x", ValueError)):
        for fn in (lambda ls: [normalize_detection_line(l) for l in ls], rc.normalize_lines):
            with pytest.raises(exc) as e:
                fn(list(lines[:5]) + [bad])
            assert exc is not AssertionError or "cors invalid." in str(e.value)


def _prediction_set():
    """(predictions of 3 images, gt): box quads in both windings, traced mask rings, and lines the protocol drops"""
    from glass_amd.evaluation import masks_to_polygons
    masks = np.zeros((3, 60, 90), dtype=bool)
    for k in range(3):
        masks[k, 10 + k:40, 8:70 + 5 * k] = True
        for t in range(0, 30, 3):                                                       # a staircase edge
            masks[k, 40:41 + t // 3, 8 + t:11 + t] = True
        masks[k, 20:24, 30:34] = False                                                  # a hole: ignored by the ring
    traced = [[(int(x), int(y)) for x, y in r] for r in masks_to_polygons(masks)]
    assert min(len(r) for r in traced) > 20
    pinch = [p for n, p, _ in C.small_cases() if n.startswith("pinch")]
    dropped = [p for _, p, w in C.small_cases() if len(p) >= 3 and (w == 0 or isinstance(w, tuple))]
    dropped += [p for n, p, w in C.block_edge_cases() if n.startswith("staircase 65,")]
    quads = [[(100 + 40 * k, 50), (130 + 40 * k, 50), (130 + 40 * k, 70), (100 + 40 * k, 70)] for k in range(6)]
    predictions, gt = [], OrderedDict()
    for i in range(3):
        rings = [quads[2 * i], quads[2 * i + 1][::-1], traced[i], pinch[i % 2]] + dropped[i::3]
        recs = [{"image_id": None, "polys": [list(q) for q in p], "rec": ["stop", "exit", "open"][k % 3],
                 "score_text": [0.9, 0.6, 0.3][k % 3], "score_detection": [0.95, 0.5][k % 2]} for k, p in enumerate(rings)]
        predictions.append({"file_name": f"{i:07d}.jpg", "instances": recs})
        gt[f"{i:07d}"] = ([[v for p in quads[2 * i] for v in p], [v for p in traced[i][:-1] for v in p], [5, 5, 60, 5, 60, 25, 5, 25]],
                          ["stop", "open", "###"])
    return predictions, gt


def _writer(predictions, ring_checker=None):
    from glass_amd.evaluation import TextResultWriter
    w = TextResultWriter(None, dataset="totaltext", ring_checker=ring_checker)
    w._predictions = [dict(p) for p in predictions]
    return w


def test_writer_with_and_without_ring_checker():
    from glass_amd.evaluation import RingChecker, RRCScorer
    dev = _dev()
    predictions, gt = _prediction_set()
    plain, batched = _writer(predictions), _writer(predictions, RingChecker(dev))
    files = plain.to_eval_format(plain.coco_results(), 0.0, 0.0)
    assert len(files) == 3 and all(len(v) >= 6 for v in files.values())
    det_zip = plain.det_zip(files)
    assert batched.det_zip(files) == det_zip
    scorer = RRCScorer(gt, False, dev)
    want = plain.evaluate(scorer, 0.5, 0.0)
    assert batched.evaluate(scorer, 0.5, 0.0) == want and want["DETECTION_ONLY_RESULTS"]["hmean"] > 0
    ts, ds = [0.0, 0.5, 0.8], [0.0, 0.6, 0.99]
    a, b = plain.sweep(scorer, ts, ds), batched.sweep(scorer, ts, ds)
    assert a.counts.shape == (3, 3, 6) and np.array_equal(a.counts, b.counts) and len({tuple(c) for c in a.counts.reshape(-1, 6).tolist()}) > 2


def test_scorer_validates_in_one_batch_with_the_same_errors():
    from glass_amd.evaluation import RingChecker, RRCScorer
    dev = _dev()
    predictions, gt = _prediction_set()
    w = _writer(predictions)
    det_zip = w.det_zip(w.to_eval_format(w.coco_results(), 0.0, 0.0))
    plain, batched = RRCScorer(gt, False, dev), RRCScorer(gt, False, dev, ring_checker=RingChecker(dev))
    assert batched.score(det_zip) == plain.score(det_zip)
    assert batched.score(det_zip, validate=False) == plain.score(det_zip)
    good, crossing, ccw = "100,50,100,70,130,70,130,50,####a", "0,0,4,0,0,3,6,3,####b", "0,0,4,0,4,3,0,3,####c"
    kinked = C.to_line(C.kinked(C.staircase(129), 64)[0][::-1], "k")                    # clockwise as the scorer wants it, sides cross
    for files, word in (({"0000000.txt": [good, crossing], "0000001.txt": [ccw]}, "intersecting"),
                        ({"0000000.txt": [good, ccw], "0000001.txt": [crossing]}, "not clockwise"),
                        ({"0000000.txt": [good], "0000001.txt": [good, kinked, crossing], "0000002.txt": ["1,2,3,####x"]}, "intersecting"),
                        ({"0000000.txt": [good, "0,0,1,1,####d", crossing]}, "not a valid polygon")):
        errors = []
        for scorer in (plain, batched):
            with pytest.raises(ValueError) as e:
                scorer.score(files)
            errors.append(str(e.value))
        assert errors[0] == errors[1] and word in errors[0], errors


def test_degenerate_calls():
    from glass_amd.evaluation import RingChecker
    from glass_amd.ops import native as K
    dev = _dev()
    verdict, area2 = K.ring_check(torch.empty((0, 2), dtype=torch.int32, device=dev), [0])
    assert verdict.shape == area2.shape == (0,)
    assert RingChecker(dev).check([]).tolist() == []
    rings = [[], [(3, 4)], [(1, 2), (5, 7)], [], [(9, 9), (9, 9)]]                     # no ring has a task
    verdict, area2 = _run(rings)
    assert verdict.cpu().tolist() == [0] * 5 and area2.cpu().tolist() == [C.shoelace2(r) for r in rings] == [0] * 5
    verdict, area2 = _run([[], [], []])                                                 # rings but no point: nothing is launched
    assert verdict.cpu().tolist() == [0, 0, 0] and area2.cpu().tolist() == [0, 0, 0]
