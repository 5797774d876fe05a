"""CPU: the ring check's ABI, the case file's independent checker against `normalize_detection_line`, and the host side of
RingChecker / TextResultWriter / RRCScorer (strings, batching, errors) with the device call replaced by the host rule."""
import inspect
import os

import numpy as np
import pytest

import ring_check_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_abi_entries_are_exported_and_declared():
    from glass_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "glass_hip.h")).read()
    for name in ("glass_ring_check_tasks", "glass_ring_check"):
        assert name in _lib.EXPORTS and name + "(" in hdr, name
    assert hdr.count("text_evaluator.py:112-137") >= 2                 # each entry cites its call site
    assert _lib.ABI_VERSION == 8


def test_task_count_helper():
    from glass_amd import _lib
    L = _lib.lib()
    for n, want in ((-1, 0), (0, 0), (2, 0), (3, 1), (64, 1), (65, 3), (128, 3), (129, 6), (1 << 20, 16384 * 16385 // 2)):
        assert int(L.glass_ring_check_tasks(n)) == want, n
    from glass_amd.ops import native as K
    assert K.ring_check_task_offsets([4, 2, 65, 0, 129]).tolist() == [0, 1, 1, 4, 4, 10]
    assert K.ring_check_task_offsets([]).tolist() == [0]


def test_checker_agrees_with_the_host_function_on_every_case():
    assert len(C.all_cases()) > 60
    for name, points, want in C.all_cases():
        got = C.expected_verdict(points)
        if len(points) >= 1:
            assert got == C.host_verdict(points), name
        if want == "keep":
            assert got in (1, 2), name
        elif isinstance(want, tuple):                                  # built for exactly this crossing, and not dropped for its area
            assert got == 0 and C.crossing_pairs([tuple(p) for p in points]) == [want] and C.shoelace2(points) != 0, name
        else:
            assert got == want, name


def test_cases_cover_what_they_are_for():
    names = [n for n, _, _ in C.all_cases()]
    assert len(set(names)) == len(names)
    ring = C.band_ring()
    assert 1500 <= len(ring) <= 1900 and ring[0] == ring[-1]
    blocks = {(len(p), i // C.BLOCK, j // C.BLOCK) for _, p, w in C.all_cases() if isinstance(w, tuple) for i, j in [w]}
    for n in (63, 64, 65, 127, 128, 129, 193):
        last = (n - 1) // C.BLOCK
        assert (n, 0, 0) in blocks and any(b[0] == n and b[2] == last for b in blocks), n
        if n > 64:
            assert any(b[0] == n and b[1] != b[2] for b in blocks), n
    assert (len(ring), 420 // C.BLOCK, 1275 // C.BLOCK) in blocks and 1275 // C.BLOCK - 420 // C.BLOCK > 10
    assert max(abs(v) for _, p, _ in C.magnitude_cases() for q in p for v in q) == C.MAX_COORD


def test_mixed_batch_has_every_verdict_among_its_quads():
    rings, index = C.mixed_batch()
    quads = [r for r, k in zip(rings, index) if k < 0]
    assert len(quads) == 3000 and sorted(k for k in index if k >= 0) == list(range(len(C.all_cases())))
    v = np.array([C.expected_verdict(q) for q in quads])
    shares = [float((v == k).mean()) for k in range(3)]
    assert min(shares) >= 0.2, shares
    assert index[:40] != sorted(index[:40])                            # shuffled: the cases are interleaved with the quads


class _HostRuleChecker:
    """a RingChecker whose device call is the host rule: everything around the call is the product's code"""

    def __new__(cls):
        from glass_amd.evaluation.ring_check import RingChecker, host_verdict
        self = RingChecker.__new__(RingChecker)
        self.max_coord = self.max_points = 1 << 20
        self.calls = []

        def check_flat(flats):
            self.calls.append(len(flats))
            return np.array([host_verdict(list(f)) if len(f) >= 2 else 0 for f in flats], dtype=np.int32)
        self.check_flat = check_flat
        return self


def _lines():
    lines = [C.to_line(p, f"w{k}") for k, (_, p, _) in enumerate(C.all_cases()) if len(p) >= 1 and len(p) < 300]
    lines += [" 1,1, 5,1,+5,4,1,4,####sp aced ", "0,0,4,0,4,3,0,3,####a,####b", "0,0,0,3,4,3,4,0,####",
              f"0,0,{(1 << 20) + 1},0,4,3,####far", "0,0,4,0,0,3,6,3,####" + "x" * 5, f"0,0,{1 << 70},0,4,3,####huge"]
    return lines


def test_normalize_lines_host_side_equals_the_list_comprehension():
    from glass_amd.evaluation import normalize_detection_line
    rc = _HostRuleChecker()
    lines = _lines()
    want = [normalize_detection_line(l) for l in lines]
    assert rc.normalize_lines(lines) == want and rc.calls == [len(lines)]              # one batched check
    assert any(w is None for w in want) and any(w is not None and w != l.strip() for w, l in zip(want, lines))
    assert rc.normalize_lines([]) == []
    for bad, exc in (("1,2,3,####x", AssertionError), ("1,2,3,4", IndexError), ("1,2,a,4,####x", ValueError), (",####x", AssertionError)):
        for fn in (lambda l: [normalize_detection_line(v) for v in l], rc.normalize_lines):
            with pytest.raises(exc) as e:
                fn(lines[:3] + [bad])
            if exc is AssertionError:
                assert "cors invalid." in str(e.value)


def _writer(ring_checker=None, **kw):
    from glass_amd.evaluation import TextResultWriter
    w = TextResultWriter(None, dataset="totaltext", ring_checker=ring_checker, **kw)
    cases = [p for _, p, _ in C.small_cases() if len(p) >= 3] + [p for n, p, _ in C.block_edge_cases() if " 65" in n]
    for i in range(3):
        recs = [{"image_id": None, "polys": [list(q) for q in p], "rec": f"w{i}{k}", "score_text": [0.9, 0.6, 0.3][k % 3],
                 "score_detection": [0.95, 0.5][k % 2]} for k, p in enumerate(cases[i::3])]
        w._predictions.append({"file_name": f"{i:07d}.jpg", "instances": recs})
    return w


def test_writer_default_is_unchanged_and_a_checker_is_called_once_per_call():
    from glass_amd.evaluation import TextResultWriter, normalize_detection_line
    assert inspect.signature(TextResultWriter.__init__).parameters["ring_checker"].default is None
    plain, rc = _writer(), _HostRuleChecker()
    batched = _writer(rc)
    assert plain.ring_checker is None
    files = plain.to_eval_format(plain.coco_results(), 0.0, 0.0)
    assert len(files) == 3 and sum(len(v) for v in files.values()) > 20
    import io
    import zipfile
    z = zipfile.ZipFile(io.BytesIO(plain.det_zip(files)))
    for name in files:                                                 # the default path: the host function, line by line
        want = "".join(l + "\n" for l in map(normalize_detection_line, files[name]) if l is not None)
        assert z.read(name).decode() == want
    assert batched.det_zip(files) == plain.det_zip(files) and rc.calls == [sum(len(v) for v in files.values())]

    class Scorer:                                                      # records what the writer hands over
        def score(self, files, validate):
            self.files = files
            return {"e2e_method": "E2E_RESULTS: precision: 0, recall: 0, hmean: 0",
                    "det_only_method": "DETECTION_ONLY_RESULTS: precision: 0, recall: 0, hmean: 0"}

        def sweep(self, files, ts, ds, validate):
            self.scored = files
            return None
    a, b = Scorer(), Scorer()
    del rc.calls[:]
    assert plain.evaluate(a, 0.5, 0.0) == batched.evaluate(b, 0.5, 0.0) and a.files == b.files and len(rc.calls) == 1
    plain.sweep(a, [0.0, 0.5], [0.0, 0.9])
    batched.sweep(b, [0.0, 0.5], [0.0, 0.9])
    assert a.scored == b.scored and len(rc.calls) == 2 and any(len(v) for v in a.scored.values())


def test_scorer_and_checker_need_a_device():
    from glass_amd._lib import GlassLibraryError
    from glass_amd.evaluation import RingChecker, RRCScorer
    assert inspect.signature(RRCScorer.__init__).parameters["ring_checker"].default is None
    with pytest.raises(GlassLibraryError):
        RingChecker("cpu")
    with pytest.raises(GlassLibraryError):
        RRCScorer({"1": ([[0, 0, 1, 0, 1, 1]], ["a"])}, False, "cpu", ring_checker=None)
