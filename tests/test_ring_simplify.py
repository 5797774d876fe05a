"""Host: the statement of the ring simplifier (glass_amd.evaluation.simplify_ring) against the independent checker of
ring_simplify_cases.py, its four stated properties, known answers, the 2^20 case that float64 cannot decide, every ValueError,
the header, and the premise of MaskPolygonizer's `keep_valid` fallback."""
import os
from fractions import Fraction

import pytest

import ring_simplify_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["glass_ring_simplify_workspace_bytes", "glass_ring_simplify_mark", "glass_ring_simplify_write"]


def _open(ring):
    return ring[:-1] if len(ring) >= 2 and ring[-1] == ring[0] else ring


def test_equals_the_checker_on_every_case():
    from glass_amd.evaluation import simplify_ring, simplify_rings_host
    shorter = 0
    for tol in C.TOLERANCES:
        rings = [r for _, r in C.all_cases()]
        got = simplify_rings_host(rings, tol)
        assert len(got) == len(rings)
        for (name, ring), g in zip(C.all_cases(), got):
            assert g == C.reference_simplify(ring, tol), (name, tol)
            assert g == simplify_ring(ring, tol), (name, tol)
            shorter += len(g) < len(ring)
    assert shorter > 100                                               # the comparison is not one of unchanged rings


def test_the_four_properties():
    from glass_amd.evaluation import simplify_ring
    for name, ring in C.all_cases():
        for tol in C.TOLERANCES:
            out = simplify_ring(ring, tol)
            closed = len(ring) >= 2 and ring[-1] == ring[0]
            # a subsequence that starts at v[0], in the form of the input
            assert not closed or (len(out) >= 2 and out[0] == ring[0] and out[-1] == ring[-1]), (name, tol)
            v, o = _open(ring), _open(out)
            assert not v or o[0] == v[0], (name, tol)
            it = iter(range(len(v)))
            idx = [next(i for i in it if v[i] == p) for p in o]        # raises StopIteration if `o` is no subsequence
            # every dropped vertex lies within the tolerance of the segment between its kept neighbours
            if len(o) >= 2 and len(o) < len(v):
                ends = idx + [len(v)]
                ring_v = v + [v[0]]
                for lo, hi in zip(ends[:-1], ends[1:]):
                    for i in range(lo + 1, hi):
                        assert C.seg_dist2(ring_v[i], ring_v[lo], ring_v[hi]) <= Fraction(tol) ** 2, (name, tol, i)
            # a second application changes nothing
            assert simplify_ring(out, tol) == out, (name, tol)
    # tolerance 0 leaves a tracer ring unchanged
    for name, ring in C.all_cases():
        if name.startswith(("blob", "band")):
            assert simplify_ring(ring, 0) == ring, name


def test_known_answers():
    from glass_amd.evaluation import simplify_ring
    stair = C.staircase(12)
    assert simplify_ring(stair, 1) == [[0, 0], [12, 12], [-12, 12], [0, 0]]           # 0.707 px from the chord: all dropped
    assert simplify_ring(stair, 0.25) == stair                                       # and all kept at a quarter pixel
    # at half a pixel ties go to the earliest vertex, so the chain to (12, 12) is peeled from its start: every vertex is kept
    # (0.707 px, or more than 0.5 px from the peeled chords) until the chain is (11, 10) .. (12, 12), a chord of slope 2 from
    # which (11, 11) and (12, 11) lie 1 / sqrt(5) = 0.447 px: those two are dropped
    assert simplify_ring(stair, 0.5) == [p for p in stair if p not in ([11, 11], [12, 11])]
    assert simplify_ring(C.staircase(9, closed=False), 1) == [[0, 0], [9, 9], [-9, 9]]
    # a 1-pixel-high word: the two other corners are within 1 px of the diagonal, the third-vertex rule keeps the farther
    thin = simplify_ring([[0, 0], [40, 0], [40, 1], [0, 1], [0, 0]], 1)
    assert thin == [[0, 0], [40, 0], [40, 1], [0, 0]] and len(set(map(tuple, thin))) == 3
    # a vertex exactly at the tolerance is dropped, one lattice step farther out it is kept
    at = [[0, 0], [10, 2], [20, 0], [20, -30], [0, -30], [0, 0]]
    assert simplify_ring(at, 2) == [[0, 0], [20, 0], [20, -30], [0, -30], [0, 0]]
    out = [[0, 0], [10, 3], [20, 0], [20, -30], [0, -30], [0, 0]]
    assert simplify_ring(out, 2) == out
    # two equidistant vertices: the earlier one wins, and at 3 px neither is farther than the tolerance
    assert simplify_ring(C.TIE, 2.75) == [[0, 0], [4, 3], [16, 0], [8, -20], [0, 0]]
    assert simplify_ring(C.TIE, 3) == [[0, 0], [16, 0], [8, -20], [0, 0]]
    # a repeated position
    assert simplify_ring(C.PINCH, 0) == C.PINCH
    assert simplify_ring(C.PINCH, 1) == [[0, 0], [2, 0], [4, 4], [2, 4], [0, 0]]       # (2, 2) lies on the chord, both times
    assert simplify_ring(C.PINCH, 1.5) == [[0, 0], [2, 0], [4, 4], [0, 0]]             # four corners at 1.414 px: the third vertex
    # open and closed forms agree up to the closing point
    for name, ring in C.all_cases():
        if len(ring) >= 5 and ring[-1] == ring[0]:
            for tol in (0.25, 1, 3):
                assert simplify_ring(ring, tol)[:-1] == simplify_ring(ring[:-1], tol), (name, tol)
    # n = 0, 1, 2, 3: unchanged, a new list
    for ring in ([], [[5, 5]], [[0, 0], [3, 4]], [[0, 0], [9, 0], [0, 9]], [[0, 0], [9, 0], [0, 9], [0, 0]]):
        got = simplify_ring(ring, 6)
        assert got == ring and got is not ring
    # zero area: A, B
    assert simplify_ring([[0, 0], [4, 2], [8, 4], [2, 1], [6, 3], [0, 0]], 1) == [[0, 0], [8, 4], [0, 0]]
    # the tracers' float rings are taken as they are, and returned as the same point objects
    fl = [[float(x), float(y)] for x, y in stair]
    got = simplify_ring(fl, 1)
    assert got == [[0.0, 0.0], [12.0, 12.0], [-12.0, 12.0], [0.0, 0.0]] and got[1] is fl[24]
    with pytest.raises(ValueError):
        simplify_ring([[0.5, 0], [1, 1], [2, 0], [1, -1]], 1)


def test_a_decision_beyond_53_bits():
    from glass_amd.evaluation import simplify_ring
    from glass_amd.evaluation.ring_simplify import chord_num
    for name, ring, tol, kept in C.high_bit_cases():
        num, L = chord_num(tuple(ring[0]), tuple(ring[2]), tuple(ring[1]))
        lhs, rhs = 16 * num, (4 * tol) ** 2 * L
        assert lhs > 1 << 60 and rhs > 1 << 60 and lhs - rhs == (16 if kept else 0), name
        assert float(lhs) == float(rhs), name                          # float64 sees no difference
        got = simplify_ring(ring, tol)
        assert got == C.reference_simplify(ring, tol), name
        assert (ring[1] in got) == kept and len(got) == (5 if kept else 4), name


def test_value_errors():
    from glass_amd.evaluation import simplify_ring, simplify_rings_host
    ring = C.staircase(5)
    for bad in (0.3, 1.1, 1 / 3, -0.25, -1, 1024.25, 2000, float("nan"), float("inf"), "one", None):
        with pytest.raises(ValueError):
            simplify_ring(ring, bad)
        with pytest.raises(ValueError):
            simplify_rings_host([ring], bad)
    for good in (0, 0.25, 1, Fraction(3, 4), 1024, 1024.0):
        simplify_ring(ring, good)


def test_feature_header_and_binding():
    import re
    from glass_amd import _lib
    from glass_amd.ops import native as K
    with open(os.path.join(ROOT, "include", "glass_hip_feature_simplify.h")) as fh:
        text = fh.read()
    assert list(_lib.signatures(text)) == NAMES
    for name in NAMES:
        assert _lib.FEATURE_EXPORTS.count(name) == 1 and name not in _lib.EXPORTS + _lib.EXT_EXPORTS + _lib.ADDON_EXPORTS, name
    for other in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if other != "glass_hip_feature_simplify.h":
            with open(os.path.join(ROOT, "include", other)) as fh:
                assert "glass_ring_simplify" not in fh.read(), other
    assert "glass_hip_feature_simplify.h" in [os.path.basename(p) for p in _lib.feature_headers()]
    for word in ("lowest index on a tie", "earliest in chain order", "third vertex", "128", "no floating point", "bit-identical"):
        assert word in text, word                                      # the contract is stated where the entry points are declared
    assert int(re.search(r"#define GLASS_RING_SIMPLIFY_LDS_POINTS (\d+)", text).group(1)) == K.RING_SIMPLIFY_LDS_POINTS
    assert K.RING_SIMPLIFY_MAX_COORD == K.RING_CHECK_MAX_COORD == 1 << 20


def test_the_fallback_has_something_to_catch():
    """`keep_valid` exists because Douglas-Peucker can make a simple ring cross itself: the seeded blobs show it"""
    case = C.invalid_after_simplification()
    found = case["found"]
    print(f"[ring_simplify] {len(found)} of {len(case['rings']) * len(case['simplified'])} simplified blob rings are dropped by normalize_detection_line "
          "while the traced ring is kept")
    assert len(found) >= 3
