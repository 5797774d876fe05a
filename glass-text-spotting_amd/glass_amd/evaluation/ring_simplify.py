"""Exact Douglas-Peucker simplification of traced mask rings: the definition, in Python integers.  The device form
(csrc/ring_simplify.hip through ops.native.simplify_rings, `MaskPolygonizer(simplify=)`) equals `simplify_ring` vertex for
vertex.  The reference has no such step (it returns the raw `exterior.coords`, text_evaluator.py:464-492); a traced ring is a
pixel-edge staircase with one vertex per turn, and every stage after it pays per vertex.

The statement.  `v[0..n-1]` are the vertices without the closing duplicate; `q4 = 4 * tolerance` is an integer in 0..4096.
  distance of p from the chord (a, b): d = b - a, w = p - a, L = d.d, t = w.d;
      num = |w|^2 * L if t <= 0, |p - b|^2 * L if t >= L, (d x w)^2 otherwise     (squared distance to the SEGMENT, times L);
      for a == b: L = 1, num = |w|^2.  "Farther than the tolerance" is 16 * num > q4^2 * L.
  anchors: A = v[0] (the tracer's start, an extreme point), B = the vertex of largest |v[i] - A|^2, lowest index on a tie.
  recursion: Douglas-Peucker on the chains A..B and B..v[n-1], A.  On a chain (lo, hi) the interior vertex of largest num is
      kept if it is farther than the tolerance (earliest in chain order on a tie) and both halves are processed, otherwise the
      whole interior is dropped.  The result does not depend on the order in which chains are processed.
  never losing a ring: if only A and B survive, the vertex of largest num against the chord (A, B) is kept too if that num
      is above zero (lowest index on a tie); if it is zero for every vertex the ring has no area and becomes A, B.
  Rings with n <= 3 and rings whose vertices all equal A are returned unchanged.

Properties (tests/test_ring_simplify.py checks each):
  - the output is a subsequence of the input that starts at v[0], closed again if the input was closed;
  - every dropped vertex lies within the tolerance of the segment between its kept neighbours;
  - a second application changes nothing;
  - tolerance 0 leaves a tracer ring unchanged: the tracer emits turn vertices only, so no vertex lies on the segment
    between its neighbours.
No floating point appears anywhere: every test is a comparison of Python integers."""
from __future__ import annotations

from fractions import Fraction
from typing import List, Sequence, Tuple

MAX_TOLERANCE = 1024


def tolerance_q4(tolerance) -> int:
    """4 * tolerance as an integer; ValueError unless the tolerance is a multiple of 1/4 in [0, 1024]"""
    try:
        q = Fraction(tolerance) * 4
    except (TypeError, ValueError, OverflowError):
        raise ValueError(f"tolerance={tolerance!r} must be a multiple of 1/4 in [0, {MAX_TOLERANCE}]") from None
    if q.denominator != 1 or q < 0 or q > 4 * MAX_TOLERANCE:
        raise ValueError(f"tolerance={tolerance!r} must be a multiple of 1/4 in [0, {MAX_TOLERANCE}]")
    return int(q)


def _integer(c) -> int:
    k = int(c)
    if k != c:
        raise ValueError(f"coordinate {c!r} is not an integer")
    return k


def chord_num(a: Tuple[int, int], b: Tuple[int, int], p: Tuple[int, int]) -> Tuple[int, int]:
    """(num, L) of point p against the chord (a, b): num / L is the squared distance of p from the segment"""
    dx, dy = b[0] - a[0], b[1] - a[1]
    wx, wy = p[0] - a[0], p[1] - a[1]
    L = dx * dx + dy * dy
    if L == 0:
        return wx * wx + wy * wy, 1
    t = wx * dx + wy * dy
    if t <= 0:
        return (wx * wx + wy * wy) * L, L
    if t >= L:
        ux, uy = p[0] - b[0], p[1] - b[1]
        return (ux * ux + uy * uy) * L, L
    c = dx * wy - dy * wx
    return c * c, L


def _farthest(v: List[Tuple[int, int]], a, b, positions) -> Tuple[int, int, int]:
    """(position, num, L) of the first position of largest num against the chord (a, b); position -1 if there is none"""
    best, best_num, L = -1, -1, 1
    for i in positions:
        num, L = chord_num(a, b, v[i])
        if num > best_num:
            best, best_num = i, num
    return best, best_num, L


def simplify_ring(points: Sequence, tolerance) -> list:
    """The ring `points` ([[x, y], ...] of integers, or of floats with integral values as the tracers return them; closed
    with points[-1] == points[0], or open) simplified at `tolerance` pixels (a multiple of 1/4 in [0, 1024]) by the statement
    of this module.  Returns a new list of the kept points, the input's own point objects, in the form of the input."""
    q4 = tolerance_q4(tolerance)
    pts = list(points)
    v = [(_integer(p[0]), _integer(p[1])) for p in pts]
    closed = len(v) >= 2 and v[-1] == v[0]
    n = len(v) - 1 if closed else len(v)
    if n <= 3 or all(v[i] == v[0] for i in range(n)):
        return pts
    A = v[0]
    far = [(v[i][0] - A[0]) ** 2 + (v[i][1] - A[1]) ** 2 for i in range(n)]
    B = far.index(max(far))
    ring = v[:n] + [A]                                                 # position n is A again: the second chain ends there
    keep = [False] * (n + 1)
    keep[0] = keep[B] = keep[n] = True
    chains = [(0, B), (B, n)]
    while chains:
        lo, hi = chains.pop()
        m, num, L = _farthest(ring, ring[lo], ring[hi], range(lo + 1, hi))
        if m >= 0 and 16 * num > q4 * q4 * L:
            keep[m] = True
            chains += [(lo, m), (m, hi)]
    if sum(keep[:n]) == 2:
        m, num, _ = _farthest(ring, A, v[B], range(n))
        if num > 0:
            keep[m] = True
    out = [pts[i] for i in range(n) if keep[i]]
    if closed:
        out.append(pts[-1])
    return out


def simplify_rings_host(rings: Sequence[Sequence], tolerance) -> list:
    """[simplify_ring(r, tolerance) for r in rings]: the host form of ops.native.simplify_rings, e.g. around a host
    `masks_to_polygons` callback"""
    return [simplify_ring(r, tolerance) for r in rings]
