"""Cases and an independent checker for the detection ring check (glass_amd.evaluation.normalize_detection_line on the host,
RingChecker / csrc/ring_check.hip on the device).

`expected_verdict` decides crossings another way than the product: it solves the intersection of the two carrier lines in
`fractions.Fraction`; two sides properly cross iff the lines are not parallel and both parameters lie strictly inside (0, 1).
(Pairs whose bounding boxes are disjoint are skipped first: they cannot cross.)  Verdicts: 0 the ring is dropped, 1 kept as
it stands, 2 kept with its point order reversed.

The cases are the smallest shapes at which the kernel can go wrong; a case that is built to have one crossing carries the
pair of sides it was built for, and the CPU test checks with `crossing_pairs` that this is the only pair."""
import functools
from fractions import Fraction

import numpy as np

MAX_COORD = 1 << 20
BLOCK = 64                                   # sides per block of csrc/ring_check.hip


# ------------------------------------------------------------------------------------------------------------ checker

def shoelace2(points):
    n = len(points)
    return sum(points[i][0] * points[(i + 1) % n][1] - points[(i + 1) % n][0] * points[i][1] for i in range(n))


def properly_cross(p, q, r, s):
    """p + t (q - p) = r + u (s - r) with 0 < t < 1 and 0 < u < 1, exactly"""
    if max(p[0], q[0]) < min(r[0], s[0]) or max(r[0], s[0]) < min(p[0], q[0]) or \
            max(p[1], q[1]) < min(r[1], s[1]) or max(r[1], s[1]) < min(p[1], q[1]):
        return False
    ax, ay, bx, by = q[0] - p[0], q[1] - p[1], s[0] - r[0], s[1] - r[1]
    den = ax * by - ay * bx
    if den == 0:
        return False
    cx, cy = r[0] - p[0], r[1] - p[1]
    t, u = Fraction(cx * by - cy * bx, den), Fraction(cx * ay - cy * ax, den)
    return 0 < t < 1 and 0 < u < 1


def crossing_pairs(points):
    """[(i, j)]: the tested pairs of sides (i + 2 <= j < n, not (0, n - 1)) that properly cross"""
    n = len(points)
    out = []
    for i in range(n):
        p, q = points[i], points[(i + 1) % n]
        for j in range(i + 2, n):
            if i == 0 and j == n - 1:
                continue
            if properly_cross(p, q, points[j], points[(j + 1) % n]):
                out.append((i, j))
    return out


@functools.lru_cache(maxsize=None)
def _expected(points):
    if len(points) < 3:
        return 0
    a2 = shoelace2(points)
    if a2 == 0 or crossing_pairs(points):
        return 0
    return 1 if a2 < 0 else 2


def expected_verdict(points):
    return _expected(tuple((int(x), int(y)) for x, y in points))


def to_line(points, rec="word"):
    return ",".join(f"{int(x)},{int(y)}" for x, y in points) + ",####" + rec


def host_verdict(points):
    """the verdict `normalize_detection_line` implies for a ring of at least one point"""
    from glass_amd.evaluation import normalize_detection_line
    out = normalize_detection_line(to_line(points))
    if out is None:
        return 0
    return 1 if out == to_line(points) else 2


# -------------------------------------------------------------------------------------------------------------- cases
# a case is (name, points, want): want 0 / 1 / 2, "keep" (1 or 2), or a pair (i, j): dropped for exactly that crossing

def _traced(mask):
    from glass_amd.evaluation import masks_to_polygons
    return [(int(x), int(y)) for x, y in masks_to_polygons(np.asarray(mask, dtype=bool)[None])[0]]


def small_cases():
    """cases 1 to 4: short rings, quads, touching, index rules"""
    quad = [(0, 0), (4, 0), (4, 3), (0, 3)]
    bow = [(0, 0), (4, 0), (0, 3), (6, 3)]                              # sides 1 and 3 cross, area2 = -6
    reach = [(0, 0), (6, 0), (6, 4), (3, 4), (2, -2)]                   # side 3 crosses side 0 = sides 0 and n - 2
    out = [
        ("no point", [], 0), ("one point", [(1, 1)], 0), ("two points", [(0, 0), (3, 4)], 0),
        ("triangle, positive shoelace", [(0, 0), (4, 0), (0, 3)], 2), ("triangle, negative shoelace", [(0, 3), (4, 0), (0, 0)], 1),
        ("triangle, collinear", [(0, 0), (1, 1), (2, 2)], 0),
        ("quad, positive shoelace", quad, 2), ("quad, negative shoelace", quad[::-1], 1),
        ("bow-tie, sides 1 x 3", bow, (1, 3)), ("bow-tie, sides 0 x 2", bow[3:] + bow[:3], (0, 2)),
        ("bow-tie of zero area", [(0, 0), (4, 0), (0, 3), (4, 3)], 0),
        ("vertex on another side", [(0, 0), (4, 0), (4, 4), (2, 0), (0, 4)], "keep"),
        ("collinear overlapping sides", [(0, 0), (6, 0), (6, 3), (4, 0), (2, 0), (0, 3)], "keep"),
        ("repeated vertex", [(0, 0), (4, 0), (4, 0), (4, 3), (0, 3)], 2),
        ("closed by its first point", quad + [quad[0]], 2),
        ("closed by its first point, reversed", (quad + [quad[0]])[::-1], 1),
        ("pinch, traced", _traced([[1, 1, 0], [1, 0, 1], [1, 1, 1]]), "keep"),
        ("pinch on the other diagonal, traced", _traced([[0, 1, 1], [1, 0, 1], [1, 1, 1]]), "keep"),
        ("sharp zigzag: only adjacent sides meet", [(0, 0), (9, 1), (1, 2), (9, 3), (1, 4), (9, 5), (0, 6), (-3, 3)], "keep"),
        ("spike back onto the first side", [(0, 0), (6, 0), (6, 4), (0, 4), (3, 0)], "keep"),
        ("one crossing, sides 0 and n - 2", reach, (0, 3)),
        ("one crossing, sides 1 and n - 1", reach[4:] + reach[:4], (1, 4)),
    ]
    return out


def staircase(n, s=4):
    """a simple ring of n >= 7 vertices: n - 1 stair corners (s right, s up, ...) from (0, 0) and one far corner above
    the start that closes it; the inside is above the stairs"""
    k = n - 1
    pts = [(s * ((t + 1) // 2), s * (t // 2)) for t in range(k)]
    pts.append((0, 4 * pts[-1][1] + 3 * s))
    return pts


def kinked(ring, t):
    """`ring` (a staircase) with corner t + 1 pulled back over the riser below corner t (t even): sides t - 1 and t + 1 cross"""
    assert t % 2 == 0 and 2 <= t and t + 2 <= len(ring) - 2
    out = list(ring)
    out[t + 1] = (ring[t][0] - 1, ring[t - 1][1] + 1)
    return out, (t - 1, t + 1)


def reached(ring, m, s=4):
    """`ring` (a staircase) with its first corner moved to just below tread 2m: the closing side, from the far corner,
    crosses that tread = sides 2m and n - 1"""
    assert 1 <= m and 2 * m + 1 <= len(ring) - 2
    out = list(ring)
    out[0] = (m * s + 3, m * s - 2)
    return out, (2 * m, len(ring) - 1)


def block_edge_cases():
    """case 5: ring lengths around the 64-side block: valid, one crossing inside block 0, one between two blocks, one with
    the last block"""
    out = []
    last_tread = {63: 10, 64: 15, 65: 5, 127: 35, 128: 10, 129: 50, 193: 40}       # m of `reached`: side 2m against side n - 1
    for n in (63, 64, 65, 127, 128, 129, 193):
        ring = staircase(n)
        out.append((f"staircase {n}", ring, 2))
        out.append((f"staircase {n} reversed", ring[::-1], 1))
        pts, pair = kinked(ring, 10)
        out.append((f"staircase {n}, crossing in block 0", pts, pair))
        if n >= 68:
            pts, pair = kinked(ring, 64)                                               # sides 63 and 65
            out.append((f"staircase {n}, crossing between blocks 0 and 1", pts, pair))
        if n >= 132:
            pts, pair = kinked(ring, 128)                                              # sides 127 and 129
            out.append((f"staircase {n}, crossing between blocks 1 and 2", pts, pair))
        pts, pair = reached(ring, last_tread[n])
        out.append((f"staircase {n}, crossing of sides {pair[0]} and {pair[1]} (last block)", pts, pair))
    return out


@functools.lru_cache(maxsize=None)
def band_ring():
    """the host tracer's outline of a slanted band, about 1,700 vertices"""
    yy, xx = np.mgrid[0:436, 0:570]
    return tuple(_traced(np.abs(yy - 0.75 * xx - 12) < 9))


def band_crossed(ring):
    """`ring` (the band) with the upper-edge corner 421 moved across the band to (266, 237), beyond the lower edge: the new
    side 421 runs exactly through the lower-edge vertex 1274 = (274, 226), the middle of that side, which is touching and no
    crossing, and the new side 420 properly crosses the lower-edge side 1275 beside it: one crossing, between sides a
    quarter and three quarters of the way round the ring (blocks 6 and 19)"""
    assert len(ring) == 1687 and ring[420:423] == [(280, 214), (282, 214), (282, 215)] and ring[1274] == (274, 226)
    out = list(ring)
    out[421] = (266, 237)
    return out, (420, 1275)


def long_ring_cases():
    """case 6: one long ring, as traced and with one far crossing"""
    ring = list(band_ring())
    out = [("band as traced", ring, "keep")]
    pts, pair = band_crossed(ring)
    out.append(("band with one crossing", pts, pair))
    return out


def magnitude_cases():
    """case 7: coordinates at +-2^20; the determinants are about 2^41 .. 2^43 and differ by one unit between the cases"""
    M = MAX_COORD
    def diag(p3):
        return [(-M, -M), (M, M - 2), (M, -M), p3]                    # (0, -1) is the middle of side 0
    def flat(y):
        return [(-M, -M + 2), (M, -M + 2), (M, M), (1, y)]
    return [
        ("2^20: vertex on the long diagonal", diag((0, -1)), "keep"), ("2^20: vertex one below the long diagonal", diag((0, -2)), "keep"),
        ("2^20: vertex one past the long diagonal", diag((0, 0)), (0, 2)),
        ("2^20: vertex on the bottom side", flat(-M + 2), "keep"), ("2^20: vertex above the bottom side", flat(-M + 3), "keep"),
        ("2^20: vertex below the bottom side", flat(-M), (0, 2)),
        ("2^20: full square", [(-M, -M), (M, -M), (M, M), (-M, M)], 2), ("2^20: full square reversed", [(-M, M), (M, M), (M, -M), (-M, -M)], 1),
        ("2^20: bow-tie", [(-M, -M), (0, -M), (-M, M), (M, M)], (1, 3)),
    ]


@functools.lru_cache(maxsize=None)
def all_cases():
    """cases 1 to 7 as a tuple of (name, points, want)"""
    return tuple(small_cases() + block_edge_cases() + long_ring_cases() + magnitude_cases())


def random_quads(count=3000, seed=20261):
    rng = np.random.RandomState(seed)
    return [[(int(x), int(y)) for x, y in q] for q in rng.randint(0, 7, size=(count, 4, 2))]


@functools.lru_cache(maxsize=None)
def mixed_batch(seed=20261):
    """case 8: (rings, case_index): 3,000 random quads and every ring of cases 1 to 7 in one shuffled order; case_index[k] is
    the index into all_cases() of ring k, or -1 for a quad"""
    quads = random_quads(seed=seed)
    rings = quads + [list(p) for _, p, _ in all_cases()]
    index = [-1] * len(quads) + list(range(len(all_cases())))
    order = np.random.RandomState(seed + 1).permutation(len(rings))
    return tuple(rings[k] for k in order), tuple(index[k] for k in order)
