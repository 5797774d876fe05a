"""Cases and an independent checker for the line grouping (include/glass_hip_feature_lines.h).

The checker is plain Python: per-pair loops with `math`, breadth-first components, `sorted` with explicit keys, `math.fsum`
for the frames.  It shares no code with glass_amd.postprocess.line_grouping.group_lines_host.  For every case it also measures
two margins: the smallest relative distance of any pair comparison to its threshold, and the smallest gap (pixels) between
adjacent ordering keys that are not exact ties.  A case is used only if both are >= MARGIN: float64 evaluations of the same
formulas differ by a few ulps (1e-16 relative), so with such margins every implementation decides every comparison alike.
Pairs whose centres lie farther apart than FAR times their summed sizes cannot link whatever their other comparisons say;
the checker skips them, and the pair margin is over the others.
"""
import math
from collections import deque

import numpy as np

DEFAULTS = {"max_angle_diff": 15.0, "min_height_ratio": 0.5, "max_offset": 0.5, "max_gap": 1.0}
MARGIN = 1e-9
FAR = 4.0
TALLY = {"tried": 0, "rejected": 0}


# ------------------------------------------------------------------------------------------------ the checker
def _rel(lhs, rhs):
    return abs(lhs - rhs) / max(abs(lhs), abs(rhs), 1e-300)


def _wrap(x):
    return (x + 180.0) % 360.0 - 180.0


def _dirs(row):
    t = math.radians(row[4])
    return (math.cos(t), -math.sin(t)), (math.sin(t), math.cos(t))


def is_valid(row):
    return all(math.isfinite(v) for v in row) and row[2] > 0 and row[3] > 0


def pair_link(bi, bj, prm=DEFAULTS):
    """(Link(i, j), the smallest relative distance of its six comparisons to their thresholds) for two valid words"""
    (ui, vi), (uj, vj) = _dirs(bi), _dirs(bj)
    dx, dy = bj[0] - bi[0], bj[1] - bi[1]
    H, h = max(bi[3], bj[3]), min(bi[3], bj[3])
    half = (bi[2] + bj[2]) / 2
    tests = [(abs(_wrap(bj[4] - bi[4])), prm["max_angle_diff"]), (prm["min_height_ratio"] * H, h)]
    tests += [(abs(dx * v[0] + dy * v[1]), prm["max_offset"] * H) for v in (vi, vj)]
    tests += [(abs(dx * u[0] + dy * u[1]) - half, prm["max_gap"] * H) for u in (ui, uj)]
    return all(lhs <= rhs for lhs, rhs in tests), min(_rel(lhs, rhs) for lhs, rhs in tests)


def reference(boxes, prm=DEFAULTS):
    """boxes [n, 5] float32 -> the expected outputs (unpadded; "line_boxes" as float64 rows, an invalid word's as its float32
    values), "links" (the set of linked pairs i < j) and the two margins"""
    rows = [[float(v) for v in r] for r in np.asarray(boxes, dtype=np.float32).reshape(-1, 5)]
    n = len(rows)
    valid = [is_valid(r) for r in rows]
    reach = (1.0 + prm["max_gap"] + prm["max_offset"]) * FAR
    size = [(r[2] + r[3]) * reach if v else 0.0 for r, v in zip(rows, valid)]
    nbr = [[] for _ in range(n)]
    links = set()
    pair_margin = math.inf
    for i in range(n):
        if not valid[i]:
            continue
        bi, si = rows[i], size[i]
        xi, yi = bi[0], bi[1]
        for j in range(i + 1, n):
            if not valid[j]:
                continue
            bj = rows[j]
            far = si + size[j]
            if abs(bj[0] - xi) > far or abs(bj[1] - yi) > far:
                continue
            ok, m = pair_link(bi, bj, prm)
            assert pair_link(bj, bi, prm)[0] == ok, (i, j)           # the rule is symmetric
            pair_margin = min(pair_margin, m)
            if ok:
                nbr[i].append(j); nbr[j].append(i); links.add((i, j))
    comp = [-1] * n
    lines = []
    for s in range(n):
        if comp[s] >= 0:
            continue
        comp[s] = s
        members, q = [s], deque([s])
        while q:
            for k in nbr[q.popleft()]:
                if comp[k] < 0:
                    comp[k] = s
                    members.append(k); q.append(k)
        lines.append(sorted(members))

    def frame(members, fallback):
        Dx = math.fsum(rows[k][2] * _dirs(rows[k])[0][0] for k in members)
        Dy = math.fsum(rows[k][2] * _dirs(rows[k])[0][1] for k in members)
        Sw = math.fsum(rows[k][2] for k in members)
        nrm = math.hypot(Dx, Dy)
        assert not members or nrm > 1e-11 * Sw or nrm < 1e-13 * Sw, "a frame within a factor of 10 of its fallback threshold"
        return (Dx / nrm, Dy / nrm) if nrm > 1e-12 * Sw else fallback

    PU = frame([k for k in range(n) if valid[k]], (1.0, 0.0))
    PV = (-PU[1], PU[0])
    key_margin = math.inf
    good, bad = [], []
    for members in lines:
        if not valid[members[0]]:
            bad.append({"words": members, "box": rows[members[0]], "root": members[0]})
            continue
        U = frame(members, _dirs(rows[members[0]])[0])
        V = (-U[1], U[0])
        proj = {k: rows[k][0] * U[0] + rows[k][1] * U[1] for k in members}
        words = sorted(members, key=lambda k: (proj[k], k))
        for a, b in zip(words[:-1], words[1:]):
            if proj[a] != proj[b]:
                key_margin = min(key_margin, proj[b] - proj[a])
        pu, pv = [], []
        for k in members:
            cx, cy, w, h, _ = rows[k]
            u, v = _dirs(rows[k])
            for su in (0.5, -0.5):
                for sv in (0.5, -0.5):
                    px, py = cx + su * w * u[0] + sv * h * v[0], cy + su * w * u[1] + sv * h * v[1]
                    pu.append(px * U[0] + py * U[1]); pv.append(px * V[0] + py * V[1])
        cu, cv = (min(pu) + max(pu)) / 2, (min(pv) + max(pv)) / 2
        mx, my = cu * U[0] + cv * V[0], cu * U[1] + cv * V[1]
        good.append({"words": words, "box": [mx, my, max(pu) - min(pu), max(pv) - min(pv), math.degrees(math.atan2(-U[1], U[0]))],
                     "root": members[0], "key": (mx * PV[0] + my * PV[1], mx * PU[0] + my * PU[1], members[0])})
    good.sort(key=lambda ln: ln["key"])
    for a, b in zip(good[:-1], good[1:]):
        for ka, kb in zip(a["key"][:2], b["key"][:2]):
            if ka != kb:
                key_margin = min(key_margin, abs(kb - ka))
                break
    bad.sort(key=lambda ln: ln["root"])
    out = {"line_id": [0] * n, "line_pos": [0] * n, "order": [], "line_start": [], "line_boxes": [], "links": links,
           "valid": valid, "pair_margin": pair_margin, "key_margin": key_margin}
    for l, ln in enumerate(good + bad):
        out["line_start"].append(len(out["order"]))
        out["line_boxes"].append(ln["box"])
        for pos, k in enumerate(ln["words"]):
            out["line_id"][k], out["line_pos"][k] = l, pos
            out["order"].append(k)
    out["line_start"].append(n)
    out["line_count"] = len(good) + len(bad)
    return out


# ------------------------------------------------------------------------------------------------ scenes
def _f32(rows):
    return np.asarray(rows, dtype=np.float32).reshape(-1, 5)


def rotate_scene(rows, angle, origin=(0.0, 0.0)):
    """the page turned by `angle` degrees in the sense of the word angle: u = (1, 0) becomes (cos, -sin)"""
    t = math.radians(angle)
    c, s = math.cos(t), math.sin(t)
    out = []
    for cx, cy, w, h, a in rows:
        x, y = cx - origin[0], cy - origin[1]
        out.append([origin[0] + x * c + y * s, origin[1] - x * s + y * c, w, h, _wrap(a + angle)])
    return out


def paragraph(seed, n, angle=0.0, width=1000.0):
    """n words set in lines across a page `width` wide, some lines split in two by a wide gap, indices shuffled"""
    rng = np.random.RandomState(seed)
    rows, y = [], 40.0
    while len(rows) < n:
        h = rng.uniform(18, 30)
        x = rng.uniform(20, 120)
        while x < width and len(rows) < n:
            w = rng.uniform(20, 90)
            rows.append([x + w / 2, y + rng.uniform(-0.08, 0.08) * h, w, h * rng.uniform(0.9, 1.1), rng.uniform(-2, 2)])
            x += w + h * (rng.uniform(2.5, 4.0) if rng.uniform() < 0.08 else rng.uniform(0.25, 0.6))
        y += h * rng.uniform(1.9, 2.4)
    rows = rotate_scene(rows, angle, (width / 2, y / 2))
    return _f32([rows[k] for k in rng.permutation(n)])


def chain(seed, n):
    """one line of n words, indices shuffled"""
    rng = np.random.RandomState(seed)
    rows, x = [], 10.0
    for _ in range(n):
        w = rng.uniform(24, 36)
        rows.append([x + w / 2, 500 + rng.uniform(-1, 1), w, rng.uniform(19, 21), rng.uniform(-1, 1)])
        x += w + rng.uniform(4, 12)
    return _f32([rows[k] for k in rng.permutation(n)])


def singletons(seed, n):
    """n words that link with nothing, on a jittered grid"""
    rng = np.random.RandomState(seed)
    side = int(math.ceil(math.sqrt(n)))
    rows = [[200.0 * (k % side) + rng.uniform(-40, 40), 200.0 * (k // side) + rng.uniform(-40, 40), rng.uniform(30, 60),
             rng.uniform(15, 25), rng.uniform(-3, 3)] for k in range(n)]
    return _f32([rows[k] for k in rng.permutation(n)])


def opposite_lines():
    """two lines through the same pixels that read in opposite directions"""
    rows = [[50.0 * k, 100.0, 40.0, 20.0, 0.0] for k in range(9)]
    rows += [[50.0 * k + 0.25, 100.125, 40.0, 20.0, 180.0] for k in range(7)]
    return _f32([rows[k] for k in (9, 0, 10, 1, 11, 2, 12, 3, 13, 4, 14, 5, 15, 6, 7, 8)])


def bridge():
    """three words; the outer two link only through the middle one"""
    return _f32([[110.0, 50.0, 40.0, 20.0, 0.0], [0.0, 50.0, 40.0, 20.0, 0.0], [55.0, 50.0, 40.0, 20.0, 0.0]])


def arc(n, tilt=0.0, radius=200.0):
    """n equal words at 10 degree steps on a circle, each along the tangent turned by `tilt`"""
    rows = []
    for k in range(n):
        phi = math.radians(10.0 * k)
        rows.append([400.0 + radius * math.cos(phi), 400.0 + radius * math.sin(phi), 25.0, 20.0, _wrap(-10.0 * k - 90.0 + tilt)])
    return _f32(rows)


def identical(n):
    return _f32([[100.0, 100.0, 40.0, 20.0, 5.0]] * n)


def with_invalid(seed, n):
    """a paragraph with words that are no words between the others: NaN, inf, zero and negative extents"""
    rows = paragraph(seed, n).copy()
    nan, inf = float("nan"), float("inf")
    for k, (col, val) in zip(range(1, n, max(1, n // 9)), ((0, nan), (2, inf), (2, 0.0), (3, -3.0), (4, nan), (1, -inf), (3, 0.0),
                                                          (4, inf), (2, -1.0))):
        rows[k, col] = val
    return rows


def usable(ref):
    return ref["pair_margin"] >= MARGIN and ref["key_margin"] >= MARGIN


def generated(make, seed, *args):
    """the first scene of make(seed, ...), make(seed + 1, ...), ... whose margins allow it, with its reference"""
    for s in range(seed, seed + 8):
        boxes = make(s, *args)
        ref = reference(boxes)
        TALLY["tried"] += 1
        if usable(ref):
            return boxes, ref
        TALLY["rejected"] += 1
    raise AssertionError(f"no usable scene among 8 seeds from {seed}")


K_LIST = (0, 1, 2, 63, 64, 65, 129, 1023, 1024)


def _hand_made(boxes):
    ref = reference(boxes)
    assert usable(ref), (ref["pair_margin"], ref["key_margin"])
    return boxes, ref


_BUILDERS = {f"paragraph of {n}": (lambda n=n: generated(paragraph, 100 + n, n))
             for n in sorted({n for K in K_LIST for n in (K, K // 2)} - {0})}
_BUILDERS.update({
    "no words": lambda: _hand_made(np.zeros((0, 5), dtype=np.float32)),
    "paragraph at 30 degrees": lambda: generated(paragraph, 7, 300, 30.0),
    "paragraph at -170 degrees": lambda: generated(paragraph, 8, 300, -170.0),
    "one line of 1024": lambda: generated(chain, 9, 1024),
    "1024 singletons": lambda: generated(singletons, 10, 1024),
    "words that are no words": lambda: generated(with_invalid, 11, 60),
    "opposite lines": lambda: _hand_made(opposite_lines()),
    "bridge": lambda: _hand_made(bridge()),
    "arc of 120 degrees": lambda: _hand_made(arc(13)),
    "closed circle": lambda: _hand_made(arc(36, 3.75)),
    "identical boxes": lambda: _hand_made(identical(70)),
})
_BUILT = {}


def case(name):
    """(name, boxes float32 [n, 5], reference), built on first use and then shared unchanged"""
    if name not in _BUILT:
        _BUILT[name] = (name, *_BUILDERS[name]())
    return _BUILT[name]


def all_cases():
    """every case; prints and checks the tally of the seeds that the margins rejected"""
    cases = [case(name) for name in _BUILDERS]
    print(f"[line_group] seeds tried {TALLY['tried']}, rejected {TALLY['rejected']}")
    assert 8 * TALLY["rejected"] <= TALLY["tried"], TALLY
    return cases


def expected_padded(ref, K):
    """the reference's integer outputs padded to K as the kernel pads them"""
    n, L = len(ref["line_id"]), ref["line_count"]
    return {"line_id": ref["line_id"] + [-1] * (K - n), "line_pos": ref["line_pos"] + [-1] * (K - n),
            "order": ref["order"] + [-1] * (K - n), "line_start": ref["line_start"] + [n] * (K - L), "line_count": L}


def box_ulps(got_row, want_row):
    """distance in float32 units in the last place between a float32 row and a float64 row rounded to float32 (0 for equal
    bits, NaN included)"""
    g = np.asarray(got_row, dtype=np.float32)
    w = np.asarray(want_row, dtype=np.float64).astype(np.float32)
    same = g.view(np.uint32) == w.view(np.uint32)
    gi, wi = g.view(np.int32).astype(np.int64), w.view(np.int32).astype(np.int64)
    gi, wi = np.where(gi < 0, -(gi & 0x7fffffff), gi), np.where(wi < 0, -(wi & 0x7fffffff), wi)
    return int(np.where(same, 0, np.abs(gi - wi)).max())
