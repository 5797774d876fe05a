"""Float64 reference and case builders for glass_merge_views (csrc/view_merge.hip, include/glass_hip_ext_views.h).  Test
helper, not product code.

Reference.  `merge_ref` restates the six steps of the header's contract and is written from them, not from the kernel: it
starts from the float32 inputs, and only the frame transform of step 2 is replayed in numpy float32 (every product and sum
rounded separately), so that the output boxes can be compared bit for bit; corners, extents, the size band, the order and
the greedy cross-view suppression are float64, with detection_tail_cases' float64 rotated IoU.

Case builders.  The merge is discontinuous (an IoU threshold, the keep rectangle, the size band, the score order), so a case
is only usable when no decision sits closer to its boundary than float32 can resolve.  Every builder draws from a fixed seed
and redraws the offending rows until these margins hold, then asserts them; nothing is skipped or masked when results are
compared:
  IoU      |iou_f64 - nms_thresh| >= IOU_MARGIN (1e-3) for every cross-view pair of candidates that pass steps 1-3;
  border   every corner of such a candidate is >= 1e-3 px away from every finite side of its view's keep rectangle - and so
           is every corner of a candidate the rectangle drops;
  size     |size - lo| >= 1e-3 and |size - hi| >= 1e-3;
  scores   pairwise distinct, unless the case is about ties (tie values are exact float32 numbers).
"""
import functools
import math

import numpy as np

from detection_tail_cases import IOU_MARGIN, _jitter, _not_disjoint, iou_cached
from known_answers import box_corners

EDGE_MARGIN = 1e-3
INF = float("inf")
THRESH = 0.5
ALL = (-INF, -INF, INF, INF)


# ------------------------------------------------------------------------------------------------ reference
def frame_f32(box, xform):
    """step 2 in float32, every operation rounded on its own: the bits the kernel must produce"""
    b = np.asarray(box, dtype=np.float32)
    ox, oy, inv = (np.float32(v) for v in xform)
    with np.errstate(all="ignore"):
        return np.array([np.float32(b[0] * inv) + ox, np.float32(b[1] * inv) + oy, b[2] * inv, b[3] * inv, b[4]], dtype=np.float32)


def extents(gbox):
    c = np.asarray(box_corners(gbox), dtype=np.float64)
    return c[:, 0].min(), c[:, 1].min(), c[:, 0].max(), c[:, 1].max()


def candidates(boxes, scores, counts, xform, keep, band):
    """steps 1-3 -> list of dicts (v, s, score, g32, g (float64 of g32), ext, size), and the rows steps 1-2 passed but 3 dropped"""
    V, K = scores.shape
    boxes, scores = np.asarray(boxes, dtype=np.float32), np.asarray(scores, dtype=np.float32)
    keep, band = np.asarray(keep, dtype=np.float32).astype(np.float64), np.asarray(band, dtype=np.float32).astype(np.float64)
    passed, dropped = [], []
    for v in range(V):
        for s in range(min(max(int(counts[v]), 0), K)):
            if not (np.isfinite(scores[v, s]) and np.isfinite(boxes[v, s]).all()):
                continue
            g32 = frame_f32(boxes[v, s], xform[v])
            g = g32.astype(np.float64)
            if not (g[2] > 0 and g[3] > 0):
                continue
            x0, y0, x1, y1 = extents(g)
            size = max(x1 - x0, y1 - y0)
            c = dict(v=v, s=s, score=float(scores[v, s]), g32=g32, g=g, ext=(x0, y0, x1, y1), size=size)
            ok = keep[v, 0] <= x0 and x1 <= keep[v, 2] and keep[v, 1] <= y0 and y1 <= keep[v, 3] and band[v, 0] < size <= band[v, 1]
            (passed if ok else dropped).append(c)
    return passed, dropped


def _near(c, G, R):
    """indices of the rows of G (float64 boxes) whose circumscribed circle is not disjoint from that of candidate box c"""
    if len(G) == 0:
        return np.zeros((0,), dtype=np.int64)
    dx, dy = G[:, 0] - c[0], G[:, 1] - c[1]
    return np.nonzero(_not_disjoint(dx * dx + dy * dy, R + 0.5 * math.hypot(c[2], c[3])))[0]


def merge_ref(boxes, scores, counts, xform, keep, band, nms_thresh, max_out):
    """-> dict: src [n] int, boxes [n,5] float32 (the bits), scores [n] float32, count n, flag 0/1"""
    V, K = scores.shape
    cands, _ = candidates(boxes, scores, counts, xform, keep, band)
    cands.sort(key=lambda c: (-c["score"], c["v"], c["s"]))          # step 4 (-0.0 and 0.0 compare equal)
    kept, KG, KR, KV = [], np.zeros((0, 5)), np.zeros((0,)), np.zeros((0,), dtype=np.int64)
    flag = 0
    for pos, c in enumerate(cands):                                   # step 5
        near = _near(c["g"], KG, KR)
        if any(KV[i] != c["v"] and iou_cached(KG[i], c["g"]) >= nms_thresh for i in near):
            continue
        kept.append(c)
        KG = np.concatenate([KG, c["g"][None]])
        KR = np.append(KR, 0.5 * math.hypot(c["g"][2], c["g"][3]))
        KV = np.append(KV, c["v"])
        if len(kept) == max_out:
            flag = int(pos + 1 < len(cands))
            break
    return dict(src=np.array([c["v"] * K + c["s"] for c in kept], dtype=np.int32),
                boxes=np.array([c["g32"] for c in kept], dtype=np.float32).reshape(-1, 5),
                scores=np.array([c["score"] for c in kept], dtype=np.float32), count=len(kept), flag=flag,
                candidates=len(cands))


def margin_violations(case, ties=False):
    """the rows (v, s) that sit too close to a decision: see the module docstring"""
    passed, dropped = candidates(case["boxes"], case["scores"], case["counts"], case["xform"], case["keep"], case["band"])
    keep, band = np.asarray(case["keep"], dtype=np.float64), np.asarray(case["band"], dtype=np.float64)
    bad = set()
    for c in passed + dropped:
        v = c["v"]
        x0, y0, x1, y1 = c["ext"]
        sides = ((keep[v, 0], (x0, x1)), (keep[v, 2], (x0, x1)), (keep[v, 1], (y0, y1)), (keep[v, 3], (y0, y1)))
        if any(np.isfinite(k) and min(abs(k - e[0]), abs(k - e[1])) < EDGE_MARGIN for k, e in sides):
            bad.add((v, c["s"]))
        if any(np.isfinite(t) and abs(c["size"] - t) < EDGE_MARGIN for t in band[v]):
            bad.add((v, c["s"]))
    if passed:
        G = np.array([c["g"] for c in passed])
        R = 0.5 * np.hypot(G[:, 2], G[:, 3])
        views = np.array([c["v"] for c in passed])
        for j, c in enumerate(passed):
            for i in _near(c["g"], G[:j], R[:j]):
                if views[i] != c["v"] and abs(iou_cached(G[i], c["g"]) - case["nms_thresh"]) < IOU_MARGIN:
                    bad.add((c["v"], c["s"]))
    if not ties:
        sc = {}
        for c in passed + dropped:
            sc.setdefault(np.float32(c["score"]).tobytes(), []).append((c["v"], c["s"]))
        for rows in sc.values():
            if len(rows) > 1:
                bad.update(rows[1:])
    return sorted(bad)


class Builder:
    """rows are recipes: put(v, draw) appends a slot to view v whose box is draw(g) -> GLOBAL box, stored in the view's own
    pixels; settle() redraws the rows margin_violations names (and their scores, unless given) until none is left"""

    def __init__(self, seed, V, K, xform, keep, band, nms_thresh=THRESH, max_out=1024):
        self.g = np.random.default_rng(seed)
        self.V, self.K = V, K
        self.xform = np.asarray(xform, dtype=np.float32).reshape(V, 3)
        self.keep = np.asarray(keep, dtype=np.float32).reshape(V, 4)
        self.band = np.asarray(band, dtype=np.float32).reshape(V, 2)
        self.boxes = np.zeros((V, K, 5), dtype=np.float32)
        self.scores = np.zeros((V, K), dtype=np.float32)
        self.fill = [0] * V
        self.recipes, self.fixed_score = {}, set()
        self.nms_thresh, self.max_out = nms_thresh, max_out

    def to_view(self, v, gbox):
        ox, oy, inv = (float(t) for t in self.xform[v])
        b = np.asarray(gbox, dtype=np.float64)
        return np.array([(b[0] - ox) / inv, (b[1] - oy) / inv, b[2] / inv, b[3] / inv, b[4]], dtype=np.float32)

    def put(self, v, draw, score=None, raw=False):
        s = self.fill[v]
        assert s < self.K, (v, s)
        self.fill[v] += 1
        self.recipes[(v, s)] = (draw, raw)
        self._draw(v, s)
        if score is not None:
            self.scores[v, s] = score
            self.fixed_score.add((v, s))
        return s

    def _draw(self, v, s):
        draw, raw = self.recipes[(v, s)]
        b = draw(self.g)
        self.boxes[v, s] = np.asarray(b, dtype=np.float32) if raw else self.to_view(v, b)

    def case(self, counts=None, ties=False, rounds=60):
        free = [(v, s) for v in range(self.V) for s in range(self.fill[v]) if (v, s) not in self.fixed_score]
        vals = self.g.permutation(np.linspace(0.05, 0.95, max(len(free), 1))).astype(np.float32)
        for (v, s), x in zip(free, vals):
            self.scores[v, s] = x
        case = dict(boxes=self.boxes, scores=self.scores, counts=np.array(self.fill if counts is None else counts, dtype=np.int32),
                    xform=self.xform, keep=self.keep, band=self.band, nms_thresh=self.nms_thresh, max_out=self.max_out,
                    V=self.V, K=self.K)
        for _ in range(rounds):
            bad = margin_violations(case, ties)
            if not bad:
                break
            for v, s in bad:
                self._draw(v, s)
                if (v, s) not in self.fixed_score:
                    self.scores[v, s] = np.float32(self.g.uniform(0.05, 0.95))
        assert margin_violations(case, ties) == [], "margins not reached"
        case["ref"] = merge_ref(case["boxes"], case["scores"], case["counts"], case["xform"], case["keep"], case["band"],
                                case["nms_thresh"], case["max_out"])
        return case


def word(g, cx, cy, wr=(14.0, 30.0), hr=(6.0, 12.0), angle=None):
    return np.array([cx, cy, g.uniform(*wr), g.uniform(*hr), g.uniform(-20, 20) if angle is None else angle], dtype=np.float64)


def grid_centres(n, pitch, cols, x0=40.0, y0=40.0):
    return [(x0 + pitch * (i % cols), y0 + pitch * (i // cols)) for i in range(n)]


def jit(base):
    return lambda g: _jitter(g, base).astype(np.float64)


# ------------------------------------------------------------------------------------------------ cases
@functools.lru_cache(maxsize=None)
def one_view_identity():
    b = Builder(1, 1, 100, [[0, 0, 1]], [ALL], [[-INF, INF]])
    for i, (cx, cy) in enumerate(grid_centres(37, 45.0, 8)):
        b.put(0, (lambda c: lambda g: word(g, *c))((cx, cy)), score=np.float32(0.99 - 0.02 * i))     # descending: the order is the slots'
    return b.case()


@functools.lru_cache(maxsize=None)
def two_views_duplicates():
    """two tiles side by side, 40 words in their overlap, a jittered copy of each in both views (in the view's pixels)"""
    b = Builder(2, 2, 64, [[0, 0, 1], [96, 0, 1]], [ALL, ALL], [[-INF, INF]] * 2)
    for cx, cy in grid_centres(40, 42.0, 4, x0=120.0, y0=30.0):
        base = word(b.g, cx, cy)
        for v in (0, 1):
            b.put(v, jit(base))
    case = b.case()
    case["words"] = 40
    return case


@functools.lru_cache(maxsize=None)
def same_view_pairs():
    """IoU ~0.9 pairs inside view 0 (both halves must stay), unrelated words in view 1"""
    b = Builder(3, 2, 32, [[0, 0, 1], [0, 0, 1]], [ALL, ALL], [[-INF, INF]] * 2)
    for cx, cy in grid_centres(12, 60.0, 4):
        base = word(b.g, cx, cy)
        b.put(0, lambda g, base=base: base)
        b.put(0, jit(base))
    for cx, cy in grid_centres(10, 60.0, 4, x0=400.0):
        b.put(1, (lambda c: lambda g: word(g, *c))((cx, cy)))
    case = b.case()
    case["pairs"] = 12
    return case


GRID = dict(size=288, tile=128, overlap=48, border=4, rho=0.5)
GRID_ANGLES = (0.0, 90.0, -90.0, 180.0, -180.0)


@functools.lru_cache(maxsize=None)
def grid_3x3_plus_full():
    """a 3 x 3 plan of 128-pixel tiles over 288 x 288 (L = 40) plus the whole image at half resolution.  Every word goes, as a
    jittered copy, to every tile that contains it whole and to the full view; a tile that cuts a word gets the fragment it
    would see - the axis-aligned part inside the tile, which touches the tile's edge."""
    from glass_amd.inference.tiling import plan_tiles
    S = GRID["size"]
    plan = plan_tiles(S, S, GRID["tile"], GRID["overlap"], GRID["border"])
    assert len(plan.tiles) == 9 and plan.max_whole == 40
    L = float(plan.max_whole)
    xform = [[t.x0, t.y0, 1.0] for t in plan.tiles] + [[0, 0, 1.0 / GRID["rho"]]]
    keep = [list(t.keep) for t in plan.tiles] + [list(ALL)]
    band = [[-INF, L]] * 9 + [[L, INF]]
    b = Builder(4, 10, 100, xform, keep, band)
    g = b.g
    words = []
    # cores of the tiles (seen by one tile), overlaps of two and of four tiles, the image's edges, and words larger than L
    for cx, cy in ((40, 40), (144, 40), (250, 44), (40, 144), (144, 144), (248, 144), (40, 250), (144, 250), (250, 250)):
        words.append(("core", word(g, cx + g.uniform(-6, 6), cy + g.uniform(-6, 6), wr=(14, 28), hr=(6, 10))))
    for cx, cy in ((104, 30), (184, 60), (104, 144), (184, 230), (30, 104), (60, 184), (144, 104), (250, 184)):
        words.append(("two", word(g, cx + g.uniform(-3, 3), cy + g.uniform(-3, 3), wr=(12, 20), hr=(6, 9))))
    for cx, cy in ((104, 104), (184, 104), (104, 184), (184, 184)):
        words.append(("four", word(g, cx + g.uniform(-3, 3), cy + g.uniform(-3, 3), wr=(12, 18), hr=(6, 9))))
    for cx, cy in ((12, 60), (276, 200), (150, 5), (60, 283)):
        words.append(("edge", word(g, cx, cy, wr=(14, 20), hr=(6, 8), angle=g.uniform(-5, 5))))
    for cx, cy in ((70, 222), (200, 24), (224, 110), (130, 70)):
        words.append(("large", word(g, cx, cy, wr=(60, 100), hr=(10, 16))))
    for i, a in enumerate(GRID_ANGLES):
        words.append(("angle", word(g, 30 + 50 * i, 208, wr=(16, 24), hr=(6, 9), angle=a)))
    n_rows = {"whole": 0, "fragment": 0}
    for kind, w in words:
        x0, y0, x1, y1 = extents(w)
        for v, t in enumerate(plan.tiles):
            tx0, ty0, tx1, ty1 = t.x0, t.y0, t.x0 + t.w, t.y0 + t.h
            if tx0 <= x0 - 1 and x1 + 1 <= tx1 and ty0 <= y0 - 1 and y1 + 1 <= ty1:
                b.put(v, jit(w))
                n_rows["whole"] += 1
                continue
            ix0, iy0, ix1, iy1 = max(x0, tx0), max(y0, ty0), min(x1, tx1), min(y1, ty1)
            if ix1 - ix0 >= 6 and iy1 - iy0 >= 4:
                frag = np.array([(ix0 + ix1) / 2, (iy0 + iy1) / 2, ix1 - ix0, iy1 - iy0, 0.0])
                # (the side on the tile's edge stays there; the free sides move a little when the row is redrawn)
                b.put(v, lambda g, f=frag, e=(ix0 == tx0, iy0 == ty0, ix1 == tx1, iy1 == ty1): _fragment(g, f, e))
                n_rows["fragment"] += 1
        b.put(9, jit(w))
    case = b.case()
    case["rows"], case["words"] = n_rows, words
    return case


def _fragment(g, f, on_edge):
    x0, y0, x1, y1 = f[0] - f[2] / 2, f[1] - f[3] / 2, f[0] + f[2] / 2, f[1] + f[3] / 2
    x0 += 0 if on_edge[0] else g.uniform(-0.5, 0.5)
    y0 += 0 if on_edge[1] else g.uniform(-0.5, 0.5)
    x1 += 0 if on_edge[2] else g.uniform(-0.5, 0.5)
    y1 += 0 if on_edge[3] else g.uniform(-0.5, 0.5)
    return np.array([(x0 + x1) / 2, (y0 + y1) / 2, x1 - x0, y1 - y0, 0.0])


TIE_VALUES = (0.75, 0.5, 0.125, 0.0, -0.0, -0.25)


@functools.lru_cache(maxsize=None)
def ties():
    """equal scores across three views and inside them: unrelated words (all stay, ordered by view, then slot) and, for each
    value, one word that views 0 and 2 both hold with that same score (the copy of view 0 stays)"""
    b = Builder(5, 3, 24, [[0, 0, 1]] * 3, [ALL] * 3, [[-INF, INF]] * 3)
    centres = iter(grid_centres(60, 50.0, 10))
    for val in TIE_VALUES:
        for v in (2, 0, 1, 0):
            b.put(v, (lambda c: lambda g: word(g, *c))(next(centres)), score=np.float32(val))
        base = word(b.g, *next(centres))
        for v in (2, 0):
            b.put(v, jit(base), score=np.float32(val))
    return b.case(ties=True)


CHUNK_TOTALS = ((64, 63), (64, 64), (65, 63), (65, 64), (65, 65))       # (candidates, survivors)


@functools.lru_cache(maxsize=None)
def chunks(cands, survivors):
    dups = cands - survivors
    b = Builder(600 + cands * 10 + survivors, 2, 64, [[0, 0, 1], [10, 20, 1]], [ALL] * 2, [[-INF, INF]] * 2)
    for i, (cx, cy) in enumerate(grid_centres(survivors, 50.0, 10, x0=60.0, y0=60.0)):
        base = word(b.g, cx, cy)
        if i < dups:
            b.put(0, jit(base))
            b.put(1, jit(base))
        else:
            b.put(i % 2, jit(base))
    case = b.case()
    assert case["ref"]["candidates"] == cands and case["ref"]["count"] == survivors
    return case


def _cap(seed, words, dups, counts_of):
    """V = 8, K = 1024: `words` distinct words on a 40-pixel grid (circumscribed circles of different words are disjoint), the
    first `dups` of them also as a jittered copy in another view"""
    V, K = 8, 1024
    b = Builder(seed, V, K, [[0, 0, 1]] * V, [ALL] * V, [[-INF, INF]] * V)
    rows = []
    for i, (cx, cy) in enumerate(grid_centres(words, 40.0, 100)):
        base = word(b.g, cx, cy, wr=(14, 28), hr=(6, 10))
        rows.append(base)
        if i < dups:
            rows.append(base)
    for i, base in enumerate(rows):
        v = counts_of(i)
        b.put(v, jit(base))
    return b


@functools.lru_cache(maxsize=None)
def cap_full():
    """8192 slots, all used; 7000 words, 1192 of them twice: far more than 1024 survivors, so the first 1024 come out, flag 1"""
    b = _cap(7, 7000, 1192, lambda i: i % 8)
    assert b.fill == [1024] * 8
    case = b.case()
    assert case["ref"]["count"] == 1024 and case["ref"]["flag"] == 1
    return case


@functools.lru_cache(maxsize=None)
def cap_exact():
    """1024 words, 100 of them twice, and the lowest score of all on a word held once: exactly 1024 survivors, the last of
    them the last candidate of the order, flag 0"""
    b = _cap(8, 1024, 100, lambda i: i % 8)
    v, s = 7, b.fill[7] - 1                  # (row 1123 = word 1023, held once)
    b.scores[v, s] = np.float32(0.01)
    b.fixed_score.add((v, s))
    case = b.case()
    assert case["ref"]["candidates"] == 1124 and case["ref"]["count"] == 1024 and case["ref"]["flag"] == 0
    assert case["ref"]["src"][-1] == v * 1024 + s
    return case


@functools.lru_cache(maxsize=None)
def deep_duplicates():
    """400 words, each held by all 8 views: 3200 candidates in 50 chunks, 400 survivors - most chunks meet several hundred kept
    boxes of other views, and seven of every eight candidates are suppressed"""
    V, K = 8, 512
    b = Builder(11, V, K, [[3 * v, 2 * v, 1] for v in range(V)], [ALL] * V, [[-INF, INF]] * V)
    for cx, cy in grid_centres(400, 40.0, 20, x0=60.0, y0=60.0):
        base = word(b.g, cx, cy, wr=(14, 28), hr=(6, 10))
        for v in range(V):
            b.put(v, jit(base))
    case = b.case()
    assert case["ref"]["candidates"] == 3200 and case["ref"]["count"] == 400
    return case


@functools.lru_cache(maxsize=None)
def counts_edges():
    """counts 0, negative, above K (clamped to K) and ordinary; every slot of every view holds a usable word"""
    b = Builder(9, 4, 8, [[0, 0, 1]] * 4, [ALL] * 4, [[-INF, INF]] * 4)
    centres = iter(grid_centres(32, 50.0, 8))
    for v in range(4):
        for _ in range(8):
            b.put(v, (lambda c: lambda g: word(g, *c))(next(centres)))
    case = b.case(counts=[0, -3, 20, 5])
    assert case["ref"]["count"] == 13
    return case


@functools.lru_cache(maxsize=None)
def nonfinite_and_empty():
    """NaN / inf in the score and in each box field, w == 0, h < 0 among ordinary words of two views"""
    b = Builder(10, 2, 24, [[5, 7, 1]] * 2, [ALL] * 2, [[-INF, INF]] * 2)
    centres = iter(grid_centres(48, 50.0, 8))
    rubbish = []
    for v in range(2):
        for i in range(20):
            s = b.put(v, (lambda c: lambda g: word(g, *c))(next(centres)))
            if i % 2 == 1:
                rubbish.append((v, s))
    case = b.case()
    bad = (np.nan, np.inf, -np.inf)
    for n, (v, s) in enumerate(rubbish):
        if n < 3:
            case["scores"][v, s] = bad[n]
        elif n < 3 + 10:
            case["boxes"][v, s, (n - 3) % 5] = bad[(n - 3) % 3] if n - 3 < 5 else bad[(n - 3 + 1) % 3]
        elif n == 13:
            case["boxes"][v, s, 2] = 0.0
        elif n == 14:
            case["boxes"][v, s, 3] = -4.0
        elif n == 15:
            case["boxes"][v, s, 2] = -0.0
    assert margin_violations(case) == []
    case["ref"] = merge_ref(case["boxes"], case["scores"], case["counts"], case["xform"], case["keep"], case["band"],
                            case["nms_thresh"], case["max_out"])
    assert case["ref"]["count"] == 40 - 16
    return case
