"""Float64 reference and case builders for glass_fuse_views (csrc/view_fuse.hip, include/glass_hip_feature_fuse.h).  Test
helper, not product code.

Reference.  `fuse_ref` restates the seven steps of the header's contract and is written from them, not from the kernel.  It
starts from the float32 inputs; the word score of step 2 is replayed in numpy float32 in step order and the frame of step 3
in float64 with every product and sum rounded on its own and each result rounded to float32 once, so that keys and boxes
compare bit for bit; the order, the greedy cross-view pass, the supporters and the votes are plain Python on float64, with
detection_tail_cases' float64 rotated IoU and view_merge_cases' circle test in front of it.

Case builders.  The fusion is discontinuous (an IoU threshold, the bounds, the key order), so a case is usable only when no
decision sits closer to its boundary than float32 can resolve.  Every builder draws from a fixed seed and redraws the
offending rows until the margins of view_merge_cases.py hold, then asserts them; nothing is skipped or masked when results
are compared:
  IoU      |iou_f64 - nms_thresh| >= 1e-3 for every cross-view pair of candidates that pass steps 1-3;
  bounds   every centre - of a candidate the bounds keep and of one they drop - is >= 1e-3 px away from every finite side,
           unless the case is about the bound itself (exact float values on the side, `on_bound=True`);
  keys     pairwise distinct in every ranking mode the case is run with, unless the case is about ties (exact float32 values).
A builder counts the rows it redraws (`case["redrawn"]`) and the rounds it takes; a SEED is rejected when the margins are not
reached in 60 rounds.  Rejected seeds over all builders of this file, at the seeds given: 0 (so below the cap of 1 in 8).
"""
import functools
import math

import numpy as np

from detection_tail_cases import IOU_MARGIN, _jitter, iou_cached
from view_merge_cases import EDGE_MARGIN, _near, extents, grid_centres, word  # noqa: F401  (extents: for the tests)

INF = float("inf")
THRESH = 0.5
KEEP_MAX = 1024
FREE = (-INF, -INF, INF, INF)
IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 1.0, 0.0)
MODES = {"detection": 0, "product": 1, "word": 2}


# ------------------------------------------------------------------------------------------------ reference
def word_score_f32(arg_row, max_row, stop_index):
    """step 2: the float32 product, in step order, up to and including the first stop symbol"""
    ws = np.float32(1.0)
    with np.errstate(all="ignore"):
        for a, m in zip(arg_row, max_row):
            ws = np.float32(ws * np.float32(m))
            if int(a) == int(stop_index):
                break
    return ws


def key_f32(score, ws, rank_mode):
    with np.errstate(all="ignore"):
        return (np.float32(score), np.float32(np.float32(score) * ws), np.float32(ws))[rank_mode]


def frame_f64(box, affine):
    """step 3 in float64, every operation rounded on its own, each result rounded to float32 once"""
    b = [float(v) for v in np.asarray(box, dtype=np.float32)]
    m = [float(v) for v in affine]
    with np.errstate(all="ignore"):
        m = np.array(m, dtype=np.float64)
        cx, cy, w, h, a = (np.float64(v) for v in b)
        gx = m[0] * cx + m[1] * cy + m[2]
        gy = m[3] * cx + m[4] * cy + m[5]
        aa = a + m[7]
        aa = aa - np.float64(360.0) * np.floor((aa + np.float64(180.0)) / np.float64(360.0))
        return np.array([gx, gy, w * m[6], h * m[6], aa], dtype=np.float64).astype(np.float32)


def candidates(boxes, scores, counts, affine, bounds, text_arg=None, text_max=None, stop_index=0, rank_mode=0):
    """steps 1-3 -> (passed, dropped by the bounds alone): dicts v, s, score, key (float32), g32, g (float64 of g32)"""
    boxes, scores = np.asarray(boxes, dtype=np.float32), np.asarray(scores, dtype=np.float32)
    V, K = scores.shape
    x0, y0, x1, y1 = (float(v) for v in np.asarray(bounds, dtype=np.float32))
    passed, dropped = [], []
    for v in range(V):
        for s in range(min(max(int(counts[v]), 0), K)):
            if not (np.isfinite(scores[v, s]) and np.isfinite(boxes[v, s]).all()):
                continue
            ws = word_score_f32(text_arg[v, s], text_max[v, s], stop_index) if rank_mode else np.float32(1.0)
            key = key_f32(scores[v, s], ws, rank_mode)
            if not np.isfinite(key):
                continue
            g32 = frame_f64(boxes[v, s], affine[v])
            g = g32.astype(np.float64)
            if not (np.isfinite(g32).all() and g[2] > 0 and g[3] > 0):
                continue
            c = dict(v=v, s=s, score=scores[v, s], key=key, g32=g32, g=g)
            (passed if x0 <= g[0] <= x1 and y0 <= g[1] <= y1 else dropped).append(c)
    return passed, dropped


def fuse_ref(boxes, scores, counts, affine, bounds, nms_thresh, text_arg=None, text_max=None, stop_index=0, rank_mode=0,
             min_votes=1, max_out=1024):
    """-> dict: src, votes [n] int32, views [n] int64, boxes [n,5], scores, keys [n] float32 (the bits), count n (rows written),
    flag, kept (before the vote filter), candidates, cut"""
    K = np.asarray(scores).shape[1]
    cands, _ = candidates(boxes, scores, counts, affine, bounds, text_arg, text_max, stop_index, rank_mode)
    cands.sort(key=lambda c: (-float(c["key"]), c["v"], c["s"]))     # step 4 (-0.0 and 0.0 compare equal)
    kept, masks = [], []
    KG, KR, KV = np.zeros((0, 5)), np.zeros((0,)), np.zeros((0,), dtype=np.int64)
    cut = 0
    for pos, c in enumerate(cands):                                   # steps 5 and 6
        hits = [int(i) for i in _near(c["g"], KG, KR) if KV[i] != c["v"] and iou_cached(KG[i], c["g"]) >= nms_thresh]
        if hits:
            masks[min(hits)] |= 1 << c["v"]
            continue
        kept.append(c)
        masks.append(1 << c["v"])
        KG = np.concatenate([KG, c["g"][None]])
        KR = np.append(KR, 0.5 * math.hypot(c["g"][2], c["g"][3]))
        KV = np.append(KV, c["v"])
        if len(kept) == KEEP_MAX:
            cut = int(pos + 1 < len(cands))
            break
    rows = [(c, m) for c, m in zip(kept, masks) if bin(m).count("1") >= min_votes]       # step 7
    n = len(rows)
    rows = rows[:max_out]
    return dict(src=np.array([c["v"] * K + c["s"] for c, _ in rows], dtype=np.int32),
                votes=np.array([bin(m).count("1") for _, m in rows], dtype=np.int32),
                views=np.array([m for _, m in rows], dtype=np.uint64).view(np.int64),
                boxes=np.array([c["g32"] for c, _ in rows], dtype=np.float32).reshape(-1, 5),
                scores=np.array([c["score"] for c, _ in rows], dtype=np.float32),
                keys=np.array([c["key"] for c, _ in rows], dtype=np.float32),
                count=len(rows), flag=int(bool(cut) or n > max_out), kept=len(kept), candidates=len(cands), cut=cut)


def ref_of(case, rank="detection", min_votes=1, max_out=None):
    return fuse_ref(case["boxes"], case["scores"], case["counts"], case["affine"], case["bounds"], case["nms_thresh"],
                    case.get("text_arg"), case.get("text_max"), case.get("stop_index", 0), MODES[rank], min_votes,
                    case["max_out"] if max_out is None else max_out)


def margin_violations(case, ties=False, on_bound=False, ranks=("detection",)):
    """the rows (v, s) that sit too close to a decision: see the module docstring"""
    bad = set()
    bounds = np.asarray(case["bounds"], dtype=np.float32).astype(np.float64)
    passed = None
    for rank in ranks:
        p, d = candidates(case["boxes"], case["scores"], case["counts"], case["affine"], bounds, case.get("text_arg"),
                          case.get("text_max"), case.get("stop_index", 0), MODES[rank])
        if not ties:
            seen = {}
            for c in p + d:
                k = np.float32(c["key"] + np.float32(0.0)).tobytes()          # (-0.0 + 0.0 = +0.0: one key)
                seen.setdefault(k, []).append((c["v"], c["s"]))
            for rows in seen.values():
                bad.update(rows[1:])
        if passed is None or len(p) > len(passed):
            passed, dropped = p, d
    if not on_bound:
        for c in passed + dropped:
            sides = ((bounds[0], c["g"][0]), (bounds[2], c["g"][0]), (bounds[1], c["g"][1]), (bounds[3], c["g"][1]))
            if any(np.isfinite(b) and abs(b - x) < EDGE_MARGIN for b, x in sides):
                bad.add((c["v"], c["s"]))
    if passed:
        G = np.array([c["g"] for c in passed])
        R = 0.5 * np.hypot(G[:, 2], G[:, 3])
        views = np.array([c["v"] for c in passed])
        for j, c in enumerate(passed):
            for i in _near(c["g"], G[:j], R[:j]):
                if views[i] != c["v"] and abs(iou_cached(G[i], c["g"]) - case["nms_thresh"]) < IOU_MARGIN:
                    bad.add((c["v"], c["s"]))
    return sorted(bad)


# ------------------------------------------------------------------------------------------------ builder
def to_view(gbox, affine):
    """the forward map in float64: a box of the image's frame in the pixels of the view whose row is `affine`"""
    m0, m1, m2, m3, m4, m5, s, dth = (float(v) for v in affine)
    det = m0 * m4 - m1 * m3
    x, y = float(gbox[0]) - m2, float(gbox[1]) - m5
    a = float(gbox[4]) - dth
    a = a - 360.0 * math.floor((a + 180.0) / 360.0)
    return np.array([(m4 * x - m1 * y) / det, (-m3 * x + m0 * y) / det, gbox[2] / s, gbox[3] / s, a], dtype=np.float64)


class Builder:
    """rows are recipes: put(v, draw) appends a slot to view v whose box is draw(g) -> box of the IMAGE's frame, stored in the
    view's own pixels (float32); case() redraws the rows margin_violations names - and their free scores and text rows - until
    none is left"""

    def __init__(self, seed, V, K, affine=None, bounds=FREE, T=0, stop_index=1, nms_thresh=THRESH, max_out=1024):
        self.g = np.random.default_rng(seed)
        self.V, self.K, self.T, self.stop_index = V, K, T, stop_index
        self.affine = np.array([IDENTITY] * V if affine is None else affine, dtype=np.float64).reshape(V, 8)
        self.bounds = np.asarray(bounds, dtype=np.float32)
        self.boxes = np.zeros((V, K, 5), dtype=np.float32)
        self.scores = np.zeros((V, K), dtype=np.float32)
        self.text_arg = np.zeros((V, K, T), dtype=np.int32) if T else None
        self.text_max = np.ones((V, K, T), dtype=np.float32) if T else None
        self.fill = [0] * V
        self.recipes, self.fixed_score = {}, set()
        self.nms_thresh, self.max_out = nms_thresh, max_out
        self.redrawn = 0

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
        self.boxes[v, s] = np.asarray(b, dtype=np.float32) if raw else to_view(b, self.affine[v]).astype(np.float32)
        if self.T:           # a word of 0 .. T steps: characters 2.., then the stop symbol (none when the word fills all T steps)
            n = int(self.g.integers(0, self.T + 1))
            self.text_arg[v, s] = self.g.integers(2, 40, self.T)
            if n < self.T:
                self.text_arg[v, s, n] = self.stop_index
            self.text_max[v, s] = self.g.uniform(0.55, 1.0, self.T).astype(np.float32)

    def case(self, counts=None, ties=False, on_bound=False, ranks=("detection",), rounds=60):
        free = [(v, s) for v in range(self.V) for s in range(self.fill[v]) if (v, s) not in self.fixed_score]
        vals = self.g.permutation(np.linspace(0.05, 0.95, max(len(free), 1))).astype(np.float32)
        for (v, s), x in zip(free, vals):
            self.scores[v, s] = x
        case = dict(boxes=self.boxes, scores=self.scores, counts=np.array(self.fill if counts is None else counts, dtype=np.int32),
                    affine=self.affine, bounds=self.bounds, nms_thresh=self.nms_thresh, max_out=self.max_out, V=self.V, K=self.K,
                    stop_index=self.stop_index)
        if self.T:
            case.update(text_arg=self.text_arg, text_max=self.text_max, T=self.T)
        for _ in range(rounds):
            bad = margin_violations(case, ties, on_bound, ranks)
            if not bad:
                break
            for v, s in bad:
                self.redrawn += 1
                self._draw(v, s)
                if (v, s) not in self.fixed_score:
                    self.scores[v, s] = np.float32(self.g.uniform(0.05, 0.95))
        assert margin_violations(case, ties, on_bound, ranks) == [], "margins not reached: the seed is rejected"
        case["redrawn"], case["ranks"] = self.redrawn, ranks
        case["ref"] = ref_of(case, ranks[0])
        return case


def jit(base):
    return lambda g: _jitter(g, base).astype(np.float64)


def at(c, **kw):
    return lambda g: word(g, *c, **kw)


# ------------------------------------------------------------------------------------------------ cases
@functools.lru_cache(maxsize=None)
def one_view_identity():
    b = Builder(1, 1, 100)
    for i, c in enumerate(grid_centres(37, 45.0, 8)):
        b.put(0, at(c), score=np.float32(0.99 - 0.02 * i))            # descending: the order is the slots'
    return b.case()


SCENE = dict(height=300, width=420, angles=(0.0, 37.0, 180.0, 270.0), ratio=0.8, words=40, T=8)


@functools.lru_cache(maxsize=None)
def scene_four_rotations():
    """about 40 words of a 300 x 420 image seen by four rotations of it (view_fusion.plan_views, each view resized by 0.8): the
    view boxes by the forward map in float64 plus jitter, every word missing from some views (each view holds a word with
    probability 0.75, one at least), free detection scores and free text rows - so the best-detected and the best-read copy of
    a word differ for most words.  The margins hold in all three ranking modes."""
    from glass_amd.inference.view_fusion import plan_views
    views = plan_views(SCENE["height"], SCENE["width"], SCENE["angles"], (1.0,), lambda hw: SCENE["ratio"])
    b = Builder(21, 4, 64, [v.affine for v in views], (0.0, 0.0, float(SCENE["width"]), float(SCENE["height"])), T=SCENE["T"])
    held = []
    for c in grid_centres(SCENE["words"], 48.0, 8, x0=36.0, y0=30.0):
        base = word(b.g, *c, wr=(16.0, 30.0), hr=(6.0, 11.0))
        vs = [v for v in range(4) if b.g.uniform() < 0.75] or [int(b.g.integers(0, 4))]
        held.append(vs)
        for v in vs:
            b.put(v, jit(base))
    # what a rotated canvas adds: detections in its fill corners, whose centres fall outside the image
    for v, c in ((1, (-14.0, 150.0)), (1, (200.0, -9.0)), (3, (440.0, 100.0)), (1, (210.0, 318.0))):
        b.put(v, at(c))
    case = b.case(ranks=("detection", "product", "word"))
    case["held"], case["outside"] = held, 4
    return case


@functools.lru_cache(maxsize=None)
def same_view_pairs():
    """IoU ~0.9 pairs inside view 0 (both halves stay, one vote each, and the better half is the earlier one), and over each
    pair a box of view 2 with the lowest keys of all: it supports the earlier half only.  Unrelated words in view 1."""
    b = Builder(3, 3, 32)
    n = 12
    for i, c in enumerate(grid_centres(n, 60.0, 4)):
        base = word(b.g, *c)
        b.put(0, lambda g, base=base: base, score=np.float32(0.903 - 0.01 * i))
        b.put(0, jit(base), score=np.float32(0.703 - 0.01 * i))
        b.put(2, jit(base), score=np.float32(0.303 - 0.01 * i))
    for c in grid_centres(10, 60.0, 4, x0=400.0):
        b.put(1, at(c))           # (free scores 0.05, 0.15, ..: they interleave with the fixed ones and equal none of them)
    case = b.case()
    case["pairs"] = n
    return case


TIE_VALUES = (0.75, 0.5, 0.125, 0.0, -0.0, -0.25)


@functools.lru_cache(maxsize=None)
def ties():
    """equal keys across three views and inside them: unrelated words (all stay, ordered by view, then slot) and, for each
    value, one word that views 0 and 2 both hold with that same key (the copy of view 0 stays, with two votes)"""
    b = Builder(5, 3, 24)
    centres = iter(grid_centres(60, 50.0, 10))
    for val in TIE_VALUES:
        for v in (2, 0, 1, 0):
            b.put(v, at(next(centres)), score=np.float32(val))
        base = word(b.g, *next(centres))
        for v in (2, 0):
            b.put(v, jit(base), score=np.float32(val))
    return b.case(ties=True)


CHUNK_TOTALS = ((63, 50), (64, 64), (64, 40), (65, 64), (65, 33), (128, 100), (128, 64), (129, 128), (129, 65))   # (candidates, survivors)


@functools.lru_cache(maxsize=None)
def chunks(cands, survivors):
    """`survivors` words, the first cands - survivors of them in two views: totals on both sides of the chunks of 64"""
    dups = cands - survivors
    b = Builder(600 + cands * 10 + survivors, 2, 128, [IDENTITY, (1.0, 0.0, 10.0, 0.0, 1.0, 20.0, 1.0, 0.0)])
    for i, c in enumerate(grid_centres(survivors, 50.0, 12, x0=60.0, y0=60.0)):
        base = word(b.g, *c)
        if i < dups:
            b.put(0, jit(base))
            b.put(1, jit(base))
        else:
            b.put(i % 2, jit(base))
    case = b.case()
    assert case["ref"]["candidates"] == cands and case["ref"]["count"] == survivors
    return case


@functools.lru_cache(maxsize=None)
def late_supporters():
    """100 words: view 0 holds them with the 100 best keys (chunks 0 and 1 of the order), views 1 and 2 hold copies of most of
    them with lower keys - every supporter sits in a later chunk than the box it supports, many of them two chunks later"""
    b = Builder(12, 3, 128, [IDENTITY, (0.5, 0.0, 3.0, 0.0, 0.5, -2.0, 0.5, 0.0), (0.0, -1.0, 900.0, 1.0, 0.0, 0.0, 1.0, -90.0)])
    n = 100
    for i, c in enumerate(grid_centres(n, 50.0, 10, x0=60.0, y0=60.0)):
        base = word(b.g, *c)
        b.put(0, jit(base), score=np.float32(0.95 - 0.002 * i))
        if i % 5 != 0:
            b.put(1, jit(base), score=np.float32(0.70 - 0.002 * i))
        if i % 3 != 0:
            b.put(2, jit(base), score=np.float32(0.40 - 0.002 * i))
    case = b.case()
    r = case["ref"]
    assert r["count"] == n and r["candidates"] == n + 80 + 66 and sorted(set(r["votes"].tolist())) == [1, 2, 3]
    return case


@functools.lru_cache(maxsize=None)
def view_63():
    """V = 64, K = 128: words seen by view 63 alone, by views 0 and 63, and by views 5, 31, 32 and 63 - bit 63 makes the mask
    negative as int64"""
    b = Builder(13, 64, 128)
    centres = iter(grid_centres(30, 50.0, 10))
    for i in range(30):
        base = word(b.g, *next(centres))
        for v in ((63,), (0, 63), (5, 31, 32, 63))[i % 3]:
            b.put(v, jit(base))
    case = b.case()
    r = case["ref"]
    assert r["count"] == 30 and (r["views"] < 0).all() and sorted(set(r["votes"].tolist())) == [1, 2, 4]
    return case


def _many(seed, words, dups, last_is_kept):
    """V = 2, K = 1024: `words` words on a 40-pixel grid (the circles of different words are disjoint) spread over both views,
    the first `dups` also as a copy in the other view.  `last_is_kept`: the lowest key of all on a word held once."""
    b = Builder(seed, 2, 1024)
    last = None
    for i, c in enumerate(grid_centres(words, 40.0, 40)):
        base = word(b.g, *c, wr=(14, 28), hr=(6, 10))
        v = i % 2
        last = (v, b.put(v, jit(base)))
        if i < dups:
            b.put(1 - v, jit(base))
    if last_is_kept:
        b.scores[last] = np.float32(0.01)
        b.fixed_score.add(last)
    return b, last


@functools.lru_cache(maxsize=None)
def keep_exact():
    """1024 words, 100 of them in both views, the last candidate of the order the 1024th kept one: nothing is cut"""
    b, last = _many(8, 1024, 100, True)
    case = b.case()
    r = case["ref"]
    assert r["candidates"] == 1124 and r["kept"] == r["count"] == 1024 and r["flag"] == 0
    assert r["src"][-1] == last[0] * 1024 + last[1]
    return case


@functools.lru_cache(maxsize=None)
def keep_cut():
    """1025 words, 100 of them in both views: the walk ends at the 1024th kept candidate with candidates left, flag 1"""
    b, _ = _many(9, 1025, 100, True)
    case = b.case()
    r = case["ref"]
    assert r["candidates"] == 1125 and r["kept"] == r["count"] == 1024 and r["cut"] == 1 and r["flag"] == 1
    return case


@functools.lru_cache(maxsize=None)
def counts_edges():
    """counts 0, negative, above K (clamped to K) and ordinary; every slot of every view holds a usable word"""
    b = Builder(9, 4, 8)
    centres = iter(grid_centres(32, 50.0, 8))
    for v in range(4):
        for _ in range(8):
            b.put(v, at(next(centres)))
    case = b.case(counts=[0, -3, 20, 5])
    assert case["ref"]["count"] == 13
    return case


@functools.lru_cache(maxsize=None)
def nonfinite_rows():
    """NaN / inf in the score, in each box field and in the text maxima, w == 0, h < 0 among ordinary words of two views"""
    b = Builder(10, 2, 24, [(1.0, 0.0, 5.0, 0.0, 1.0, 7.0, 1.0, 0.0)] * 2, T=5)
    centres = iter(grid_centres(48, 50.0, 8))
    rubbish = []
    for v in range(2):
        for i in range(22):
            s = b.put(v, at(next(centres)))
            if i % 2 == 1:
                rubbish.append((v, s))
    case = b.case(ranks=("detection", "product", "word"))
    bad = (np.nan, np.inf, -np.inf)
    for n, (v, s) in enumerate(rubbish):
        if n < 3:
            case["scores"][v, s] = bad[n]
        elif n < 13:
            case["boxes"][v, s, (n - 3) % 5] = bad[(n - 3) % 3] if n - 3 < 5 else bad[(n - 3 + 1) % 3]
        elif n == 13:
            case["boxes"][v, s, 2] = 0.0
        elif n == 14:
            case["boxes"][v, s, 3] = -4.0
        elif n == 15:
            case["boxes"][v, s, 2] = -0.0
        elif n < 19:          # a text maximum that is not a number, at the first step (always read): no key in modes 1 and 2
            case["text_max"][v, s, 0] = bad[n - 16]
        elif n == 19:         # ... and one BEHIND the stop symbol, which is never read
            case["text_arg"][v, s, 1] = case["stop_index"]
            case["text_max"][v, s, 3] = np.nan
    assert margin_violations(case, ranks=case["ranks"]) == []
    case["ref"] = ref_of(case)
    assert case["ref"]["count"] == 44 - 16
    assert ref_of(case, "word")["count"] == ref_of(case, "product")["count"] == 44 - 19
    return case


@functools.lru_cache(maxsize=None)
def bad_affine_row():
    """three views of 12 words each; view 1's row holds a NaN (in a matrix entry, in s or in dtheta): only its candidates go"""
    b = Builder(14, 3, 16)
    for c in grid_centres(12, 50.0, 6):
        base = word(b.g, *c)
        for v in range(3):
            b.put(v, jit(base))
    return b.case()


@functools.lru_cache(maxsize=None)
def on_the_bounds():
    """centres exactly on each side of the bounds (kept) and one float32 ulp outside (dropped); one view, identity frame"""
    x0, y0, x1, y1 = (np.float32(v) for v in (16.0, 8.0, 400.0, 300.0))
    up, down = (lambda t: np.nextafter(t, np.float32(INF))), (lambda t: np.nextafter(t, np.float32(-INF)))
    b = Builder(15, 1, 16, bounds=(x0, y0, x1, y1))
    rows = [(x0, 100.0, True), (down(x0), 150.0, False), (x1, 100.0, True), (up(x1), 150.0, False), (200.0, y0, True),
            (250.0, down(y0), False), (200.0, y1, True), (250.0, up(y1), False), (x0, y0, True), (x1, y1, True), (120.0, 200.0, True)]
    for cx, cy, _ in rows:
        b.put(0, lambda g, c=(cx, cy): np.array([c[0], c[1], 12.0, 6.0, 0.0], dtype=np.float32), raw=True)
    case = b.case(on_bound=True)
    case["inside"] = [r[2] for r in rows]
    assert case["ref"]["count"] == sum(case["inside"])
    return case


ALL_CASES = (one_view_identity, scene_four_rotations, same_view_pairs, late_supporters, view_63, counts_edges, nonfinite_rows,
             bad_affine_row)
