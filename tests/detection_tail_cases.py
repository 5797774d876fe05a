"""Float64 references and case builders for the detection tail: box_decode_kernel and nms_select_kernel
(csrc/proposals.hip) and detections_finalize_kernel (csrc/detections.hip).  Test helper, not product code.

References.  Each one starts from the float32 inputs the kernel receives, computes in float64 and is written from the
documented semantics (detectron2 Box2BoxTransformRotated.apply_deltas, RotatedBoxes.clip / scale / nonempty,
batched_nms_rotated, GlassRCNN._postprocess), not from the kernels.  The IoU is known_answers.iou_f64 (Sutherland-
Hodgman clipping); categories are handled by the property "boxes of different categories never suppress each other",
not by imitating the coordinate offset.

Case builders.  The kernels are discontinuous (thresholds, a clip switch at |angle| = 1 degree, argmax), so a case is
only usable when no decision sits closer to its boundary than float32 can resolve.  Every builder draws from a fixed
seed and redraws the offending rows until these margins hold, then returns the case; nothing is skipped or masked
when results are compared:

  IOU_MARGIN    |iou_f64 - nms_thresh| >= 1e-3 for every same-category pair of surviving rows (50x the 2e-5 the suite
                asserts for the kernel's own IoU).  Centres, sizes and angles are continuous random values, so distinct
                boxes never share an edge line; bit-equal duplicates (IoU 1) are allowed and wanted.
  CLIP_MARGIN   the normalised angle is >= 1e-3 degrees away from +-1, and every clipped extent is either exactly 0
                (the box lies outside by >= 1e-3 px) or >= 1e-3 px.
  ORIENT_MARGIN top-1 minus top-2 orientation logit >= 1e-3, except bit-equal ties (the first maximum wins).
  scores        all distinct unless the case is about ties; tie values are exact float32 numbers.
"""
import functools
import math

import numpy as np

from known_answers import iou_f64

SCALE_CLAMP = math.log(1000.0 / 16)
NMS_CLIP, NMS_DROP_EMPTY = 1, 2
IOU_MARGIN = 1e-3
CLIP_MARGIN = 1e-3
ORIENT_MARGIN = 1e-3
WEIGHT_SETS = ((1.0, 1.0, 1.0, 1.0, 2.0), (10.0, 10.0, 5.0, 5.0, 10.0))     # RPN, box head


def _f64(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def norm_angle(a):
    return (a + 180.0) % 360.0 - 180.0


def angle_diff(a, b):
    """circular difference in degrees, in [-180, 180)"""
    return (np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64) + 180.0) % 360.0 - 180.0


# ------------------------------------------------------------------------------------------------ box decode
def decode_ref(cls, deltas, orient, props, weights):
    """Box2BoxTransformRotated.apply_deltas + the two softmaxes of the box head.
    -> boxes [R,5], foreground probability [R] (column 0 of the 2-way softmax), (argmax, max probability) [R,2]."""
    cls, deltas, orient, props = _f64(cls), _f64(deltas), _f64(orient), _f64(props)
    wx, wy, ww, wh, wa = (float(v) for v in weights)
    with np.errstate(all="ignore"):
        dx, dy, dw, dh, da = deltas[:, 0] / wx, deltas[:, 1] / wy, deltas[:, 2] / ww, deltas[:, 3] / wh, deltas[:, 4] / wa
        dw = np.where(dw > SCALE_CLAMP, SCALE_CLAMP, dw)             # clamp(max=): NaN stays NaN
        dh = np.where(dh > SCALE_CLAMP, SCALE_CLAMP, dh)
        boxes = np.empty_like(props)
        boxes[:, 0] = dx * props[:, 2] + props[:, 0]
        boxes[:, 1] = dy * props[:, 3] + props[:, 1]
        boxes[:, 2] = np.exp(dw) * props[:, 2]
        boxes[:, 3] = np.exp(dh) * props[:, 3]
        boxes[:, 4] = norm_angle(da * 180.0 / math.pi + props[:, 4])
        e = np.exp(cls - cls.max(axis=1, keepdims=True))
        fg = e[:, 0] / e.sum(axis=1)
        eo = np.exp(orient - orient.max(axis=1, keepdims=True))
        po = eo / eo.sum(axis=1, keepdims=True)
    am = np.argmax(orient, axis=1)                                   # first maximum
    return boxes, fg, np.stack([am.astype(np.float64), po[np.arange(len(am)), am]], axis=1)


def _orient_logits(g, R):
    o = (g.standard_normal((R, 4)) * 2.0).astype(np.float32)
    for r in range(R):
        while True:
            s = np.sort(o[r].astype(np.float64))
            if s[3] - s[2] >= ORIENT_MARGIN:
                break
            o[r] = (g.standard_normal(4) * 2.0).astype(np.float32)
    return o


def orient_margin_ok(orient):
    """every row: top-1 minus top-2 >= ORIENT_MARGIN, or the top values are bit-equal"""
    s = np.sort(_f64(orient), axis=1)
    gap = s[:, 3] - s[:, 2]
    return bool(np.all((gap >= ORIENT_MARGIN) | (gap == 0.0)))


def _proposals(g, R, lo=10.0, hi=150.0):
    return np.stack([g.uniform(lo, hi, R), g.uniform(lo, hi, R), g.uniform(12, 80, R), g.uniform(8, 36, R),
                     g.uniform(-180, 180, R)], axis=1).astype(np.float32)


@functools.lru_cache(maxsize=None)
def decode_case(R, wset):
    """R rows for weight set `wset`; the special rows (clamp edge, angle wraps, saturated logits, orientation ties,
    non-finite deltas) sit at fixed slots spread over [0, R), the last row included.
    -> dict(cls, deltas, orient, props, weights, nonfinite_rows, clamp_rows)."""
    weights = WEIGHT_SETS[wset]
    g = np.random.default_rng(1000 + 10 * R + wset)
    cls = (g.standard_normal((R, 2)) * 2.0).astype(np.float32)
    deltas = (g.standard_normal((R, 5)) * np.array(weights) * [0.1, 0.1, 0.2, 0.2, 0.3]).astype(np.float32)
    orient = _orient_logits(g, R)
    props = _proposals(g, R)
    ww, wh, wa = weights[2], weights[3], weights[4]
    clamp32 = float(np.float32(SCALE_CLAMP))
    specials = []
    for v in (np.nextafter(np.float32(clamp32 * ww), np.float32(0)), np.float32(clamp32 * ww), np.float32(40.0 * ww), np.float32(1e30)):
        specials.append(("dw", 2, v))
    for v in (np.nextafter(np.float32(clamp32 * wh), np.float32(0)), np.float32(clamp32 * wh), np.float32(40.0 * wh)):
        specials.append(("dh", 3, v))
    for wraps in (0, 1, 3):
        for sign in (1.0, -1.0):
            specials.append(("da", 4, np.float32(sign * (wraps * 2.0 * math.pi + 0.4) * wa)))
    for c in ((50.0, -50.0), (-50.0, 50.0), (100.0, 0.0), (0.0, 100.0)):
        specials.append(("cls", None, c))
    for tie in ((0, 1), (1, 3), (2, 3), (0, 1, 2, 3)):
        specials.append(("tie", None, tie))
    bad = [(k, np.float32(np.nan)) for k in range(5)] + [(0, np.float32(np.inf)), (1, np.float32(-np.inf)), (4, np.float32(np.inf))]
    for k, v in bad:
        specials.append(("bad", k, v))
    slots = sorted(set(int(round(i * (R - 1) / max(1, len(specials) - 1))) for i in range(len(specials)))) if R >= 2 * len(specials) else []
    nonfinite, clamped = [], []
    for slot, (kind, k, v) in zip(slots, specials):
        if kind in ("dw", "dh", "da"):
            deltas[slot, k] = v
            if kind != "da":
                clamped.append(slot)
        elif kind == "cls":
            cls[slot] = v
        elif kind == "tie":
            orient[slot] = np.float32(-1.0) + np.arange(4, dtype=np.float32) * np.float32(-0.25)
            orient[slot, list(v)] = np.float32(1.75)
        else:
            deltas[slot, k] = v
            nonfinite.append(slot)
    return dict(cls=cls, deltas=deltas, orient=orient, props=props, weights=weights, nonfinite_rows=nonfinite,
                clamp_rows=clamped, special_slots=slots)


# ------------------------------------------------------------------------------------------------ clip
def clip_ref(b, h, w):
    """RotatedBoxes.clip of one float64 box: normalise the angle; clip only when |angle| <= 1 degree"""
    b = np.array(b, dtype=np.float64)
    b[4] = norm_angle(b[4])
    if abs(b[4]) <= 1.0:
        x1, y1, x2, y2 = b[0] - b[2] / 2, b[1] - b[3] / 2, b[0] + b[2] / 2, b[1] + b[3] / 2
        x1, x2 = min(max(x1, 0.0), float(w)), min(max(x2, 0.0), float(w))
        y1, y2 = min(max(y1, 0.0), float(h)), min(max(y2, 0.0), float(h))
        b[0], b[1] = (x1 + x2) / 2, (y1 + y2) / 2
        b[2], b[3] = min(b[2], x2 - x1), min(b[3], y2 - y1)
    return b


def clip_margin_ok(b, h, w):
    """CLIP_MARGIN for one float64 box against an h x w image"""
    a = float(norm_angle(b[4]))
    if abs(abs(a) - 1.0) < CLIP_MARGIN:
        return False
    if abs(a) > 1.0:
        return True
    for c, e, lim in ((b[0], b[2], float(w)), (b[1], b[3], float(h))):
        lo, hi = c - e / 2, c + e / 2
        ext = min(max(hi, 0.0), lim) - min(max(lo, 0.0), lim)
        outside = hi <= -CLIP_MARGIN or lo >= lim + CLIP_MARGIN
        if not (outside or ext >= CLIP_MARGIN):
            return False
    return True


# ------------------------------------------------------------------------------------------------ IoU, pairs, margins
_IOU = {}


COARSE_S = 8192          # from this many rows on, a pair whose float32 oracle IoU is exactly 0 is not evaluated in float64


def _oracle_iou_is_zero(a, b):
    import ctypes
    from oracle import d2ops
    fp = ctypes.POINTER(ctypes.c_float)
    a32, b32 = a.astype(np.float32), b.astype(np.float32)
    return d2ops.lib().d2o_single_box_iou_rotated(a32.ctypes.data_as(fp), b32.ctypes.data_as(fp)) == 0.0


def iou_cached(a, b, coarse=False):
    ka, kb = a.tobytes(), b.tobytes()
    key = (ka, kb) if ka <= kb else (kb, ka)
    v = _IOU.get(key)
    if v is None:
        v = _IOU[key] = 0.0 if coarse and _oracle_iou_is_zero(a, b) else iou_f64(a, b)
    return v


def _radius(B):
    return 0.5 * np.hypot(B[:, 2], B[:, 3])


def _not_disjoint(d2, rsum):
    """the circumscribed circles of two boxes are not disjoint (when they are, the IoU is exactly 0)"""
    return d2 <= rsum * rsum * (1.0 + 1e-9) + 1e-9


def near_pairs(B, cat=None, alive=None):
    """pairs (i, j), i < j, of alive rows of the same category whose circumscribed circles are not disjoint"""
    n = len(B)
    if n == 0:
        return np.zeros((0, 2), dtype=np.int64)
    r = _radius(B)
    o = np.argsort(B[:, 0], kind="stable")                           # sweep along x: only a window of columns per block of rows
    x, reach = B[o, 0], 2.0 * float(r.max()) + 1.0
    out = [np.zeros((0, 2), dtype=np.int64)]
    for s in range(0, n, 256):
        e = min(n, s + 256)
        c0, c1 = np.searchsorted(x, x[s] - reach), np.searchsorted(x, x[e - 1] + reach)
        rows, cols = o[s:e], o[c0:c1]
        dx, dy = B[rows, None, 0] - B[None, cols, 0], B[rows, None, 1] - B[None, cols, 1]
        m = _not_disjoint(dx * dx + dy * dy, r[rows, None] + r[None, cols]) & (rows[:, None] < cols[None, :])
        if cat is not None:
            m &= cat[rows, None] == cat[None, cols]
        if alive is not None:
            m &= alive[rows, None] & alive[None, cols]
        ii, jj = np.nonzero(m)
        out.append(np.stack([rows[ii], cols[jj]], axis=1))
    out = np.concatenate(out)
    return out[np.lexsort((out[:, 1], out[:, 0]))]


def iou_margin_violations(B, threshs, cat=None, alive=None):
    """the near pairs whose float64 IoU is closer than IOU_MARGIN to one of `threshs`"""
    bad = []
    coarse = len(B) >= COARSE_S // 2
    for i, j in near_pairs(B, cat, alive):
        v = iou_cached(B[i], B[j], coarse)
        if any(abs(v - t) < IOU_MARGIN for t in threshs):
            bad.append((int(i), int(j)))
    return bad


def _settle(B, regen, threshs, deps=None, cat=None, alive=None, rounds=60):
    """redraw (regen(i) -> new effective float64 box of row i; rows in deps[i] are re-derived after it) the
    higher-indexed row of every pair that violates IOU_MARGIN until none does.  B is modified in place."""
    deps = deps or {}
    for _ in range(rounds):
        bad = iou_margin_violations(B, threshs, cat, alive() if callable(alive) else alive)
        if not bad:
            return B
        for i in sorted(set(max(p) for p in bad)):
            B[i] = regen(i)
            for d in deps.get(i, ()):
                B[d] = regen(d)
    raise AssertionError("IoU margin not reached")


# ------------------------------------------------------------------------------------------------ NMS select
def nms_image_detail(boxes, scores, cat, cnt, hw, score_thresh, nms_thresh, post_topk, flags):
    """one image.  -> dict: order (surviving source slots, sorted), eff (their clipped float64 boxes), kept_pos
    (positions in `order` that are kept), sup_by (position -> kept positions that suppress it), keep (source slots)."""
    boxes, s32 = _f64(boxes), np.asarray(scores, dtype=np.float32)
    thr = float(np.float32(score_thresh))
    nthr = float(np.float32(nms_thresh))
    h, w = int(hw[0]), int(hw[1])
    cand, eff = [], {}
    for s in range(min(int(cnt), len(s32))):
        if not (np.isfinite(s32[s]) and np.isfinite(boxes[s]).all()):
            continue
        b = clip_ref(boxes[s], h, w) if flags & NMS_CLIP else boxes[s].copy()
        if (flags & NMS_DROP_EMPTY) and (b[2] <= 0 or b[3] <= 0):
            continue
        if not float(s32[s]) > thr:
            continue
        cand.append(s)
        eff[s] = b
    order = sorted(cand, key=lambda s: (-float(s32[s]), s))          # -0.0 == +0.0; stable: lower slot first
    E = np.array([eff[s] for s in order], dtype=np.float64).reshape(-1, 5)
    C = np.asarray(cat)[order] if cat is not None else None
    r = _radius(E)
    kept_pos, sup_by = [], {}
    kept_arr = np.zeros((len(order),), dtype=np.int64)
    coarse = len(s32) >= COARSE_S
    for p in range(len(order)):
        if len(kept_pos) >= post_topk:
            break
        hits = []
        if kept_pos:
            kp = kept_arr[: len(kept_pos)]
            dx, dy = E[kp, 0] - E[p, 0], E[kp, 1] - E[p, 1]
            m = _not_disjoint(dx * dx + dy * dy, r[kp] + r[p])
            if C is not None:
                m &= C[kp] == C[p]
            hits = [int(q) for q in kp[m] if iou_cached(E[q], E[p], coarse) >= nthr]
        if hits:
            sup_by[p] = hits
        else:
            kept_arr[len(kept_pos)] = p
            kept_pos.append(p)
    return dict(order=order, eff=E, kept_pos=kept_pos, sup_by=sup_by, keep=[order[p] for p in kept_pos])


def nms_select_ref(boxes, scores, cat, valid_count, image_hw, score_thresh, nms_thresh, post_topk, flags):
    """boxes [N,S,5], scores [N,S], cat [N,S] or None, valid_count [N] or None -> kept source slots per image"""
    N, S = np.asarray(scores).shape
    return [nms_image_detail(boxes[n], scores[n], None if cat is None else cat[n], S if valid_count is None else valid_count[n],
                             image_hw[n], score_thresh, nms_thresh, post_topk, flags)["keep"] for n in range(N)]


def nms_clipped_boxes(case, n, slots):
    """the (clipped) float64 source boxes of `slots` of image n, as out_boxes must hold them"""
    b = _f64(case["boxes"][n])
    h, w = case["image_hw"][n]
    return np.array([clip_ref(b[s], h, w) if case["flags"] & NMS_CLIP else b[s] for s in slots], dtype=np.float64).reshape(-1, 5)


def _draw_box(g, lo, hi, wr=(12.0, 90.0), hr=(8.0, 40.0)):
    return np.array([g.uniform(lo, hi), g.uniform(lo, hi), g.uniform(*wr), g.uniform(*hr), g.uniform(-180, 180)], dtype=np.float32)


def _jitter(g, b):
    """a copy offset by a few percent of the size: IoU with the original roughly 0.8 .. 0.95"""
    return np.array([b[0] + g.uniform(-0.04, 0.04) * b[2], b[1] + g.uniform(-0.04, 0.04) * b[3], b[2] * (1 + g.uniform(-0.03, 0.03)),
                     b[3] * (1 + g.uniform(-0.03, 0.03)), b[4] + g.uniform(-1.5, 1.5)], dtype=np.float32)


def _box_set(g, S, nfree, njit, lo, hi, threshs, wr=(12.0, 90.0), hr=(8.0, 40.0)):
    """S float32 boxes: nfree drawn freely, njit jittered copies of free ones, the rest bit-equal duplicates of free
    ones, settled to IOU_MARGIN for `threshs`.  -> raw [S,5] float32, kind [S] (0 free, 1 jitter, 2 duplicate), base [S]"""
    nfree, njit = min(nfree, S), min(njit, S - min(nfree, S))
    raw = np.zeros((S, 5), dtype=np.float32)
    kind = np.zeros((S,), dtype=np.int32)
    base = np.full((S,), -1, dtype=np.int64)
    for i in range(S):
        if i < nfree:
            raw[i] = _draw_box(g, lo, hi, wr, hr)
        else:
            base[i] = int(g.integers(0, nfree))
            kind[i] = 1 if i < nfree + njit else 2
            raw[i] = _jitter(g, raw[base[i]]) if kind[i] == 1 else raw[base[i]]
    deps = {}
    for i in range(S):
        if kind[i] == 1:
            deps.setdefault(int(base[i]), []).append(i)

    def regen(i):
        raw[i] = _draw_box(g, lo, hi, wr, hr) if kind[i] == 0 else _jitter(g, raw[base[i]])
        return raw[i].astype(np.float64)

    _settle(raw.astype(np.float64), regen, threshs, deps=deps, alive=kind != 2)
    dup = kind == 2
    raw[dup] = raw[base[dup]]
    return raw, kind, base


def _distinct_scores(g, S, lo, hi):
    return g.permutation(np.linspace(lo, hi, S)).astype(np.float32)


RUBBISH_SCORES = (np.nan, np.inf, 5.0, 7.0)


def _two_images(g, raw, scores, cat, valid1):
    """image 0: the rows as given, all valid.  image 1: a permutation of them with valid_count = valid1 and rubbish
    behind it: NaN and +inf scores, and finite top scores on huge or NaN boxes."""
    S = len(raw)
    perm = g.permutation(S)
    boxes = np.stack([raw, raw[perm]]).astype(np.float32)
    sc = np.stack([scores, scores[perm]]).astype(np.float32)
    ct = None if cat is None else np.stack([cat, cat[perm]]).astype(np.int32)
    for k, s in enumerate(range(valid1, S)):
        sc[1, s] = RUBBISH_SCORES[k % 4]
        if k % 4 == 2:
            boxes[1, s, 2:4] = 1e18
        if k % 4 == 3:
            boxes[1, s, k % 5] = np.nan
    return boxes, sc, ct, np.array([S, valid1], dtype=np.int32)


def _case(boxes, scores, cat, valid_count, hw, score_thresh, nms_thresh, flags, **extra):
    d = dict(boxes=boxes, scores=scores, cat=cat, valid_count=valid_count, image_hw=np.array([hw, hw], dtype=np.int32),
             score_thresh=score_thresh, nms_thresh=nms_thresh, flags=flags)
    d.update(extra)
    return d


DENSE_THRESHS = (0.35, 0.7)
DENSE_TOPKS = (1024, 100, 64, 1)


@functools.lru_cache(maxsize=None)
def dense_case():
    """S = 320 (250 free + 50 jittered + 20 duplicate boxes in [20,140]^2), settled for both thresholds.  The 64 best
    scores go to a set of mutually non-overlapping boxes, so post_topk = 64 is reached by the last candidate of chunk 0."""
    g = np.random.default_rng(320)
    S = 320
    raw, kind, _ = _box_set(g, S, 250, 50, 20.0, 140.0, DENSE_THRESHS)
    B = raw.astype(np.float64)
    indep = []
    for i in g.permutation(S):
        if len(indep) < 64 and all(iou_cached(B[i], B[j]) < min(DENSE_THRESHS) for j in indep):
            indep.append(int(i))
    assert len(indep) == 64
    vals = np.sort(np.linspace(0.02, 0.98, S).astype(np.float32))[::-1]
    scores = np.zeros((S,), dtype=np.float32)
    scores[g.permutation(indep)] = vals[:64]
    rest = np.setdiff1d(np.arange(S), indep)
    scores[g.permutation(rest)] = vals[64:]
    boxes, sc, _, vc = _two_images(g, raw, scores, None, 200)
    return _case(boxes, sc, None, vc, (4096, 4096), 0.05, None, 0, kind=kind)


@functools.lru_cache(maxsize=None)
def category_case():
    """S = 300: 100 boxes, each once per category 0..2, on a 120 x 160 image with CLIP | DROP_EMPTY and negative scores.
    40 of the 100 are near-horizontal, so they are clipped; some of those lie outside and become empty."""
    g = np.random.default_rng(300)
    H, W, nb, thr = 120, 160, 100, 0.5
    raw = np.zeros((nb, 5), dtype=np.float32)

    def draw(i):
        while True:
            if i < 60:
                b = np.array([g.uniform(0, W), g.uniform(0, H), g.uniform(12, 90), g.uniform(8, 40), g.uniform(-180, 180)], dtype=np.float32)
            elif i < 70:                                              # near-horizontal and outside the image
                side = g.integers(0, 4)
                cx = (-70.0, W + 70.0, g.uniform(0, W), g.uniform(0, W))[side]
                cy = (g.uniform(0, H), g.uniform(0, H), -40.0, H + 40.0)[side]
                b = np.array([cx, cy, g.uniform(12, 90), g.uniform(8, 40), g.uniform(-0.9, 0.9)], dtype=np.float32)
            else:                                                     # near-horizontal, mostly straddling an edge
                b = np.array([g.uniform(-30, W + 30), g.uniform(-15, H + 15), g.uniform(12, 90), g.uniform(8, 40), g.uniform(-0.9, 0.9)],
                             dtype=np.float32)
            if clip_margin_ok(b.astype(np.float64), H, W):
                raw[i] = b
                return clip_ref(b.astype(np.float64), H, W)

    E = np.array([draw(i) for i in range(nb)])
    _settle(E, draw, (thr,), alive=lambda: (E[:, 2] > 0) & (E[:, 3] > 0))
    rows = g.permutation(3 * nb)
    base, cat = rows % nb, (rows // nb).astype(np.int32)
    scores = _distinct_scores(g, 3 * nb, -8.0, 3.0)
    boxes, sc, ct, vc = _two_images(g, raw[base], scores, cat, 240)
    return _case(boxes, sc, ct, vc, (H, W), float("-inf"), thr, NMS_CLIP | NMS_DROP_EMPTY, base=base, post_topk=1024)


TIE_VALUES = (-1.5, -0.25, -0.0, 0.0, 0.125, 0.5, 0.75, 2.0)


@functools.lru_cache(maxsize=None)
def tie_case():
    """S = 150: 60 free boxes, 30 jittered and 60 bit-equal duplicates; scores drawn from 8 exact values, -0.0 and +0.0
    among them, so most decisions are made by the slot index alone"""
    g = np.random.default_rng(150)
    S = 150
    raw, kind, _ = _box_set(g, S, 60, 30, 20.0, 140.0, (0.5,))
    order = g.permutation(S)
    raw, kind = raw[order], kind[order]
    scores = np.array(TIE_VALUES, dtype=np.float32)[g.integers(0, 8, S)]
    boxes, sc, _, vc = _two_images(g, raw, scores, None, 110)
    return _case(boxes, sc, None, vc, (4096, 4096), float("-inf"), 0.5, 0, kind=kind, post_topk=1024)


FILTER_THRESH = 0.3


@functools.lru_cache(maxsize=None)
def filter_case():
    """S = 24.  Slots 0..11: healthy boxes on a grid, far apart.  Slot 12 + k: a bit-equal copy of box k with the best
    score and a non-finite value in field k of (score, cx, cy, w, h, angle): were it not dropped it would suppress
    box k.  Slot 18: score == score_thresh; 19: the next float32 above it; 20..23: negative and zero scores."""
    g = np.random.default_rng(24)
    S = 24
    raw = np.zeros((S, 5), dtype=np.float32)
    for k in range(S):
        raw[k] = [60.0 + 120.0 * (k % 6), 60.0 + 120.0 * (k // 6), g.uniform(30, 80), g.uniform(20, 40), g.uniform(-180, 180)]
    scores = _distinct_scores(g, S, 0.4, 0.9)
    bad = (np.nan, np.inf, -np.inf, np.nan, np.inf, -np.inf)
    for k in range(6):
        raw[12 + k] = raw[k]
        scores[12 + k] = 0.95 + 0.001 * k
        if k == 0:
            scores[12] = bad[0]
        else:
            raw[12 + k, k - 1] = bad[k]
    t = np.float32(FILTER_THRESH)
    scores[18], scores[19] = t, np.nextafter(t, np.float32(1))
    scores[20:24] = [-0.5, -3.0, 0.0, -0.0]
    boxes, sc, _, vc = _two_images(g, raw, scores, None, 22)
    return _case(boxes, sc, None, vc, (4096, 4096), FILTER_THRESH, 0.5, NMS_CLIP, post_topk=1024)


SIZE_EDGES = (1, 64, 65, 1000)


@functools.lru_cache(maxsize=None)
def size_case(S):
    """S boxes (60 % free, 25 % jittered, 15 % duplicates) on a square whose side grows with sqrt(S)"""
    g = np.random.default_rng(5000 + S)
    side = 30.0 * math.sqrt(S) + 40.0
    nfree = max(1, (S * 6 + 9) // 10)
    raw, kind, _ = _box_set(g, S, nfree, S // 4, 20.0, 20.0 + side, (0.5,), wr=(12.0, 60.0), hr=(8.0, 30.0))
    order = g.permutation(S)
    raw, kind = raw[order], kind[order]
    scores = _distinct_scores(g, S, 0.02, 0.98) if S > 1 else np.array([0.5], dtype=np.float32)
    boxes, sc, _, vc = _two_images(g, raw, scores, None, (S * 5) // 8)
    return _case(boxes, sc, None, vc, (4096, 4096), 0.05, 0.5, 0, kind=kind, post_topk=1024)


@functools.lru_cache(maxsize=None)
def identical_case():
    """S = 65 copies of one box with distinct scores: exactly the best-scored one survives"""
    g = np.random.default_rng(65)
    raw = np.tile(np.array([[70.0, 50.0, 40.0, 20.0, 33.0]], dtype=np.float32), (65, 1))
    boxes, sc, _, vc = _two_images(g, raw, _distinct_scores(g, 65, 0.1, 0.9), None, 40)
    return _case(boxes, sc, None, vc, (4096, 4096), 0.05, 0.5, 0, post_topk=1024)


@functools.lru_cache(maxsize=None)
def nothing_valid_case():
    """S = 65.  image 0: every score at or below the threshold; image 1: healthy rows, valid_count = 0"""
    g = np.random.default_rng(66)
    raw = np.stack([_draw_box(g, 20.0, 400.0) for _ in range(65)])
    sc0 = _distinct_scores(g, 65, -0.5, 0.05)
    sc0[3] = np.float32(0.05)
    boxes = np.stack([raw, raw]).astype(np.float32)
    sc = np.stack([sc0, _distinct_scores(g, 65, 0.5, 0.9)]).astype(np.float32)
    return _case(boxes, sc, None, np.array([65, 0], dtype=np.int32), (4096, 4096), 0.05, 0.5, 0, post_topk=1024)


@functools.lru_cache(maxsize=None)
def big_case():
    """S = 8192 boxes spread over [0,3000]^2: the greedy result reaches post_topk = 1024 (a full kept list, the longest
    candidates-vs-kept pair loop).  A copy scores a little below its original, so the best rows hold many suppressions.
    Pairs are pre-filtered by centre distance and by the oracle's float32 IoU being exactly 0 (COARSE_S); all others,
    so every pair that decides anything, are evaluated in float64."""
    g = np.random.default_rng(8192)
    S = 8192
    raw, kind, base = _box_set(g, S, 7000, 1000, 0.0, 3000.0, (0.5,), wr=(10.0, 40.0), hr=(6.0, 20.0))
    key = g.random(S)
    key[kind != 0] = key[base[kind != 0]] + g.uniform(0.002, 0.03, int((kind != 0).sum()))
    scores = np.zeros((S,), dtype=np.float32)
    scores[np.argsort(key)] = np.linspace(0.99, 0.01, S).astype(np.float32)
    order = g.permutation(S)
    raw, kind, scores = raw[order], kind[order], scores[order]
    boxes, sc, _, vc = _two_images(g, raw, scores, None, 5120)
    return _case(boxes, sc, None, vc, (4096, 4096), 0.05, 0.5, 0, kind=kind, post_topk=1024)


def nms_margin_violations(case, threshs=None):
    """IOU_MARGIN (and CLIP_MARGIN with CLIP) violations over the surviving rows of both images of a case"""
    threshs = threshs or (case["nms_thresh"],)
    bad = []
    for n in range(2):
        d = nms_image_detail(case["boxes"][n], case["scores"][n], None if case["cat"] is None else case["cat"][n],
                             case["valid_count"][n], case["image_hw"][n], case["score_thresh"], 2.0, 1 << 30, case["flags"])
        cat = None if case["cat"] is None else np.asarray(case["cat"][n])[d["order"]]
        bad += [(n,) + p for p in iou_margin_violations(d["eff"], threshs, cat)]
        if case["flags"] & NMS_CLIP:
            h, w = case["image_hw"][n]
            raw = _f64(case["boxes"][n])
            bad += [(n, s, "clip") for s in d["order"] if not clip_margin_ok(raw[s], h, w)]
    return bad


# ------------------------------------------------------------------------------------------------ detections finalize
def _finalize_box(b, sx, sy, out_h, out_w, min_box_dim, do_filter_small):
    """one float64 box -> (keep, new box): filter_small_boxes, RotatedBoxes.scale, clip, nonempty"""
    keep = (not do_filter_small) or min(b[2], b[3]) >= min_box_dim
    t = b[4] * math.pi / 180.0
    c, s = math.cos(t), math.sin(t)
    nb = np.array([b[0] * sx, b[1] * sy, b[2] * math.sqrt((sx * c) ** 2 + (sy * s) ** 2), b[3] * math.sqrt((sx * s) ** 2 + (sy * c) ** 2),
                   math.atan2(sx * s, sy * c) * 180.0 / math.pi])
    nb = clip_ref(nb, out_h, out_w)
    return bool(keep and nb[2] > 0 and nb[3] > 0), nb


def finalize_ref(boxes, scores, orient, text, counts, roi_start, scale_xy, out_hw, min_box_dim, do_filter_small):
    """GlassRCNN._postprocess over padded [N,K,...] inputs -> per image (kept slots, their new float64 boxes).
    The kept scores / orientations / text rows are plain gathers of the inputs by the kept slots (text row of slot j of
    image n: roi_start[n] + j), so the reference returns the slots and the boxes only.  counts[n] > K means K."""
    boxes, scale_xy = _f64(boxes), _f64(scale_xy)
    N, K = boxes.shape[:2]
    out = []
    for n in range(N):
        kept, nbs = [], []
        for j in range(min(int(counts[n]), K)):
            k, nb = _finalize_box(boxes[n, j], scale_xy[n, 0], scale_xy[n, 1], int(out_hw[n][0]), int(out_hw[n][1]), float(min_box_dim),
                                  do_filter_small)
            if k:
                kept.append(j)
                nbs.append(nb)
        out.append((np.array(kept, dtype=np.int64), np.array(nbs, dtype=np.float64).reshape(-1, 5)))
    return out


def finalize_margin_ok(b, sx, sy, out_h, out_w):
    """CLIP_MARGIN on the scaled box (angle after scale away from +-1 degree, clipped extents 0 or >= 1e-3 px)"""
    t = b[4] * math.pi / 180.0
    c, s = math.cos(t), math.sin(t)
    nb = np.array([b[0] * sx, b[1] * sy, b[2] * math.sqrt((sx * c) ** 2 + (sy * s) ** 2), b[3] * math.sqrt((sx * s) ** 2 + (sy * c) ** 2),
                   math.atan2(sx * s, sy * c) * 180.0 / math.pi])
    return clip_margin_ok(nb, out_h, out_w)


FINALIZE_ANGLES = (0.0, 0.5, -0.5, 45.0, -45.0, 90.0, -90.0, 179.9, -179.9)
MIN_BOX_DIM = 2.0


def _finalize_slot(g, want, in_hw, sxy, out_hw, special_angle):
    """a float32 box whose reference decision is `want`.  Kept: plain, min(w, h) == MIN_BOX_DIM exactly, or clipped
    but not empty.  Dropped: too small, or near-horizontal and outside the output image."""
    H, W = in_hw
    while True:
        mode = int(g.integers(0, 4))
        a = special_angle if special_angle is not None else g.uniform(-180, 180)
        b = [g.uniform(0.1 * W, 0.9 * W), g.uniform(0.1 * H, 0.9 * H), g.uniform(3, 60), g.uniform(3, 40), a]
        if want:
            if mode == 1:
                b[2 + int(g.integers(0, 2))] = MIN_BOX_DIM
            elif mode == 2 and special_angle is None:
                b[0], b[4] = g.uniform(-5, 10), g.uniform(-0.6, 0.6)                 # straddles the left edge
            elif mode == 3 and special_angle is None:
                b[1], b[4] = H + g.uniform(-8, 4), g.uniform(-0.6, 0.6)              # straddles the bottom edge
        else:
            if mode < 2 or special_angle not in (None, 0.0, 0.5, -0.5):
                b[2 + int(g.integers(0, 2))] = g.uniform(0.5, 1.99)
            else:
                b[0] = -g.uniform(40, 80) if mode == 2 else W + g.uniform(40, 80)
                b[2] = g.uniform(3, 40)
                if special_angle is None:
                    b[4] = g.uniform(-0.6, 0.6)
        b = np.array(b, dtype=np.float32)
        b64 = b.astype(np.float64)
        sx, sy = float(np.float32(sxy[0])), float(np.float32(sxy[1]))
        if finalize_margin_ok(b64, sx, sy, out_hw[0], out_hw[1]) and _finalize_box(b64, sx, sy, out_hw[0], out_hw[1], MIN_BOX_DIM, True)[0] == want:
            return b


def _finalize_build(seed, K, counts, in_hws, out_hws, patterns):
    g = np.random.default_rng(seed)
    N = len(counts)
    scale = np.array([[o[1] / i[1], o[0] / i[0]] for i, o in zip(in_hws, out_hws)], dtype=np.float32)
    boxes = np.zeros((N, K, 5), dtype=np.float32)
    for n in range(N):
        for j in range(K):
            want = bool(patterns[n][j]) if j < min(counts[n], K) else True       # rows behind the count: healthy boxes
            special = FINALIZE_ANGLES[(j // 3) % len(FINALIZE_ANGLES)] if j % 3 == 0 else None
            boxes[n, j] = _finalize_slot(g, want, in_hws[n], scale[n], out_hws[n], special)
    scores = g.permutation(np.linspace(0.05, 0.99, N * K)).astype(np.float32).reshape(N, K)
    orient = np.stack([g.integers(0, 4, (N, K)).astype(np.float32), g.uniform(0.25, 1.0, (N, K)).astype(np.float32)], axis=2)
    clamped = [min(c, K) for c in counts]
    return dict(boxes=boxes, scores=scores, orient=orient, counts=np.array(counts, dtype=np.int32), clamped=clamped,
                roi_start=np.concatenate([[0], np.cumsum(clamped)[:-1]]).astype(np.int32), scale_xy=scale,
                out_hw=np.array(out_hws, dtype=np.int32), in_hw=list(in_hws), min_box_dim=MIN_BOX_DIM, K=K, N=N)


@functools.lru_cache(maxsize=None)
def finalize_case():
    """N = 4, K = 600, counts [600, 0, 257, 1000 (clamped to K)], scales 450/300 x 400/200 and 1/1.6.  Keep pattern:
    random in most wavefronts, slots 512..575 of image 0 all kept, slots 64..127 of image 3 all dropped."""
    g = np.random.default_rng(600)
    K = 600
    pat = [g.random(K) < p for p in (0.7, 0.5, 0.5, 0.6)]
    pat[0][512:576] = True
    pat[3][64:128] = False
    pat[2][256] = True
    return _finalize_build(601, K, (600, 0, 257, 1000), ((200, 300), (160, 160), (160, 200), (200, 300)),
                           ((400, 450), (160, 160), (100, 125), (400, 450)), pat)


@functools.lru_cache(maxsize=None)
def finalize_full_case():
    """N = 2, K = 1024, counts [1024, 1000]: every slot is kept (keep_src filled to its last entry)"""
    K = 1024
    return _finalize_build(1024, K, (1024, 1000), ((200, 300), (160, 200)), ((400, 450), (100, 125)), [np.ones(K, dtype=bool)] * 2)


def wave_keep_table(kept, count):
    """kept/dropped slot counts of every (256-slot chunk, wavefront) of one image: {(chunk, wave): (kept, dropped)}"""
    mask = np.zeros((count,), dtype=bool)
    mask[np.asarray(kept, dtype=np.int64)] = True
    out = {}
    for s in range(0, count, 64):
        m = mask[s:s + 64]
        out[(s // 256, (s // 64) % 4)] = (int(m.sum()), int(len(m) - m.sum()))
    return out


# ------------------------------------------------------------------------------------------------ decode -> NMS chain
CHAIN = dict(N=2, P=300, counts=(300, 180), score_thresh=0.05, nms_thresh=0.35, topk=100, hw=(160, 160), weights=WEIGHT_SETS[1])


@functools.lru_cache(maxsize=None)
def chain_case():
    """random box-head outputs for 2 x 300 proposal slots, redrawn row by row until the decoded boxes have the IoU and
    clip margins, the foreground probabilities are >= 1e-5 apart from each other and >= 1e-4 from the threshold, and the
    orientation logits have theirs.  Slots behind the proposal count hold rubbish."""
    g = np.random.default_rng(77)
    N, P, wts, (H, W) = CHAIN["N"], CHAIN["P"], CHAIN["weights"], CHAIN["hw"]
    cls = np.zeros((N, P, 2), dtype=np.float32)
    deltas = np.zeros((N, P, 5), dtype=np.float32)
    props = np.zeros((N, P, 5), dtype=np.float32)
    orient = np.stack([_orient_logits(g, P) for _ in range(N)])
    for n in range(N):
        cnt = CHAIN["counts"][n]

        def one(i):
            dl, pr, lg = deltas[n, i:i + 1], props[n, i:i + 1], cls[n, i:i + 1]
            return decode_ref(lg, dl, orient[n, i:i + 1], pr, wts)

        def draw(i):
            while True:
                props[n, i] = _proposals(g, 1)[0]
                if i % 6 == 0:
                    props[n, i, 4] = g.uniform(-0.5, 0.5)
                    props[n, i, 0] = g.choice([g.uniform(0, 15), g.uniform(W - 15, W)])
                deltas[n, i] = (g.standard_normal(5) * np.array(wts) * [0.1, 0.1, 0.15, 0.15, 0.005 if i % 6 == 0 else 0.2]).astype(np.float32)
                b = one(i)[0][0]
                if clip_margin_ok(b, H, W):
                    return clip_ref(b, H, W)

        def draw_cls(i):
            cls[n, i] = (g.standard_normal(2) * 2.0).astype(np.float32)
            return one(i)[1][0]

        E = np.array([draw(i) for i in range(cnt)])
        fg = np.array([draw_cls(i) for i in range(cnt)])
        for _ in range(100):
            o = np.argsort(fg)
            close = set(int(o[k + 1]) for k in np.nonzero(np.diff(fg[o]) < 1e-5)[0])
            close |= set(int(i) for i in np.nonzero(np.abs(fg - float(np.float32(CHAIN["score_thresh"]))) < 1e-4)[0])
            if not close:
                break
            for i in close:
                fg[i] = draw_cls(i)
        else:
            raise AssertionError("score margin not reached")
        _settle(E, draw, (CHAIN["nms_thresh"],), alive=fg > CHAIN["score_thresh"])
        for k, i in enumerate(range(cnt, P)):                        # padding slots
            if k % 3 == 0:
                cls[n, i], deltas[n, i, k % 5], props[n, i] = (9.0, -9.0), np.nan, _proposals(g, 1)[0]
            elif k % 3 == 1:
                cls[n, i], props[n, i] = (9.0, -9.0), _proposals(g, 1)[0]
    return dict(cls=cls, deltas=deltas, orient=orient, props=props, counts=np.array(CHAIN["counts"], dtype=np.int32),
                image_hw=np.array([CHAIN["hw"]] * N, dtype=np.int32))


def chain_ref(case):
    """decode_ref then nms_select_ref, as RotatedFastRCNNOutputLayers.inference_batched chains the two kernels"""
    N, P = CHAIN["N"], CHAIN["P"]
    b, fg, o2 = decode_ref(case["cls"].reshape(-1, 2), case["deltas"].reshape(-1, 5), case["orient"].reshape(-1, 4),
                           case["props"].reshape(-1, 5), CHAIN["weights"])
    b32, fg32 = b.astype(np.float32).reshape(N, P, 5), fg.astype(np.float32).reshape(N, P)
    keep = nms_select_ref(b32, fg32, None, case["counts"], case["image_hw"], CHAIN["score_thresh"], CHAIN["nms_thresh"], CHAIN["topk"], NMS_CLIP)
    return keep, b.reshape(N, P, 5), fg.reshape(N, P), o2.reshape(N, P, 2)
