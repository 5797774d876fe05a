"""Float64 reference and case builders for the word post-processor (csrc/postprocess.hip for K <= 128 padded detections
per image, csrc/postprocess_dense.hip up to 1024).  Test helper, not product code.

Reference.  `reference_image` is the whole post-processor of one image - optional un-scaling, filter_small_boxes, score >=
VALID_CONFIDENCE, merge_intersecting_boxes, score >= DETECT_THRESHOLD, boxes_to_polygons, argmax text decode and text-score
filter - written from the semantics (glass_amd/postprocess/post_processor_rotated_boxes.py's host functions, which mirror
reference post_processor_rotated_boxes.py:66-286, and the header comment of csrc/postprocess.hip), not from either kernel.
It starts from the float32 inputs, computes in float64, and rounds to float32 exactly where the reference's float32 tensors
do: the un-scaled boxes and every merged box that is written back.  Its IoU is known_answers.iou_f64 (Sutherland-Hodgman
clipping), evaluated only for pairs whose circumscribed circles overlap (exactly 0 otherwise); its minimum-area rectangle
is oracle/min_area_rect.py's brute force with return_gap=True.

Case builders.  The post-processor is a chain of threshold decisions, so a case is only usable when, along the
reference's WHOLE trajectory (every merge iteration), no decision sits closer to its boundary than float32 resolves.
`reference_image(check=True)` raises MarginError at the first decision inside these margins, and every builder draws
from a fixed seed and redraws the image until none is raised; a builder that runs out of draws fails.  Nothing is skipped
or masked when results are compared.

  MARGIN = 1e-3  on IoA vs minimal_ioa and MERGE_IOA_THRESH, on IoU vs 0.99, on the height ratio vs both bounds, on scores
                 vs VALID_CONFIDENCE / DETECT_THRESHOLD; in degrees on the angle test and on the four branch boundaries of
                 the orientation correction (and on the +-180 wrap of the merged angle); in pixels on MIN_BOX_DIMENSION;
                 relative on the word score vs TEXT_THRESHOLD
  RECT_GAP = 1e-6  relative gap between the best and the next distinct rectangle area of a merge
  PARALLEL_MARGIN = 0.05 degrees between the directions (mod 90) of two INTERSECTING boxes that are not bit-equal.  The
                 post-processor's IoU is detectron2's float32 polygon clipping (csrc/rotated_iou.h restates it): an edge
                 crossing is t = cross / det with det = |e1| |e2| sin(d_angle), and the cross products of 300-px edges carry
                 about |e|^2 2^-23 = 1e-2 of rounding, so below ~1e-3 rad the crossing of two near-parallel edges - a corner
                 of the intersection polygon when the boxes nearly coincide - is not resolved in float32.  Such pairs arise
                 when two merges of one iteration share their defining hull edge; on one (true IoU 0.9961, directions
                 2.9e-5 degrees apart) detectron2's own CPU op returns 0.8535, on the other side of the 0.99 test.  A decision
                 the reference's float32 IoU cannot resolve is no test of the kernel, so such draws are rejected like any
                 other margin.  Bit-equal boxes (both elements of a merged pair) are fine: every det is exactly 0, the
                 crossings are skipped and the corners-inside tests give IoU 1.
  scores         all distinct (no case here is about ties)
"""
import functools
import math

import numpy as np

from known_answers import iou_f64
from oracle.min_area_rect import min_area_rect_bruteforce

MARGIN = 1e-3
RECT_GAP = 1e-6
PARALLEL_MARGIN = 0.05
NMS_IOU = 0.99
# MIN_BOX_DIMENSION, VALID_CONFIDENCE, DETECT_THRESHOLD, MERGE_IOA_THRESH, PAIRS_HEIGHT_RATIO_THRESH, MAX_ANGLE_DIFF,
# minimal_ioa, TEXT_THRESHOLD: the shipped configuration (glass_amd/config/defaults.py add_post_process_config)
THRESHOLDS = (2.0, 0.15, 0.25, 0.3, 0.35, 15.0, 0.01, 0.25)
STOP, CLASSES = 94, 97


class MarginError(Exception):
    pass


def _f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def polygon_f64(b):
    """boxes_to_polygons (:219-250) of one box"""
    cx, cy, w, h, a = (float(v) for v in b)
    t = (-a / 180.0) * math.pi
    s, c = math.sin(t), math.cos(t)
    return np.array([[cx + (h * s - w * c) / 2, cy - (h * c + w * s) / 2], [cx + (h * s + w * c) / 2, cy - (h * c - w * s) / 2],
                     [cx - (h * s - w * c) / 2, cy + (h * c + w * s) / 2], [cx - (h * s + w * c) / 2, cy + (h * c - w * s) / 2]])


def unscale_f64(b, sx, sy):
    """RotatedBoxes.scale (detectron2 structures/rotated_boxes.py), as GlassRunner's un-scaling applies it"""
    cx, cy, w, h, a = (float(v) for v in b)
    t = a * math.pi / 180.0
    c, s = math.cos(t), math.sin(t)
    return np.array([cx * sx, cy * sy, w * math.sqrt((sx * c) ** 2 + (sy * s) ** 2), h * math.sqrt((sx * s) ** 2 + (sy * c) ** 2),
                     math.atan2(sx * s, sy * c) * 180.0 / math.pi])


class _Iou:
    """iou_f64 of the pairs whose circumscribed circles overlap, cached by the boxes' float32 bits (most boxes do not change
    from one merge iteration to the next)"""

    def __init__(self):
        self.cache = {}

    def near_pairs(self, B):
        n = len(B)
        if n < 2:
            return []
        r = 0.5 * np.hypot(B[:, 2], B[:, 3])
        d2 = (B[:, None, 0] - B[None, :, 0]) ** 2 + (B[:, None, 1] - B[None, :, 1]) ** 2
        i, j = np.nonzero(np.triu(d2 <= (r[:, None] + r[None, :]) ** 2, 1))
        return list(zip(i.tolist(), j.tolist()))                      # row-major

    def __call__(self, b1, b2, viol=None):
        key = (b1.astype(np.float32).tobytes(), b2.astype(np.float32).tobytes())
        v = self.cache.get(key)
        if v is None:
            v = self.cache[key] = iou_f64(b1, b2)
        if viol is not None and v > 0 and key[0] != key[1]:
            d = abs((b1[4] - b2[4] + 45.0) % 90.0 - 45.0)
            if d < PARALLEL_MARGIN:
                viol(f"intersecting boxes parallel to {d} degrees")
        return v


def merge_pair_f64(b1, b2, s1, s2, viol):
    """_merge_rotated_boxes (:187-216) + polygons_to_rotated_boxes (:253-286) for one pair"""
    pts = np.concatenate([polygon_f64(b1), polygon_f64(b2)])
    ((cx, cy), (w, h), ang), gap = min_area_rect_bruteforce(pts, return_gap=True)
    if not gap >= RECT_GAP * w * h:
        viol(f"rectangle areas {w * h} and +{gap}")
    orient = (b1[4] if s1 >= s2 else b2[4]) * math.pi / 180.0          # radians into a degree-valued test (reference quirk)
    angle = 90.0 - ang
    diff = (orient - angle + 180.0) % 360.0 - 180.0
    for edge in (-135.0, -45.0, 45.0, 135.0):
        if abs(diff - edge) < MARGIN:
            viol(f"orientation branch {diff}")
    if -45 < diff <= 45:
        width, height = h, w
    elif 45 < diff <= 135:
        width, height = w, h
        angle += 90
    elif -135 < diff <= -45:
        width, height = w, h
        angle -= 90
    else:
        width, height = h, w
        angle += 180
    angle = (angle + 180.0) % 360.0 - 180.0
    if abs(angle) > 180.0 - MARGIN:
        viol(f"merged angle {angle} at the wrap")
    return _f32([cx, cy, width, height, angle])


def reference_image(boxes, scores, text=None, scale=None, thresholds=THRESHOLDS, stop=STOP, check=True):
    """One image: boxes float32 [n,5], scores float32 [n], text float32 [n,T,C] | None, scale (sx, sy) | None.
    Returns dict(boxes [m,5], scores [m], polygons [m,4,2], src [m], char [m,T], text_score [m], text_len [m], stats)."""
    min_dim, valid, detect, merge_ioa, hratio, max_ang, minimal_ioa, text_thr = (float(np.float32(v)) for v in thresholds)

    def viol(msg):
        if check:
            raise MarginError(msg)

    def near(v, t, what):
        if abs(v - t) < MARGIN:
            viol(f"{what}: {v} vs {t}")

    B = np.asarray(boxes, dtype=np.float32).astype(np.float64).reshape(-1, 5)
    S = np.asarray(scores, dtype=np.float32).astype(np.float64).reshape(-1)
    if scale is not None and (np.float32(scale[0]) != 1 or np.float32(scale[1]) != 1):
        sx, sy = float(np.float32(scale[0])), float(np.float32(scale[1]))
        B = _f32(np.array([unscale_f64(b, sx, sy) for b in B]).reshape(-1, 5))
    if check and len(np.unique(S)) != len(S):
        viol("scores not distinct")
    keep = []
    for k in range(len(B)):
        near(min(B[k, 2], B[k, 3]), min_dim, "min box dim")
        near(S[k], valid, "valid score")
        near(S[k], detect, "detect score")
        if min(B[k, 2], B[k, 3]) >= min_dim and S[k] >= valid:
            keep.append(k)
    src = np.array(keep, dtype=np.int64)
    B, S = B[src].copy(), S[src].copy()
    stats = {"n0": len(B), "iters": 0, "merges": 0, "removed": 0, "writeback_rule": False, "reordered": False, "near_pairs": 0}
    iou = _Iou()
    while len(B):
        npairs = iou.near_pairs(B)
        stats["near_pairs"] = max(stats["near_pairs"], len(npairs))
        valid_pairs = []
        for i, j in npairs:
            u = iou(B[i], B[j], viol)
            a1, a2 = B[i, 2] * B[i, 3], B[j, 2] * B[j, 3]
            ioa = (a1 + a2) * u / (1.0 + u) / min(a1, a2)               # pairwise_ioa_rotated (glass/structures/boxes.py:33-48)
            near(ioa, minimal_ioa, "minimal IoA")
            if ioa < minimal_ioa:
                continue
            ad = abs((B[j, 4] - B[i, 4] + 180.0) % 360.0 - 180.0)
            near(ad, max_ang, "angle")
            near(ad, 180.0 - max_ang, "angle")
            hr = B[j, 3] / B[i, 3]
            near(hr, hratio, "height ratio")
            near(hr, 1.0 / (hratio + 1e-6), "height ratio")
            near(ioa, merge_ioa, "merge IoA")
            if ((ad < max_ang or ad > 180.0 - max_ang) and hratio < hr < 1.0 / (hratio + 1e-6) and min(S[i], S[j]) >= valid
                    and ioa >= merge_ioa):
                valid_pairs.append((i, j))
        if not valid_pairs:
            break
        stats["iters"] += 1
        stats["merges"] += len(valid_pairs)
        merged = [merge_pair_f64(B[i], B[j], S[i], S[j], viol) for i, j in valid_pairs]
        as_first, as_second = {}, {}
        for i, j in valid_pairs:
            as_first[i] = as_first.get(i, 0) + 1
            as_second[j] = as_second.get(j, 0) + 1
        if any(as_second.get(b, 0) >= 2 and as_first.get(b, 0) >= 1 for b in as_second):
            stats["writeback_rule"] = True
        new = B.copy()
        for (i, _), m in zip(valid_pairs, merged):                       # tensor[pairs[:, 0]] = merged     (last wins)
            new[i] = m
        for (_, j), m in zip(valid_pairs, merged):                       # tensor[pairs[:, 1]] = merged.clone()
            new[j] = m
        B = new
        # nms_rotated(0.99): stable descending score order, greedy
        hi = {}
        for i, j in iou.near_pairs(B):
            u = iou(B[i], B[j], viol)
            near(u, NMS_IOU, "NMS IoU")
            if u >= NMS_IOU:
                hi.setdefault(i, set()).add(j)
                hi.setdefault(j, set()).add(i)
        order = sorted(range(len(B)), key=lambda k: (-S[k], k))
        kept = []
        for k in order:
            if not any(a in hi.get(k, ()) for a in kept):
                kept.append(k)
        stats["removed"] += len(B) - len(kept)
        if kept != sorted(kept):
            stats["reordered"] = True
        kept = np.array(kept, dtype=np.int64)
        B, S, src = B[kept], S[kept], src[kept]
    n = len(B)
    T = 0 if text is None else int(text.shape[1])
    char = np.zeros((n, max(T, 1)), dtype=np.int64)
    tscore, tlen = np.ones(n), np.zeros(n, dtype=np.int64)
    final = []
    for k in range(n):
        ok = S[k] >= detect
        if text is not None:
            row = np.asarray(text[src[k]], dtype=np.float32)
            char[k] = row.argmax(1)                                      # the first maximum, as torch.max
            p = row.max(1).astype(np.float64)
            stops = np.nonzero(char[k] == stop)[0]
            upto = int(stops[0]) + 1 if len(stops) else T                 # up to and including the stop symbol
            tlen[k] = int(stops[0]) if len(stops) else T
            tscore[k] = float(np.prod(p[:upto]))
            if abs(tscore[k] - text_thr) < MARGIN * text_thr:
                viol(f"text score {tscore[k]}")
            ok = ok and tscore[k] >= text_thr
        if ok:
            final.append(k)
    final = np.array(final, dtype=np.int64)
    B, S = B[final].reshape(-1, 5), S[final]
    return {"boxes": B, "scores": S, "polygons": np.array([polygon_f64(b) for b in B]).reshape(-1, 4, 2), "src": src[final],
            "char": char[final], "text_score": tscore[final], "text_len": tlen[final], "stats": stats}


# ------------------------------------------------------------------------------------------------ scenes
def _clusters(g):
    """The merge structures every non-trivial scene carries, in input order (relative order is kept when they are spread
    over the image's slots).  Local coordinates; each cluster is shifted to its own place."""
    out = []
    # near-duplicates forced as in test_device_postprocessor_equals_host_restatement_with_text: b, b + small offset
    for k in range(3):
        b = np.array([200.0 + 260 * k + g.uniform(-3, 3), 90.0 + g.uniform(-3, 3), g.uniform(70, 110), g.uniform(20, 30), g.uniform(-12, 12)])
        d = np.array([8.0, 1.0, 2.0, 0.5, 1.0]) if k != 1 else np.array([-6.0, 0.5, -3.0, 0.2, -2.0])
        out += [b, b + d + g.uniform(-0.2, 0.2, 5)]
    # a chain of 6 boxes along a 20-degree line plus a crossing box: merges cascade over several iterations
    ang = math.radians(20.0)
    x0, y0 = 1100.0 + g.uniform(-3, 3), 420.0 + g.uniform(-3, 3)
    out += [np.array([x0 + 50 * i * math.cos(ang), y0 - 50 * i * math.sin(ang), 90.0 + g.uniform(-1, 1), 24.0 + i, 20.0 + 0.5 * i])
            for i in range(6)]
    out.append(np.array([x0 + 100.0, y0 - 40.0, 90.0, 24.0, -70.0]))
    # the write-back rule: a long box that is SECOND element of two valid pairs (two short boxes inside it, earlier in the
    # order) and FIRST element of another (a third short box, later in the order)
    cx, cy, a = 1800.0 + g.uniform(-3, 3), 120.0 + g.uniform(-3, 3), g.uniform(-6, 6)
    t = math.radians(a)
    along = lambda d: (cx + d * math.cos(t), cy - d * math.sin(t))
    out.append(np.array([*along(-70.0), 50.0 + g.uniform(-2, 2), 23.0, a + 1.0]))
    out.append(np.array([*along(2.0), 50.0 + g.uniform(-2, 2), 24.5, a - 1.0]))
    out.append(np.array([cx, cy, 200.0, 24.0, a]))
    out.append(np.array([*along(70.0), 50.0 + g.uniform(-2, 2), 23.5, a + 0.5]))
    # the small-box filter: two boxes below MIN_BOX_DIMENSION
    out.append(np.array([2300.0, 100.0, 60.0, 1.2, 3.0]))
    out.append(np.array([2300.0, 200.0, 1.5, 30.0, -4.0]))
    return out


def _scene(g, count, kind, scale):
    """`count` boxes + scores.  kind "sparse": a grid of words whose neighbours' circumscribed circles overlap along the rows
    but whose rectangles do not (near pairs, IoU 0: nothing merges).  kind "mixed": a grid of words with disjoint circles
    plus the clusters above, spread over the slots in their own order.  With un-scaling the scene is drawn in output
    coordinates and divided by the scale, so the kernel's un-scaling brings it back."""
    if count == 0:
        return np.zeros((0, 5), np.float32), np.zeros((0,), np.float32)
    cl = _clusters(g) if (kind == "mixed" and count >= 64) else []
    ngrid = count - len(cl)
    cols = max(1, int(math.ceil(math.sqrt(ngrid))))
    pitch_x, pitch_y = (48.0, 74.0) if kind == "sparse" else (74.0, 74.0)
    grid = []
    for k in range(ngrid):
        r, c = divmod(k, cols)
        # sparse: near-square words 48 px apart - circles (diameter ~ 56) overlap, rectangles (extent <= 43 at 4 degrees) do not
        w, h, a = ((g.uniform(38, 42), g.uniform(36, 40), g.uniform(-4, 4)) if kind == "sparse" else
                   (g.uniform(40, 64), g.uniform(14, 24), g.uniform(-8, 8)))
        grid.append(np.array([60.0 + pitch_x * c + g.uniform(-1, 1), 700.0 + pitch_y * r + g.uniform(-1, 1), w, h, a]))
    slots = np.sort(g.choice(count, size=len(cl), replace=False)) if cl else np.array([], dtype=np.int64)
    boxes = np.zeros((count, 5))
    isc = np.zeros(count, dtype=bool)
    isc[slots] = True
    boxes[isc] = np.array(cl).reshape(-1, 5)
    boxes[~isc] = np.array(grid).reshape(-1, 5)
    if scale is not None:
        sx, sy = scale
        boxes = np.array([unscale_f64(b, 1.0 / sx, 1.0 / sy) for b in boxes])
    # distinct scores away from the thresholds; grid words also below VALID_CONFIDENCE and between it and DETECT_THRESHOLD,
    # cluster boxes above both so the structures survive the filters
    scores = np.where(isc, g.uniform(0.3, 0.94, count), g.uniform(0.06, 0.94, count)).astype(np.float32)
    while True:
        bad = (np.abs(scores - 0.15) < 2 * MARGIN) | (np.abs(scores - 0.25) < 2 * MARGIN)
        _, first = np.unique(scores, return_index=True)
        bad[np.setdiff1d(np.arange(count), first)] = True
        if not bad.any():
            break
        scores[bad] = g.uniform(0.3, 0.94, int(bad.sum())).astype(np.float32)
    return boxes.astype(np.float32), scores


def _text(g, K, count, T):
    """peaked character distributions [K,T,C]; two boxes in three have a stop symbol somewhere, the third has none"""
    text = np.zeros((K, T, CLASSES), dtype=np.float32)
    if count == 0:
        return text
    p = g.uniform(0.955, 0.9995, (count, T)).astype(np.float32)
    peak = g.integers(0, STOP, (count, T))
    stop_at = g.integers(1, T, count)
    for k in range(count):
        if k % 3 != 2:
            peak[k, stop_at[k]] = STOP
    text[:count] = ((1.0 - p) / (CLASSES - 1))[:, :, None]
    np.put_along_axis(text[:count], peak[:, :, None], p[:, :, None], axis=2)
    return text


#           name: (seed, K, counts, kind, scale or None, T)
CASE_SPECS = {
    "small_mixed": (11, 128, (128, 100, 1, 0), "mixed", None, 26),            # fits both kernels
    "small_scaled": (12, 128, (0, 128, 77), "mixed", (1.25, 1.2), 51),
    "k129_mixed": (21, 129, (129, 128, 1, 0), "mixed", (1.25, 1.2), 51),
    "k129_sparse": (22, 129, (0, 129, 128, 1), "sparse", None, 26),
    "k300_mixed": (31, 300, (257, 256, 193, 192), "mixed", None, 26),
    "k300_sparse": (32, 300, (192, 193, 256, 257), "sparse", (1.25, 1.2), 51),
    "k1024_mixed": (41, 1024, (1024, 1023, 513, 512), "mixed", (1.25, 1.2), 26),
    "k1024_sparse": (42, 1024, (512, 513, 1023, 1024), "sparse", None, 51),
    "k1024_cascade": (43, 1024, (1024,), "mixed", None, 26),                  # the determinism case
}
SMALL_CASES = ("small_mixed", "small_scaled")
DENSE_CASES = tuple(k for k in CASE_SPECS if k not in SMALL_CASES)
MAX_DRAWS = 60


def draw_image(key, count, kind, scale, K, T):
    """One image inside the margins: (boxes [count,5], scores [count], text [K,T,C], reference dict, number of draws).
    `key`: the seed sequence; draw d uses default_rng([*key, d])."""
    for draw in range(MAX_DRAWS):
        g = np.random.default_rng([*key, draw])
        b, s = _scene(g, count, kind, scale)
        tx = _text(g, K, count, T)
        try:
            ref = reference_image(b, s, tx[:count], scale)
        except MarginError:
            continue
        break
    else:
        raise AssertionError(f"image {key} ({count} {kind} boxes): no draw inside the margins in {MAX_DRAWS} tries")
    st = ref["stats"]
    if kind == "mixed" and count >= 64:
        assert st["iters"] >= 3 and st["merges"] >= 8 and st["removed"] >= 8, (key, st)      # the chain cascades
        assert st["writeback_rule"] and st["reordered"], (key, st)
    if kind == "sparse":
        assert st["iters"] == 0 and (count < 64 or st["near_pairs"] >= count // 2), (key, st)
    return b, s, tx, ref, draw + 1


@functools.lru_cache(maxsize=None)
def build_case(name):
    """dict(K, T, boxes [N,K,5], scores [N,K], counts [N], text [N,K,T,C], scale_xy [N,2] | None, ref [N] reference dicts,
    draws [N]).  Raises AssertionError when an image cannot be drawn inside the margins, or lacks what its kind promises."""
    seed, K, counts, kind, scale, T = CASE_SPECS[name]
    N = len(counts)
    boxes = np.zeros((N, K, 5), np.float32)
    scores = np.zeros((N, K), np.float32)
    text = np.zeros((N, K, T, CLASSES), np.float32)
    refs, draws = [], []
    for n, count in enumerate(counts):
        boxes[n, :count], scores[n, :count], text[n], ref, d = draw_image((seed, n), count, kind, scale, K, T)
        refs.append(ref)
        draws.append(d)
    scale_xy = None if scale is None else np.tile(np.array(scale, np.float32), (N, 1))
    return {"name": name, "K": K, "T": T, "boxes": boxes, "scores": scores, "counts": np.array(counts, np.int32), "text": text,
            "scale_xy": scale_xy, "ref": refs, "draws": draws}


def pad_case(case, K):
    """the same inputs zero-padded to a wider K"""
    N, K0 = case["scores"].shape
    assert K >= K0
    out = dict(case, K=K)
    for k in ("boxes", "scores", "text"):
        a = case[k]
        p = np.zeros((N, K) + a.shape[2:], a.dtype)
        p[:, :K0] = a
        out[k] = p
    return out
