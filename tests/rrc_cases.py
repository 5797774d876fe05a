"""Exact checker and seeded cases for the RRC scorer tests (tests/test_rrc_score.py, tests/test_gpu_rrc_score.py).

The reference scorer cannot be run (its `Polygon` and `Levenshtein` C packages are absent), so expected values come from
this file:
  * `exact_intersection`: intersection area of two simple integer polygons by vertical-slab decomposition in
    `fractions.Fraction`.  The x axis is cut at every vertex abscissa and every edge-edge crossing; inside a slab no two
    edges cross, so each polygon is a stack of trapezoids between consecutive edges (even-odd) and the overlap of two
    stacks is a sum of trapezoids.  Exact on integer input, and a different algorithm from the kernel's (which sums a
    closed form over edge pairs and never cuts anything).
  * `check_score`: the protocol (don't-care marks, greedy matching in GT order, per-image and global tallies, the two
    result lines) written over those exact areas, with comparisons in rational arithmetic.
  * the error bound of the kernel's fp64 formula, `inter_bound`, and the bands around the protocol's two thresholds in
    which an fp64 decision may differ from the exact one (`iou_band`, `dontcare_band`).
  * seeded cases.  The large decisions case takes the checker several seconds per run, so its answers are recorded in
    tests/golden/rrc_decisions.json with a digest of the generated files; regenerate with `python tests/rrc_cases.py`.

Parsing and the word-spotting string rules are taken from glass_amd.evaluation.rrc_score (tables in
tests/test_rrc_score.py pin them); geometry, decisions and tallies here share nothing with it.
"""
import hashlib
import json
import math
import os
import random
import sys
from collections import OrderedDict
from fractions import Fraction as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_DECISIONS = os.path.join(ROOT, "tests", "golden", "rrc_decisions.json")

# ---------------------------------------------------------------------------------------------------- error bound
# Bound on |inter_fp64 - inter_exact| for the kernel's formula (csrc/rrc_score.hip), u = 2^-53, W x H the joint bounding
# box, shifted coordinates exact integers in [0, W] x [0, H].  First order in u, per edge pair with x-overlap dx <= W:
#   slope m = dy / dx_e: 1 rounding.  Height a = y1 + (x - x1) * m: |(x - x1) * m| <= H, so the slope's and the product's
#   roundings give 2 H u and the sum (|a| <= H) one more: each of the four heights is off by <= 3 H u.
#   s = (a0 + a1 + b0 + b1) / 4 * dx: inputs 12 H u, three additions of values <= 4 H: 12 H u, /4 exact: 6 H u, times
#   dx with one rounding of a value <= H dx: <= 7 H dx u.
#   d0 = a0 - b0, d1 = a1 - b1: 6 H u inherited + 1 H u each.  The integral of |a - b| as a function of (d0, d1) is
#   continuous across the crossing / non-crossing branches with |partial derivative| <= dx / 2 in each argument, so the
#   inherited error is <= 7 H dx u whichever branch the rounded signs select; evaluating the branch costs at most 5
#   roundings of a value <= H dx: 12 H dx u on the integral, 6 H dx u on its half.
#   term = s - half: one rounding of a value <= H dx.  Per term: (7 + 6 + 1) H dx u = 14 W H u.
# Summation: each lane adds its terms with Kahan's compensated sum, error <= (2 u + O(n u^2)) * sum |term| (Higham,
# Accuracy and Stability of Numerical Algorithms, 4.3), then a shuffle tree of at most 6 levels, each <= u * sum |term|;
# |term| <= W H.  Summation: 8 W H u per term.  The orientation factor is +-1 and the clamp at 0 only moves towards the
# exact value (>= 0).  Total first order: 22 u ne nf W H; c = 32 leaves room for the second-order terms and for fused
# multiply-adds being rounded differently from the two-step count above.  It is not fitted to any output.
BOUND_C = 32


def inter_bound(A, B):
    """c * 2^-53 * ne * nf * W * H for two rings [(x, y), ...]."""
    xs, ys = [p[0] for p in A] + [p[0] for p in B], [p[1] for p in A] + [p[1] for p in B]
    return BOUND_C * 2.0 ** -53 * len(A) * len(B) * max(max(xs) - min(xs), 1) * max(max(ys) - min(ys), 1)


def iou_band(bound, union):
    """fp64 `inter / (ag + ad - inter) > 0.5` may differ from the exact decision only if |2 I - U| is inside this band:
    2 I' - U' moves by 3 * bound with the error of I', by 2 u U for the two roundings of the union, and the division
    (one rounding of a quotient near 1/2) can hide a further 2 u U; 8 u U covers both with room."""
    return 3 * bound + 8 * 2.0 ** -53 * float(union)


def dontcare_band(bound, area_d):
    """The same for `inter / area_d > 0.5` on 2 I - area_d: 2 * bound, and the division's rounding, 2 u area_d (4 taken)."""
    return 2 * bound + 4 * 2.0 ** -53 * float(area_d)


# ------------------------------------------------------------------------------------------------- exact geometry

def ring(flat):
    return [(int(flat[i]), int(flat[i + 1])) for i in range(0, len(flat), 2)]


def shoelace2(P):
    return sum(P[i][0] * P[(i + 1) % len(P)][1] - P[(i + 1) % len(P)][0] * P[i][1] for i in range(len(P)))


def exact_area(P):
    return F(abs(shoelace2(P)), 2)


def _edges(P):
    out = []
    for i in range(len(P)):
        (x1, y1), (x2, y2) = P[i], P[(i + 1) % len(P)]
        if x1 != x2:                                            # vertical edges bound no area under them
            out.append((x1, y1, x2, y2) if x1 < x2 else (x2, y2, x1, y1))
    return out


def _y_at(e, x):
    return e[1] + F(e[3] - e[1], e[2] - e[0]) * (x - e[0])


def _crossing_x(e, f):
    """abscissa where two non-vertical segments meet in a single point, or None"""
    dxe, dye, dxf, dyf = e[2] - e[0], e[3] - e[1], f[2] - f[0], f[3] - f[1]
    den = dxe * dyf - dye * dxf
    if den == 0:
        return None
    t = F((f[0] - e[0]) * dyf - (f[1] - e[1]) * dxf, den)
    x = e[0] + t * dxe
    return x if max(e[0], f[0]) <= x <= min(e[2], f[2]) else None


def _stack(edges, xl, xr, xm):
    """the polygon inside the slab: [(lower edge, upper edge), ...] by the even-odd rule"""
    span = sorted((e for e in edges if e[0] <= xl and e[2] >= xr), key=lambda e: (_y_at(e, xm), _y_at(e, xl), _y_at(e, xr)))
    assert len(span) % 2 == 0, "ring is not closed"
    return [(span[i], span[i + 1]) for i in range(0, len(span), 2)]


def exact_intersection(A, B):
    """Area of the intersection of two simple rings with integer vertices, as a Fraction."""
    if min(max(p[0] for p in A), max(p[0] for p in B)) <= max(min(p[0] for p in A), min(p[0] for p in B)) or \
            min(max(p[1] for p in A), max(p[1] for p in B)) <= max(min(p[1] for p in A), min(p[1] for p in B)):
        return F(0)
    ea, eb = _edges(A), _edges(B)
    cuts = {F(p[0]) for p in A} | {F(p[0]) for p in B}
    every = ea + eb
    for i in range(len(every)):
        for j in range(i + 1, len(every)):
            if every[i][2] > every[j][0] and every[j][2] > every[i][0]:
                x = _crossing_x(every[i], every[j])
                if x is not None:
                    cuts.add(x)
    cuts = sorted(cuts)
    total = F(0)
    for xl, xr in zip(cuts, cuts[1:]):
        xm = (xl + xr) / 2
        sa, sb = _stack(ea, xl, xr, xm), _stack(eb, xl, xr, xm)
        for la, ua in sa:
            for lb, ub in sb:
                lo = la if _y_at(la, xm) >= _y_at(lb, xm) else lb
                hi = ua if _y_at(ua, xm) <= _y_at(ub, xm) else ub
                if _y_at(hi, xm) > _y_at(lo, xm):
                    total += ((_y_at(hi, xl) - _y_at(lo, xl)) + (_y_at(hi, xr) - _y_at(lo, xr))) / 2 * (xr - xl)
    return total


# ------------------------------------------------------------------------------------------------ exact protocol

def exact_image(gt_rings, det_rings):
    """(areas of GT, areas of detections, inter [G][D]) as Fractions"""
    return ([exact_area(g) for g in gt_rings], [exact_area(d) for d in det_rings],
            [[exact_intersection(g, d) for d in det_rings] for g in gt_rings])


def decide(ag, ad, inter, gt_dc):
    """don't-care detections and the greedy matching of one care set over exact areas"""
    G, D = len(ag), len(ad)
    det_dc = []
    for d in range(D):
        hit = any(gt_dc[g] and ad[d] != 0 and inter[g][d] / ad[d] > F(1, 2) for g in range(G))
        det_dc.append(1 if hit else 0)
    match, used = [-1] * G, [False] * D
    for g in range(G):
        if gt_dc[g]:
            continue
        for d in range(D):
            if used[d] or det_dc[d]:
                continue
            union = ag[g] + ad[d] - inter[g][d]
            if union != 0 and inter[g][d] / union > F(1, 2):
                match[g], used[d] = d, True
                break
    return det_dc, match


def _prh(correct, n_gt, n_det):
    if n_gt == 0:
        r, p = 1.0, (0.0 if n_det > 0 else 1.0)
    else:
        r, p = correct / n_gt, (0 if n_det == 0 else correct / n_det)
    return p, r, (0 if p + r == 0 else 2.0 * p * r / (p + r))


def _method(tag, matched, n_gt, n_det):
    r = 0 if n_gt == 0 else matched / n_gt
    p = 0 if n_det == 0 else matched / n_det
    h = 0 if r + p == 0 else 2 * r * p / (r + p)
    return f"{tag}: precision: {p}, recall: {r}, hmean: {h}"


def check_score(gt, submission, word_spotting, geometry=None):
    """The expected result dictionary.  gt: {key: (rings as flat lists, transcriptions)}; submission: {key: [lines]};
    geometry: optional {key: exact_image(...)} computed earlier.  iouMat holds Fractions; 'decisions' is added per
    sample: (det_dc_e2e, det_dc_det, match_e2e, match_det)."""
    from glass_amd.evaluation import rrc_score as R
    for key in submission:
        if key not in gt:
            raise ValueError("The sample %s not present in GT" % key)
    per_sample, tot = OrderedDict(), [0] * 6
    for key, (rings, texts) in gt.items():
        trans, dc_e2e, dc_det = R.ground_truth_care(texts, word_spotting)
        dets = [R.parse_detection_line(l) for l in submission.get(key, [])]
        gr, dr = [ring(p) for p in rings], [ring(p) for p, _ in dets]
        ag, ad, inter = (geometry or {}).get(key) or exact_image(gr, dr)
        ddc_e, m_e = decide(ag, ad, inter, dc_e2e)
        ddc_d, m_d = decide(ag, ad, inter, dc_det)
        correct = 0
        for g, d in enumerate(m_e):
            if d >= 0:
                a, b = trans[g].upper().replace("####", ""), dets[d][1].upper()
                correct += (a == b) if word_spotting else R.transcription_match(a, b)
        n = (correct, len(gr) - sum(dc_e2e), len(dr) - sum(ddc_e), sum(d >= 0 for d in m_d), len(gr) - sum(dc_det),
             len(dr) - sum(ddc_d))
        tot = [a + b for a, b in zip(tot, n)]
        p, r, h = _prh(n[0], n[1], n[2])
        iou = []
        if gr and dr and len(dr) <= 100:
            iou = [[(inter[g][d] / (ag[g] + ad[d] - inter[g][d])) if ag[g] + ad[d] - inter[g][d] != 0 else F(0)
                    for d in range(len(dr))] for g in range(len(gr))]
        per_sample[key] = {"precision": p, "recall": r, "hmean": h, "iouMat": iou,
                           "gtPolPoints": [[float(v) for v in q] for q in rings],
                           "detPolPoints": [[float(v) for v in q] for q, _ in dets], "gtTrans": trans,
                           "detTrans": [t for _, t in dets], "gtDontCare": [g for g, f in enumerate(dc_e2e) if f],
                           "detDontCare": [d for d, f in enumerate(ddc_e) if f], "decisions": (ddc_e, ddc_d, m_e, m_d)}
    return {"calculated": True, "Message": "", "e2e_method": _method("E2E_RESULTS", *tot[:3]),
            "det_only_method": _method("DETECTION_ONLY_RESULTS", *tot[3:]), "per_sample": per_sample}


# ---------------------------------------------------------------------------------------------------- polygon cases

def _simple(P):
    from glass_amd.evaluation import normalize_detection_line
    if len(set(P)) != len(P):
        return False
    return normalize_detection_line(",".join(f"{x},{y}" for x, y in P) + ",####x") is not None


def star(r, n, cx, cy, rx, ry, convex):
    """n-point ring around (cx, cy): vertices at increasing angles, on the ellipse (convex up to rounding) or at random
    radii (star-shaped, concave); redrawn until it is simple after rounding to integers"""
    for attempt in range(10 ** 6):
        n = max(3, n - (attempt + 1) // 20)                     # a small ellipse has few distinct integer points
        ang = sorted(r.uniform(0, 2 * math.pi) for _ in range(n))
        P = []
        for a in ang:
            k = 1.0 if convex else r.uniform(0.35, 1.0)
            P.append((int(round(cx + k * rx * math.cos(a))), int(round(cy + k * ry * math.sin(a)))))
        if _simple(P):
            return P


def rot_quad(r, cx, cy, w, h, deg):
    t = math.radians(deg)
    c, s = math.cos(t), math.sin(t)
    return [(int(round(cx + (a * w * c - b * h * s) / 2)), int(round(cy + (a * w * s + b * h * c) / 2)))
            for a, b in ((-1, -1), (1, -1), (1, 1), (-1, 1))]


def area_pairs(seed=20261016):
    """[(name, A, B)]: pairs of simple rings for the intersection-area test"""
    r = random.Random(seed)
    rect = lambda x, y, w, h: [(x, y), (x + w, y), (x + w, y + h), (x, y + h)]
    L = [(0, 0), (10, 0), (10, 4), (4, 4), (4, 10), (0, 10)]
    out = [("offset squares", rect(0, 0, 10, 10), rect(5, 5, 10, 10)), ("square in L", L, rect(2, 2, 6, 6)),
           ("reversed", rect(0, 0, 10, 10), rect(5, 5, 10, 10)[::-1]), ("triangle square", [(0, 0), (10, 0), (0, 10)], rect(0, 0, 5, 5)),
           ("shared hypotenuse", [(0, 0), (10, 0), (0, 10)], [(10, 10), (0, 10), (10, 0)]), ("disjoint", rect(0, 0, 10, 10), rect(20, 0, 3, 3)),
           ("touching boxes", rect(0, 0, 10, 10), rect(10, 0, 10, 10)), ("identical", L, list(L)), ("nested", rect(0, 0, 100, 100), rect(40, 40, 5, 5)),
           ("shared edge inside", rect(0, 0, 10, 10), rect(0, 0, 10, 4)), ("shared vertex", rect(0, 0, 10, 10), [(10, 10), (20, 12), (12, 20)]),
           ("closed ring", rect(0, 0, 10, 10) + [(0, 0)], rect(5, 5, 10, 10) + [(5, 5)]),
           ("near parallel", [(0, 0), (100000, 1), (100000, 3), (0, 2)], [(0, 1), (100000, 1), (100000, 2), (0, 3)]),
           ("near parallel 2", [(0, 0), (99991, 7), (99991, 9), (0, 2)], [(3, 1), (100003, 7), (100003, 9), (3, 3)]),
           ("tiny", [(0, 0), (1, 0), (1, 1)], [(0, 0), (1, 1), (0, 1), ][::-1]), ("tiny 2", rect(7, 7, 1, 1), rect(7, 7, 2, 1)),
           ("image sized", rect(-1048576, -1048576, 2097152, 2097152), [(-1048576, 0), (0, -1048576), (1048576, 0), (0, 1048576)]),
           ("comb", [(0, 0), (12, 0), (12, 10), (10, 10), (10, 2), (8, 2), (8, 10), (6, 10), (6, 2), (4, 2), (4, 10), (2, 10), (2, 2), (0, 2)],
            rect(1, 5, 10, 3))]
    for k in range(150):
        na, nb = r.choice([3, 4, 4, 5, 8, 12]), r.choice([3, 4, 4, 6, 10, 16])
        s = r.choice([3, 30, 300, 30000])
        A = star(r, na, r.randint(-s, s), r.randint(-s, s), r.randint(2, 2 * s), r.randint(2, s), r.random() < 0.5)
        B = star(r, nb, A[0][0] + r.randint(-s, s), A[0][1] + r.randint(-s, s), r.randint(2, 2 * s), r.randint(2, s), r.random() < 0.5)
        out.append((f"random {k}", A if r.random() < 0.5 else A[::-1], B if r.random() < 0.5 else B[::-1]))
    for k in range(24):
        na, nb = r.choice([24, 48, 64, 96]), r.choice([20, 64, 80])
        A = star(r, na, 500, 400, r.randint(100, 400), r.randint(40, 200), k % 3 == 0)
        B = star(r, nb, 500 + r.randint(-150, 150), 400 + r.randint(-80, 80), r.randint(100, 400), r.randint(40, 200), k % 2 == 0)
        out.append((f"many points {k}", A, B[::-1] if k % 4 == 0 else B))
    for k in range(12):                                         # rotated word boxes that share a vertex or an edge with a copy
        A = rot_quad(r, 300, 200, r.randint(40, 200), r.randint(10, 60), r.uniform(-60, 60))
        dx, dy = A[1][0] - A[0][0], A[1][1] - A[0][1]
        out.append((f"slid along edge {k}", A, [(x + dx // 2, y + dy // 2) for x, y in A]))
        out.append((f"split by diagonal {k}", A, [A[0], A[1], A[2]]))
    return out


# -------------------------------------------------------------------------------------------------- protocol cases

_WORDS = ["hello", "World", "STOP", "cafe", "it's", "John's", "ab", "A-B", "-dash-", "exit!", "(note)", "two words", "x×y", "Ünï", "street",
          "42nd", "OPEN", "sale", "###"]


def _line(P, text):
    return ",".join(f"{x},{y}" for x, y in P) + ",####" + text


def _clockwise(P):
    """orientation the detection files must have (normalize_detection_line: negative shoelace)"""
    return P[::-1] if shoelace2(P) > 0 else P


def tie_case():
    """Axis-aligned rectangles on the protocol's thresholds, all exactly representable.  Per image: what must happen."""
    rect = lambda x, y, w, h: [x, y, x + w, y, x + w, y + h, x, y + h]
    det = lambda x, y, w, h, t="word": _line(_clockwise(ring(rect(x, y, w, h))), t)
    gt = OrderedDict([
        ("1", ([rect(0, 0, 20, 10)], ["word"])),                 # det 10x10 inside: IoU = 100 / 200 = 0.5 exactly: no match
        ("2", ([rect(0, 0, 20, 10)], ["word"])),                 # det 11x10: IoU = 110 / 200: match
        ("3", ([rect(0, 0, 10, 10)], ["###"])),                  # det half on it: 50 / 100 = 0.5: not don't-care
        ("4", ([rect(0, 0, 10, 10)], ["###"])),                  # 60 / 100: don't-care
        ("5", ([rect(0, 0, 30, 10), rect(0, 0, 30, 10)], ["word", "word"])),   # det 15x10 (0.5) and 30x10: first GT takes det 1
        ("6", ([[10, 10, 50, 10, 90, 10, 50, 10]], ["word"])),   # zero-area GT and a detection over it: union > 0, IoU 0
    ])
    sub = OrderedDict([("1", [det(0, 0, 10, 10)]), ("2", [det(0, 0, 11, 10)]), ("3", [det(5, 0, 10, 10)]), ("4", [det(4, 0, 10, 10)]),
                       ("5", [det(0, 0, 15, 10), det(0, 0, 30, 10)]), ("6", [det(0, 0, 100, 20)])])
    want = {"1": ([0], [0], [-1], [-1]), "2": ([0], [0], [0], [0]), "3": ([0], [0], [-1], [-1]), "4": ([1], [1], [-1], [-1]),
            "5": ([0, 0], [0, 0], [1, -1], [1, -1]), "6": ([0], [0], [-1], [-1])}
    return gt, sub, want


def decisions_case(n_images=220, seed=7, redraws=None):
    """(gt, submission, planted keys, redraws): a multi-image totaltext-style case.  GT words overlap (jittered copies, so
    the greedy order matters), some are don't-care, detections are jittered copies of GT words, boxes over two GT words or
    random; planted images hold the exact ties of `tie_case`, a zero-area GT and an image with more than 100 detections.

    Every polygon k is drawn from its own stream Random((seed, k, attempt)).  With redraws=None the exact checker looks at
    every (GT, detection) pair outside the planted images: a pair whose 2 I - U or 2 I - area_d lies inside the band
    where an fp64 decision may differ from the exact one (`iou_band`, `dontcare_band`) has its detection drawn again
    (attempt + 1), and at most 1 % of the pairs may be redrawn (asserted).  The attempts used are returned and recorded
    in the golden file; passing them back as `redraws` rebuilds the same case without the checker."""
    verify = redraws is None
    redraws = {} if redraws is None else {int(k): int(v) for k, v in redraws.items()}
    tg, ts, _ = tie_case()
    gt, sub, planted = OrderedDict(), OrderedDict(), []
    for i, key in enumerate(tg):
        k7 = "%07d" % (i + 1)
        gt[k7], sub[k7] = tg[key], ts[key]
        planted.append(k7)
    geometry, n_pairs, n_redrawn, poly_id = {}, 0, 0, 0
    master = random.Random(seed)
    for i in range(len(planted), n_images):
        key = "%07d" % (i + 1)
        G = master.choice([0, 1, 2, 3, 4, 5, 6, 8])
        rings, texts = [], []
        for g in range(G):
            r = random.Random(f"{seed}/gt/{i}/{g}")
            if rings and r.random() < 0.3:
                P = [(x + r.randint(-4, 4), y + r.randint(-4, 4)) for x, y in ring(rings[-1])]
                P = P if _simple(P) else ring(rings[-1])
            elif r.random() < 0.25:
                P = star(r, r.randint(6, 14), r.randint(60, 580), r.randint(40, 440), r.randint(20, 80), r.randint(8, 30), False)
            else:
                P = rot_quad(r, r.randint(60, 580), r.randint(40, 440), r.randint(20, 140), r.randint(8, 40), r.uniform(-40, 40))
                if not _simple(P):
                    P = [(10, 10), (60, 12), (58, 30), (9, 28)]
            rings.append([v for p in (P if r.random() < 0.5 else P[::-1]) for v in p])
            texts.append(r.choice(_WORDS))
        gt[key] = (rings, texts)
        if master.random() < 0.06:
            continue                                            # image absent from the submission
        D = master.choice([0, 1, 2, 3, 5, 8, 12])
        gr = [ring(p) for p in rings]
        ag = [exact_area(g) for g in gr]
        lines, dets = [], []
        for d in range(D):
            attempt = redraws.get(poly_id, 0) if not verify else 0
            while True:
                r = random.Random(f"{seed}/det/{i}/{d}/{attempt}")
                u = r.random()
                if gr and u < 0.6:
                    src = r.randrange(len(gr))
                    P = [(x + r.randint(-6, 6), y + r.randint(-6, 6)) for x, y in gr[src]]
                    text = texts[src] if r.random() < 0.7 else r.choice(_WORDS)
                elif len(gr) >= 2 and u < 0.75:
                    a, b = r.sample(range(len(gr)), 2)
                    xs, ys = [p[0] for p in gr[a] + gr[b]], [p[1] for p in gr[a] + gr[b]]
                    P, text = [(min(xs), min(ys)), (max(xs), min(ys)), (max(xs), max(ys)), (min(xs), max(ys))], texts[a]
                else:
                    P = rot_quad(r, r.randint(60, 580), r.randint(40, 440), r.randint(20, 140), r.randint(8, 40), r.uniform(-40, 40))
                    text = r.choice(_WORDS)
                text = "word" if text == "###" else text
                if not _simple(P):
                    attempt += 1                                # an invalid ring is not a detection; not counted as a redraw
                    continue
                P = _clockwise(P)
                if not verify:
                    break
                ad = exact_area(P)
                col = [exact_intersection(g, P) for g in gr]
                bad = False
                for g in range(len(gr)):
                    b = inter_bound(gr[g], P)
                    union = ag[g] + ad - col[g]
                    if abs(2 * col[g] - union) <= iou_band(b, union) or abs(2 * col[g] - ad) <= dontcare_band(b, ad):
                        bad = True
                if not bad:
                    break
                n_redrawn += len(gr)
                attempt += 1
            if verify:
                if attempt:
                    redraws[poly_id] = attempt
                dets.append((ad, col))
            n_pairs += len(gr)
            poly_id += 1
            lines.append(_line(P, text))
        sub[key] = lines
        if verify:
            geometry[key] = (ag, [a for a, _ in dets], [[c[g] for _, c in dets] for g in range(len(gr))])
    # one image with more than 100 detections (iouMat is [] there)
    key = "%07d" % (n_images + 1)
    r = random.Random(f"{seed}/many")
    gt[key] = ([[0, 0, 400, 0, 400, 30, 0, 30], [0, 100, 50, 100, 50, 120, 0, 120]], ["long", "###"])
    sub[key] = [_line(_clockwise([(4 * d, 1 + d % 3), (4 * d + 3, 1 + d % 3), (4 * d + 3, 20), (4 * d, 20)]), "x") for d in range(100)] + \
               [_line(_clockwise([(1, 1), (399, 2), (398, 29), (2, 28)]), "LONG")]
    planted.append(key)
    decisions_case.geometry = geometry                          # exact areas of the verified images, for check_score
    if verify:
        assert n_redrawn * 100 <= n_pairs, f"{n_redrawn} of {n_pairs} pairs fell inside the decision band: the bound is too wide"
    return gt, sub, planted, redraws


def case_digest(gt, sub):
    h = hashlib.sha256()
    h.update(json.dumps([list(gt.items()), list(sub.items())], sort_keys=True).encode())
    return h.hexdigest()


def recorded(result):
    """the discrete part of a result dictionary, JSON-friendly"""
    return {"e2e_method": result["e2e_method"], "det_only_method": result["det_only_method"],
            "per_sample": {k: {"precision": s["precision"], "recall": s["recall"], "hmean": s["hmean"], "gtDontCare": s["gtDontCare"],
                               "detDontCare": s["detDontCare"], "decisions": [list(x) for x in s["decisions"]]}
                           for k, s in result["per_sample"].items()}}


def load_decisions_golden():
    with open(GOLDEN_DECISIONS) as f:
        return json.load(f)


def write_decisions_golden():
    gt, sub, planted, redraws = decisions_case()
    geometry = decisions_case.geometry
    out = {"digest": case_digest(gt, sub), "redraws": redraws, "planted": planted}
    for ws in (False, True):
        out["word_spotting" if ws else "e2e"] = recorded(check_score(gt, sub, ws, geometry))
    with open(GOLDEN_DECISIONS, "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print(f"wrote {GOLDEN_DECISIONS}: {len(gt)} images, redraws {redraws}, {out['e2e']['e2e_method']}")


if __name__ == "__main__":
    for p in (ROOT, os.path.join(ROOT, "glass-text-spotting_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    write_decisions_golden()
