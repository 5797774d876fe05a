"""Cases and an independent checker for the page order and the blocks (include/glass_hip_feature_layout.h).

The checker is plain Python: per-pair loops with `math`, `math.fsum` for the frame, sets of predecessors, a `while` loop for the
emission.  It shares no code with glass_amd.postprocess.line_order.order_lines_host.  Rule 2 asks, per pair, for a line between
the two in height that overlaps both; every line keeps the lines it overlaps sorted by mv, so that question is one bisection
and a set test, not a loop over all lines.  For every case the checker also measures three margins: the smallest distance
(pixels) of any `over` or block comparison to its threshold, the smallest non-zero |mv_a - mv_b| and |mu_a - mu_b|, and the
frame's distance from its fallback (asserted, as in line_group_cases.py).  A case is used only if the first two are >= MARGIN:
float64 evaluations of the same formulas differ by a few ulps (1e-13 px at these sizes), so with such margins every
implementation decides every comparison alike.
"""
import math
from bisect import bisect_left, bisect_right

import numpy as np

DEFAULTS = {"min_overlap": 0.1, "block_max_gap": 0.8, "block_min_height_ratio": 0.7}
MARGIN = 1e-9
TALLY = {"tried": 0, "rejected": 0}


# ------------------------------------------------------------------------------------------------ the checker
def is_valid(row):
    return all(math.isfinite(v) for v in row) and row[2] > 0 and row[3] > 0


def _dirs(row):
    t = math.radians(row[4])
    return (math.cos(t), -math.sin(t)), (math.sin(t), math.cos(t))


def reference(boxes, prm=DEFAULTS):
    """line boxes [L, 5] float32 -> the expected outputs (unpadded; "block_boxes" as float64 rows, an invalid line's as its
    float32 values), "valid", "edges" (the number of precedence edges) and the margins"""
    rows = [[float(v) for v in r] for r in np.asarray(boxes, dtype=np.float32).reshape(-1, 5)]
    L = len(rows)
    valid = [is_valid(r) for r in rows]
    good = [k for k in range(L) if valid[k]]
    Dx = math.fsum(rows[k][2] * _dirs(rows[k])[0][0] for k in good)
    Dy = math.fsum(rows[k][2] * _dirs(rows[k])[0][1] for k in good)
    Sw = math.fsum(rows[k][2] for k in good)
    nrm = math.hypot(Dx, Dy)
    assert not good or nrm > 1e-11 * Sw or nrm < 1e-13 * Sw, "a frame within a factor of 10 of its fallback threshold"
    PU = (Dx / nrm, Dy / nrm) if nrm > 1e-12 * Sw else (1.0, 0.0)
    PV = (-PU[1], PU[0])
    ulo, uhi, vlo, vhi, mu, mv = ({} for _ in range(6))
    for k in good:
        cx, cy, w, h, _ = rows[k]
        u, v = _dirs(rows[k])
        pu, pv = [], []
        for su in (0.5, -0.5):
            for sv in (0.5, -0.5):
                px, py = cx + su * w * u[0] + sv * h * v[0], cy + su * w * u[1] + sv * h * v[1]
                pu.append(px * PU[0] + py * PU[1]); pv.append(px * PV[0] + py * PV[1])
        ulo[k], uhi[k], vlo[k], vhi[k] = min(pu), max(pu), min(pv), max(pv)
        mu[k], mv[k] = cx * PU[0] + cy * PU[1], cx * PV[0] + cy * PV[1]
    cmp_margin = math.inf
    key_margin = math.inf
    for vals in (mv, mu):
        s = sorted(vals.values())
        key_margin = min([key_margin] + [b - a for a, b in zip(s[:-1], s[1:]) if b != a])

    def over(a, b):
        lhs = min(uhi[a], uhi[b]) - max(ulo[a], ulo[b])
        rhs = prm["min_overlap"] * min(uhi[a] - ulo[a], uhi[b] - ulo[b])
        return lhs > rhs, abs(lhs - rhs)

    ovl = {k: [] for k in good}
    for x, a in enumerate(good):
        for b in good[x + 1:]:
            ok, m = over(a, b)
            cmp_margin = min(cmp_margin, m)
            if ok:
                ovl[a].append(b); ovl[b].append(a)
    ovl_set = {k: set(v) for k, v in ovl.items()}
    ovl_ids = {k: sorted(v, key=lambda c: mv[c]) for k, v in ovl.items()}          # the lines over k, sorted by mv
    ovl_mv = {k: [mv[c] for c in v] for k, v in ovl_ids.items()}

    def separated(a, b):
        """is there a c over both a and b with mv strictly between theirs"""
        if len(ovl_ids[a]) > len(ovl_ids[b]):
            a, b = b, a
        lo, hi = min(mv[a], mv[b]), max(mv[a], mv[b])
        i, j = bisect_right(ovl_mv[a], lo), bisect_left(ovl_mv[a], hi)
        return i < j and not ovl_set[b].isdisjoint(ovl_ids[a][i:j])

    pred = {k: set() for k in good}
    succ = {k: [] for k in good}
    edges = 0
    for x, a in enumerate(good):
        for b in good[x + 1:]:
            first = None
            if b in ovl_set[a]:
                if mv[a] != mv[b]:
                    first = a if mv[a] < mv[b] else b
            elif mu[a] != mu[b] and not separated(a, b):
                first = a if mu[a] < mu[b] else b
            if first is not None:
                second = b if first == a else a
                pred[second].add(first); succ[first].append(second)
                edges += 1

    by_key = sorted(good, key=lambda k: (mv[k], mu[k], k))
    left = list(by_key)
    order, forced = [], 0
    while left:
        e = next((k for k in left if not pred[k]), None)
        if e is None:
            e = left[0]
            forced += 1
        left.remove(e)
        for b in succ[e]:
            pred[b].discard(e)
        order.append(e)

    blocks = []
    for q in order:
        same = False
        if blocks:
            p = blocks[-1][-1]
            H, hmin = max(rows[p][3], rows[q][3]), min(rows[p][3], rows[q][3])
            gap, ratio = (vlo[q] - vhi[p], prm["block_max_gap"] * H), (hmin, prm["block_min_height_ratio"] * H)
            cmp_margin = min(cmp_margin, abs(gap[0] - gap[1]), abs(ratio[0] - ratio[1]))
            same = q in ovl_set[p] and mv[p] < mv[q] and gap[0] <= gap[1] and ratio[0] >= ratio[1]
        if same:
            blocks[-1].append(q)
        else:
            blocks.append([q])
    block_boxes = []
    for members in blocks:
        umin, umax = min(ulo[k] for k in members), max(uhi[k] for k in members)
        vmin, vmax = min(vlo[k] for k in members), max(vhi[k] for k in members)
        cu, cv = (umin + umax) / 2, (vmin + vmax) / 2
        block_boxes.append([cu * PU[0] + cv * PV[0], cu * PU[1] + cv * PV[1], umax - umin, vmax - vmin,
                            math.degrees(math.atan2(-PU[1], PU[0]))])
    for k in range(L):
        if not valid[k]:
            blocks.append([k]); block_boxes.append(rows[k]); order.append(k)
    out = {"page_rank": [0] * L, "page_order": order, "block_id": [0] * L, "block_start": [], "block_boxes": block_boxes,
           "block_count": len(blocks), "forced": forced, "valid": valid, "edges": edges, "cmp_margin": cmp_margin,
           "key_margin": key_margin}
    at = 0
    for bid, members in enumerate(blocks):
        out["block_start"].append(at)
        for k in members:
            out["page_rank"][k], out["block_id"][k] = at, bid
            at += 1
    out["block_start"].append(L)
    return out


def line_first(ref, line_start, K):
    """words in the lines ahead of each line in the order; a line_start entry outside [0, K] or a decreasing pair: size 0"""
    first, ahead = [0] * len(ref["page_order"]), 0
    for k in ref["page_order"]:
        first[k] = ahead
        a, b = int(line_start[k]), int(line_start[k + 1])
        if 0 <= a <= K and 0 <= b <= K and a <= b:
            ahead += b - a
    return first


# ------------------------------------------------------------------------------------------------ scenes
def _f32(rows):
    return np.asarray(rows, dtype=np.float32).reshape(-1, 5)


def _wrap(x):
    return (x + 180.0) % 360.0 - 180.0


def rotate_scene(rows, angle, origin=(0.0, 0.0)):
    """the page turned by `angle` degrees in the sense of the line angle: u = (1, 0) becomes (cos, -sin)"""
    t = math.radians(angle)
    c, s = math.cos(t), math.sin(t)
    return [[origin[0] + (cx - origin[0]) * c + (cy - origin[1]) * s, origin[1] - (cx - origin[0]) * s + (cy - origin[1]) * c, w, h,
             _wrap(a + angle)] for cx, cy, w, h, a in rows]


def shuffled(rows, rng):
    """(float32 boxes with shuffled indices, the indices in the order of construction)"""
    perm = rng.permutation(len(rows))                                  # new index k holds the row perm[k]
    where = np.empty((len(rows),), dtype=np.int64)
    where[perm] = np.arange(len(rows))
    return _f32([rows[k] for k in perm]), [int(k) for k in where]


def page(seed, n, columns=2, angle=0.0, bands=1, header=True):
    """n lines: a header over `columns` columns of paragraphs whose gaps sit at the same height in every column, ragged last
    lines, and with bands > 1 a full-width line between two such bands.  Built in reading order: header, then band by band the
    columns left to right, each top to bottom."""
    rng = np.random.RandomState(seed)
    col_w, gutter, pitch, para_gap, h = 300.0, 40.0, 28.0, 30.0, 20.0
    width = columns * col_w + (columns - 1) * gutter
    rows, y = [], 30.0

    def wide_line():
        nonlocal y
        rows.append([width / 2 + rng.uniform(-1, 1), y + rng.uniform(-0.4, 0.4), width - rng.uniform(0, 8), h + 4.0, rng.uniform(-0.5, 0.5)])
        y += pitch + para_gap

    if header and n > 0:
        wide_line()
    body = n - len(rows) - (bands - 1)
    for band in range(bands):
        if band:
            wide_line()
        share = body // bands + (1 if band < body % bands else 0)
        depth = -(-share // columns)                                   # lines per column, the last column may be shorter
        breaks = set(rng.choice(np.arange(2, max(depth, 3)), size=min(2, max(depth - 2, 0)), replace=False).tolist()) if depth > 3 else set()
        y_of, yy = [], y
        for r in range(depth):                                         # the same heights, and the same gaps, in every column
            if r in breaks:
                yy += para_gap
            y_of.append(yy)
            yy += pitch
        for c in range(columns):
            x0 = c * (col_w + gutter)
            for r in range(min(depth, share - c * depth)):
                last = r + 1 in breaks or r + 1 == depth               # a paragraph's last line is ragged
                w = col_w * rng.uniform(0.35, 0.8) if last else col_w - rng.uniform(0, 6)
                rows.append([x0 + w / 2 + rng.uniform(0, 2), y_of[r] + rng.uniform(-0.4, 0.4), w, h * rng.uniform(0.95, 1.05),
                             rng.uniform(-0.5, 0.5)])
        y = yy + para_gap
    assert len(rows) == n, (len(rows), n)
    rows = rotate_scene(rows, angle, (width / 2, y / 2))
    return shuffled(rows, rng)


def one_row(seed, n):
    """n lines side by side in one row, none over another"""
    rng = np.random.RandomState(seed)
    rows = [[30.0 * k + rng.uniform(-2, 2), 500.0 + rng.uniform(-3, 3), rng.uniform(16, 22), rng.uniform(18, 22), rng.uniform(-1, 1)]
            for k in range(n)]
    return shuffled(rows, rng)


def random_boxes(seed, n):
    """n overlapping boxes thrown on a page: the rules contradict each other, and the order has forced emissions"""
    rng = np.random.RandomState(seed)
    rows = [[rng.uniform(0, 700), rng.uniform(0, 700), rng.uniform(30, 300), rng.uniform(15, 30), rng.uniform(-3, 3)] for _ in range(n)]
    return _f32(rows), None


def identical(n):
    return _f32([[100.0, 100.0, 40.0, 20.0, 5.0]] * n), None


def four_line_cycle():
    return _f32([[200, 241, 301, 20, 0], [100, 242, 300.5, 20, 0], [450, 80, 240, 20, 0], [350, 83, 61.5, 20, 0]]), None


def with_invalid(seed, n):
    """a page with lines that are no lines between the others: NaN, inf, zero and negative extents"""
    boxes, built = page(seed, n)
    boxes = boxes.copy()
    nan, inf = float("nan"), float("inf")
    bad = {}
    for k, (col, val) in zip(range(1, n, max(1, n // 9)), ((0, nan), (2, inf), (2, 0.0), (3, -3.0), (4, nan), (1, -inf), (3, 0.0),
                                                          (4, inf), (2, -1.0))):
        boxes[k, col] = val
        bad[k] = True
    return boxes, [k for k in built if k not in bad] + sorted(bad)


def usable(ref):
    return ref["cmp_margin"] >= MARGIN and ref["key_margin"] >= MARGIN


def generated(make, seed, *args):
    """the first scene of make(seed, ...), make(seed + 1, ...), ... whose margins allow it, with its order of construction (or
    None) and its reference"""
    for s in range(seed, seed + 8):
        boxes, built = make(s, *args)
        ref = reference(boxes)
        TALLY["tried"] += 1
        if usable(ref):
            return boxes, built, ref
        TALLY["rejected"] += 1
    raise AssertionError(f"no usable scene among 8 seeds from {seed}")


def _hand_made(scene):
    boxes, built = scene
    ref = reference(boxes)
    assert usable(ref), (ref["cmp_margin"], ref["key_margin"])
    return boxes, built, ref


K_LIST = (0, 1, 2, 63, 64, 65, 129, 1023, 1024)

_BUILDERS = {f"page of {n}": (lambda n=n: generated(page, 100 + n, n))
             for n in sorted({n for K in K_LIST for n in (K, K // 2)} - {0})}
_BUILDERS.update({
    "no lines": lambda: _hand_made((np.zeros((0, 5), dtype=np.float32), [])),
    "2 columns": lambda: generated(page, 5, 150, 2),
    "3 columns": lambda: generated(page, 6, 181, 3),
    "4 columns": lambda: generated(page, 7, 203, 4),
    "3 columns at 30 degrees": lambda: generated(page, 8, 160, 3, 30.0),
    "2 columns at -170 degrees": lambda: generated(page, 9, 140, 2, -170.0),
    "4 columns at 30 degrees": lambda: generated(page, 10, 170, 4, 30.0),
    "2 columns at 30 degrees": lambda: generated(page, 18, 133, 2, 30.0),
    "3 columns at -170 degrees": lambda: generated(page, 19, 175, 3, -170.0),
    "4 columns at -170 degrees": lambda: generated(page, 20, 190, 4, -170.0),
    "a full-width line between two bands": lambda: generated(page, 11, 121, 2, 0.0, 2),
    "two bands of 3 columns at -170 degrees": lambda: generated(page, 12, 150, 3, -170.0, 2),
    "one column of 1024": lambda: generated(page, 13, 1024, 1, 0.0, 1, False),
    "one row of 1024": lambda: generated(one_row, 14, 1024),
    "identical boxes": lambda: _hand_made(identical(70)),
    "random overlapping boxes": lambda: generated(random_boxes, 15, 200),
    "random overlapping boxes, 65": lambda: generated(random_boxes, 16, 65),
    "four-line cycle": lambda: _hand_made(four_line_cycle()),
    "lines that are no lines": lambda: generated(with_invalid, 17, 60),
})
PAGES = tuple(n for n in _BUILDERS if "column" in n or "bands" in n or n.startswith("page of") or n in ("one row of 1024",
                                                                                                        "lines that are no lines"))
_BUILT = {}


def case(name):
    """(name, boxes float32 [L, 5], the order of construction or None, reference), built on first use and then shared unchanged"""
    if name not in _BUILT:
        _BUILT[name] = (name, *_BUILDERS[name]())
    return _BUILT[name]


def all_cases():
    """every case; prints and checks the tally of the seeds that the margins rejected"""
    cases = [case(name) for name in _BUILDERS]
    print(f"[line_order] seeds tried {TALLY['tried']}, rejected {TALLY['rejected']}")
    assert 8 * TALLY["rejected"] <= TALLY["tried"], TALLY
    return cases


INT_FIELDS = ("page_rank", "page_order", "block_id", "block_start")


def expected_padded(ref, K):
    """the reference's integer outputs padded to K as the kernel pads them"""
    L, B = len(ref["page_rank"]), ref["block_count"]
    return {"page_rank": ref["page_rank"] + [-1] * (K - L), "page_order": ref["page_order"] + [-1] * (K - L),
            "block_id": ref["block_id"] + [-1] * (K - L), "block_start": ref["block_start"] + [L] * (K - B),
            "block_count": B, "forced": ref["forced"]}


def box_ulps(got_row, want_row):
    """distance in float32 units in the last place between a float32 row and a float64 row rounded to float32 (0 for equal
    bits, NaN included)"""
    g = np.asarray(got_row, dtype=np.float32)
    w = np.asarray(want_row, dtype=np.float64).astype(np.float32)
    same = g.view(np.uint32) == w.view(np.uint32)
    gi, wi = g.view(np.int32).astype(np.int64), w.view(np.int32).astype(np.int64)
    gi, wi = np.where(gi < 0, -(gi & 0x7fffffff), gi), np.where(wi < 0, -(wi & 0x7fffffff), wi)
    return int(np.where(same, 0, np.abs(gi - wi)).max())
