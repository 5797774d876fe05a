"""Cases and an independent checker for the rows, cells, tables and columns (include/glass_hip_feature_grid.h).

The checker is plain Python: per-pair loops with `math`, `math.fsum` for the frame, components by repeated set union, numbers by
`sorted`.  It uses no bit words and shares no code with glass_amd.postprocess.row_grid.row_grid_host.  For every case it also
measures two margins: the smallest distance (pixels) of any comparison it makes to its threshold, and the smallest non-zero
difference between two keys (mv, mu, ulo).  A case is used only if both are >= MARGIN: float64 evaluations of the same formulas
differ by a few ulps (1e-13 px at these sizes), so with such margins every implementation decides every comparison alike.
(A pair is decided in the order beside, then the heights shared, then the like heights - or, not beside, over, then the gap - and
a comparison behind one that already failed is not made: it cannot change the result.)
"""
import math

import numpy as np

from line_order_cases import box_ulps, rotate_scene, shuffled  # noqa: F401  (scene helpers; no part of either checker)

DEFAULTS = {"row_min_overlap": 0.5, "row_min_height_ratio": 0.5, "column_min_overlap": 0.1, "table_max_row_gap": 2.0}
MARGIN = 1e-9
TALLY = {"tried": 0, "rejected": 0}
INT_FIELDS = ("row_id", "row_pos", "table_id", "col_id", "row_order", "row_start", "table_rows", "table_cols")


# ------------------------------------------------------------------------------------------------ the checker
def is_valid(row):
    return all(math.isfinite(v) for v in row) and row[2] > 0 and row[3] > 0


def _dirs(row):
    t = math.radians(row[4])
    return (math.cos(t), -math.sin(t)), (math.sin(t), math.cos(t))


def _components(nodes, edges):
    """{node: the frozen set of its component}, by repeated set union"""
    comp = {k: {k} for k in nodes}
    for a, b in edges:
        A, B = comp[a], comp[b]
        if A is not B:
            if len(A) < len(B):
                A, B = B, A
            A |= B
            for k in B:
                comp[k] = A
    return comp


def reference(boxes, prm=DEFAULTS):
    """line boxes [L, 5] float32 -> the expected outputs (unpadded lists; the boxes as float64 rows, an invalid line's as its
    float32 values), "valid" and the margins"""
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
    ulo, uhi, vlo, vhi, mu, mv, hh = ([0.0] * L for _ in range(7))
    for k in good:
        cx, cy, w, h, _ = rows[k]
        u, v = _dirs(rows[k])
        pu, pv = [], []
        for su in (0.5, -0.5):
            for sv in (0.5, -0.5):
                px, py = cx + su * w * u[0] + sv * h * v[0], cy + su * w * u[1] + sv * h * v[1]
                pu.append(px * PU[0] + py * PU[1]); pv.append(px * PV[0] + py * PV[1])
        ulo[k], uhi[k], vlo[k], vhi[k], hh[k] = min(pu), max(pu), min(pv), max(pv), h
        mu[k], mv[k] = cx * PU[0] + cy * PU[1], cx * PV[0] + cy * PV[1]
    key_margin = math.inf
    for vals in (mv, mu, ulo):
        s = sorted(vals[k] for k in good)
        key_margin = min([key_margin] + [b - a for a, b in zip(s[:-1], s[1:]) if b != a])

    # ---- the pairs: row-mates, and the pairs that are over each other and near (column-mates once the rows are known)
    cmp_margin = math.inf
    rowmates, near = [], []
    r_ov, r_hr, c_ov, t_gap = (prm[k] for k in ("row_min_overlap", "row_min_height_ratio", "column_min_overlap", "table_max_row_gap"))
    for x, a in enumerate(good):
        ulo_a, uhi_a, vlo_a, vhi_a, h_a = ulo[a], uhi[a], vlo[a], vhi[a], hh[a]
        for b in good[x + 1:]:
            ovl = min(uhi_a, uhi[b]) - max(ulo_a, ulo[b])
            m = abs(ovl)
            if ovl <= 0:                                               # beside
                shared = min(vhi_a, vhi[b]) - max(vlo_a, vlo[b])
                need = r_ov * min(vhi_a - vlo_a, vhi[b] - vlo[b])
                m = min(m, abs(shared - need))
                if shared >= need:
                    lo, hi = min(h_a, hh[b]), r_hr * max(h_a, hh[b])
                    m = min(m, abs(lo - hi))
                    if lo >= hi:
                        rowmates.append((a, b))
            else:
                need = c_ov * min(uhi_a - ulo_a, uhi[b] - ulo[b])
                m = min(m, abs(ovl - need))
                if ovl > need:
                    gap, most = max(vlo_a, vlo[b]) - min(vhi_a, vhi[b]), t_gap * max(h_a, hh[b])
                    m = min(m, abs(gap - most))
                    if gap <= most:
                        near.append((a, b))
            if m < cmp_margin:
                cmp_margin = m

    row_of = _components(good, rowmates)
    multi = [k for k in good if len(row_of[k]) >= 2]
    colmates = [(a, b) for a, b in near if len(row_of[a]) >= 2 and len(row_of[b]) >= 2 and row_of[a] is not row_of[b]]
    col_of = _components(multi, colmates)
    table_of = _components(multi, [(a, b) for a, b in rowmates] + colmates)

    def distinct(comp, nodes):
        seen, out = set(), []
        for k in nodes:
            if id(comp[k]) not in seen:
                seen.add(id(comp[k])); out.append(comp[k])
        return out

    def enclose(members):
        umin, umax = min(ulo[k] for k in members), max(uhi[k] for k in members)
        vmin, vmax = min(vlo[k] for k in members), max(vhi[k] for k in members)
        cu, cv = (umin + umax) / 2, (vmin + vmax) / 2
        return [cu * PU[0] + cv * PV[0], cu * PU[1] + cv * PV[1], umax - umin, vmax - vmin, math.degrees(math.atan2(-PU[1], PU[0]))]

    the_rows = sorted(distinct(row_of, good), key=lambda s: (min(mv[k] for k in s), min(s)))
    the_rows = [sorted(s, key=lambda k: (mu[k], k)) for s in the_rows]
    row_boxes = [enclose(s) for s in the_rows]
    for k in range(L):
        if not valid[k]:
            the_rows.append([k]); row_boxes.append(rows[k])
    out = {"row_id": [0] * L, "row_pos": [0] * L, "table_id": [-1] * L, "col_id": [-1] * L, "row_order": [], "row_start": [],
           "row_boxes": row_boxes, "row_count": len(the_rows), "valid": valid, "cmp_margin": cmp_margin, "key_margin": key_margin,
           "multi_rows": sum(len(s) >= 2 for s in the_rows)}
    for r, cells in enumerate(the_rows):
        out["row_start"].append(len(out["row_order"]))
        for q, k in enumerate(cells):
            out["row_id"][k], out["row_pos"][k] = r, q
            out["row_order"].append(k)
    out["row_start"].append(L)
    tables = sorted(distinct(table_of, multi), key=lambda s: min(out["row_id"][k] for k in s))
    out["table_count"] = len(tables)
    out["table_boxes"] = [enclose(s) for s in tables]
    out["table_rows"] = [len({out["row_id"][k] for k in s}) for s in tables]
    out["table_cols"] = []
    for tb, s in enumerate(tables):
        cols = sorted(distinct(col_of, sorted(s)), key=lambda c: (min(ulo[k] for k in c), min(c)))
        out["table_cols"].append(len(cols))
        for q, c in enumerate(cols):
            for k in c:
                out["table_id"][k], out["col_id"][k] = tb, q
    return out


def row_first(ref, line_start, K):
    """words in the lines ahead of each line in row_order; a line_start entry outside [0, K] or a decreasing pair: size 0"""
    first, ahead = [0] * len(ref["row_order"]), 0
    for k in ref["row_order"]:
        first[k] = ahead
        a, b = int(line_start[k]), int(line_start[k + 1])
        if 0 <= a <= K and 0 <= b <= K and a <= b:
            ahead += b - a
    return first


def expected_padded(ref, K):
    """the reference's integer outputs padded to K as the kernel pads them"""
    L, R, T = len(ref["row_id"]), ref["row_count"], ref["table_count"]
    out = {k: ref[k] + [-1] * (K - L) for k in ("row_id", "row_pos", "table_id", "col_id", "row_order")}
    out.update({"row_start": ref["row_start"] + [L] * (K - R), "table_rows": ref["table_rows"] + [0] * (K - T),
                "table_cols": ref["table_cols"] + [0] * (K - T), "row_count": R, "table_count": T})
    return out


# ------------------------------------------------------------------------------------------------ scenes
# Every scene sits on a coarse grid (a pitch of 28 px, heights of 20 px, gutters of tens of pixels) with a jitter of a fraction
# of a pixel, so every comparison is pixels from its threshold.  Each returns (float32 boxes with shuffled indices, the texts of
# the lines by index or None).
def _f32(rows):
    return np.asarray(rows, dtype=np.float32).reshape(-1, 5)


def _finish(rows, texts, rng, angle=0.0):
    xs, ys = [r[0] for r in rows] or [0.0], [r[1] for r in rows] or [0.0]
    rows = rotate_scene(rows, angle, ((min(xs) + max(xs)) / 2, (min(ys) + max(ys)) / 2))
    boxes, where = shuffled(rows, rng)                                  # line where[k] is the k-th of the construction
    named = [None] * len(rows)
    for k, w in enumerate(where):
        named[w] = texts[k]
    return boxes, named


def _line(rng, x0, y, w, h=20.0, jitter=True):
    """a line whose left end is at x0"""
    j = (lambda s: rng.uniform(-s, s)) if jitter else (lambda s: 0.0)
    return [x0 + w / 2 + j(0.5), y + j(0.4), w, h * (1.0 + j(0.03)), j(0.4)]


def _right(rng, x1, y, w, h=20.0):
    """a line whose right end is at x1"""
    return _line(rng, x1 - w, y, w, h)


def receipt(seed, angle=0.0):
    """two header lines, three item / price pairs with a continuation line under the second, TOTAL / amount, a footer"""
    rng = np.random.RandomState(seed)
    rows, texts = [], []

    def add(row, text):
        rows.append(row); texts.append(text)
    add(_line(rng, 90.0, 40.0, 220.0, 26.0), "ACME STORE")
    add(_line(rng, 110.0, 72.0, 180.0, 18.0), "12 Main Street")
    y = 130.0
    for name, w, price, pw, more in (("Coffee", 70.0, "3.50", 44.0, None), ("Sandwich deluxe", 170.0, "12.00", 52.0, "with cheese"),
                                     ("Tea", 36.0, "2.00", 44.0, None)):
        add(_line(rng, 40.0, y, w), name)
        add(_right(rng, 360.0, y, pw), price)
        y += 28.0
        if more:
            add(_line(rng, 60.0, y, 110.0), more)
            y += 28.0
    y += 60.0
    add(_line(rng, 40.0, y, 70.0, 22.0), "TOTAL")
    add(_right(rng, 360.0, y, 56.0, 22.0), "17.50")
    add(_line(rng, 130.0, y + 50.0, 140.0), "Thank you")
    return _finish(rows, texts, rng, angle)


def table(seed, R, C, title=True, footnote=True, below=None, angle=0.0):
    """an R x C table (left-aligned cells, columns 160 px apart) under a spanning title, a prose footnote under it and, with
    below = (rows, columns, distance), a second table that far (pixels, box to box) under the footnote's place"""
    rng = np.random.RandomState(seed)
    rows, texts, y = [], [], 40.0
    if title:
        rows.append(_line(rng, 0.0, y, 160.0 * C - 20.0, 24.0)); texts.append("title")
        y += 44.0
    for r in range(R):
        for c in range(C):
            rows.append(_line(rng, 160.0 * c, y, rng.uniform(60.0, 130.0))); texts.append(f"r{r}c{c}")
        y += 28.0
    if footnote:
        y += 16.0
        rows.append(_line(rng, 0.0, y, 160.0 * C - 50.0)); texts.append("footnote")
        y += 28.0
    if below:
        R2, C2, distance = below
        y += distance - 8.0                                            # (the pitch of 28 leaves 8 px between two boxes)
        for r in range(R2):
            for c in range(C2):
                rows.append(_line(rng, 160.0 * c, y, rng.uniform(60.0, 130.0))); texts.append(f"s{r}c{c}")
            y += 28.0
    return _finish(rows, texts, rng, angle)


def prose_columns(seed, n_rows):
    """two columns of prose whose lines stand at equal heights: rows by rule"""
    rng = np.random.RandomState(seed)
    rows, texts = [], []
    for r in range(n_rows):
        for c in range(2):
            rows.append(_line(rng, 340.0 * c, 40.0 + 28.0 * r, 300.0 - rng.uniform(0, 6))); texts.append(f"c{c}l{r}")
    return _finish(rows, texts, rng)


def staircase(seed, n):
    """n lines side by side, each 8 px lower than the one before: every line shares 12 of its 20 px with its neighbours and 4
    with the next but one, so it is a row-mate of its neighbours only - one row of diameter n - 1"""
    rng = np.random.RandomState(seed)
    rows = [[30.0 * k + rng.uniform(-2, 2), 100.0 + 8.0 * k + rng.uniform(-0.3, 0.3), rng.uniform(16, 22), 20.0, rng.uniform(-0.2, 0.2)]
            for k in range(n)]
    return _finish(rows, [f"s{k}" for k in range(n)], rng)


def diagonal(seed, n):
    """n // 2 rows of two cells (and a line of its own if n is odd); every row stands 30 px to the right of the one above and
    its cells are 50 px wide, so a cell is over the next row's cell only - two columns of diameter n // 2 - 1, one table"""
    rng = np.random.RandomState(seed)
    rows, texts = [], []
    for r in range(n // 2):
        for c in range(2):
            rows.append([25.0 + 30.0 * r + 40000.0 * c + rng.uniform(-1, 1), 100.0 + 28.0 * r + rng.uniform(-0.3, 0.3),
                         50.0 + rng.uniform(-1, 1), 20.0, rng.uniform(-0.01, 0.01)])
            texts.append(f"r{r}c{c}")
    if n % 2:
        rows.append([20000.0, 20.0, 300.0, 20.0, 0.0]); texts.append("alone")
    return _finish(rows, texts, rng)


def singletons(seed, n):
    """n lines one under the other: n rows of one line, no table"""
    rng = np.random.RandomState(seed)
    rows = [_line(rng, rng.uniform(0, 30), 40.0 + 28.0 * k, rng.uniform(100, 300)) for k in range(n)]
    return _finish(rows, [f"l{k}" for k in range(n)], rng)


def identical(n):
    return _f32([[100.0, 100.0, 40.0, 20.0, 5.0]] * n), [f"i{k}" for k in range(n)]


def shared_column():
    """row 0: A and B close together and D far right; row 1: C under both A and B, E under D.  A, B and C are one column: two
    lines of one row in one column"""
    rows = [[20.0, 100.0, 40.0, 20.0, 0.0], [80.0, 100.5, 40.0, 20.0, 0.0], [450.0, 99.5, 100.0, 20.0, 0.0],
            [50.5, 128.0, 100.0, 20.0, 0.0], [451.0, 128.5, 100.0, 20.0, 0.0]]
    return _f32(rows), ["A", "B", "D", "C", "E"]


def grid_page(seed, n):
    """n lines of a receipt-like page: item / amount pairs, now and then a continuation line or a heading of its own, and a
    wider gap between groups"""
    rng = np.random.RandomState(seed)
    rows, texts, y, k = [], [], 40.0, 0
    while len(rows) < n:
        kind = k % 7
        if kind in (3, 6) or len(rows) + 1 == n:
            rows.append(_line(rng, 60.0 if kind == 3 else 0.0, y, rng.uniform(100, 200))); texts.append(f"line {k}")
        else:
            rows.append(_line(rng, 40.0, y, rng.uniform(40, 180))); texts.append(f"item {k}")
            rows.append(_right(rng, 420.0, y, rng.uniform(40, 60))); texts.append(f"amount {k}")
        y += 28.0 + (70.0 if kind == 6 else 0.0)
        k += 1
    return _finish(rows, texts, rng)


def with_invalid(seed, n):
    """a page with lines that are no lines between the others: NaN, inf, zero and negative extents"""
    boxes, texts = grid_page(seed, n)
    boxes = boxes.copy()
    nan, inf = float("nan"), float("inf")
    for k, (col, val) in zip(range(1, n, max(1, n // 9)), ((0, nan), (2, inf), (2, 0.0), (3, -3.0), (4, nan), (1, -inf), (3, 0.0),
                                                          (4, inf), (2, -1.0))):
        boxes[k, col] = val
    return boxes, texts


def usable(ref):
    return ref["cmp_margin"] >= MARGIN and ref["key_margin"] >= MARGIN


def generated(make, seed, *args):
    """the first scene of make(seed, ...), make(seed + 1, ...), ... whose margins allow it, with its texts and its reference"""
    for s in range(seed, seed + 8):
        boxes, texts = make(s, *args)
        ref = reference(boxes)
        TALLY["tried"] += 1
        if usable(ref):
            return boxes, texts, ref
        TALLY["rejected"] += 1
    raise AssertionError(f"no usable scene among 8 seeds from {seed}")


def _hand_made(scene):
    boxes, texts = scene
    ref = reference(boxes)
    assert usable(ref), (ref["cmp_margin"], ref["key_margin"])
    return boxes, texts, ref


K_LIST = (0, 1, 2, 63, 64, 65, 129, 1023, 1024)

_BUILDERS = {f"page of {n}": (lambda n=n: generated(grid_page, 100 + n, n))
             for n in sorted({n for K in K_LIST for n in (K, K // 2)} - {0})}
_BUILDERS.update({
    "no lines": lambda: _hand_made((np.zeros((0, 5), dtype=np.float32), [])),
    "receipt": lambda: generated(receipt, 5),
    "receipt at 30 degrees": lambda: generated(receipt, 6, 30.0),
    "receipt at -170 degrees": lambda: generated(receipt, 7, -170.0),
    "4 x 3 table and a 2 x 2 table far below": lambda: generated(table, 8, 4, 3, True, True, (2, 2, 120.0)),
    "7 x 5 table at 30 degrees": lambda: generated(table, 9, 7, 5, True, True, None, 30.0),
    "two tables, close": lambda: generated(table, 10, 3, 2, False, False, (2, 2, 30.0)),
    "two tables, far": lambda: generated(table, 11, 3, 2, False, False, (2, 2, 55.0)),
    "two prose columns": lambda: generated(prose_columns, 12, 4),
    "staircase of 65": lambda: generated(staircase, 13, 65),
    "staircase of 1024": lambda: generated(staircase, 14, 1024),
    "diagonal of 129": lambda: generated(diagonal, 15, 129),
    "diagonal of 1024": lambda: generated(diagonal, 16, 1024),
    "singletons, 1023": lambda: generated(singletons, 17, 1023),
    "identical boxes": lambda: _hand_made(identical(70)),
    "two lines of one row in one column": lambda: _hand_made(shared_column()),
    "lines that are no lines": lambda: generated(with_invalid, 18, 60),
})
_BUILT = {}


def case(name):
    """(name, boxes float32 [L, 5], the lines' texts, reference), built on first use and then shared unchanged"""
    if name not in _BUILT:
        _BUILT[name] = (name, *_BUILDERS[name]())
    return _BUILT[name]


def all_cases():
    """every case; prints and checks the tally of the seeds that the margins rejected"""
    cases = [case(name) for name in _BUILDERS]
    print(f"[row_grid] seeds tried {TALLY['tried']}, rejected {TALLY['rejected']}")
    assert 10 * TALLY["rejected"] <= TALLY["tried"], TALLY
    return cases
