"""Text lines of one image aligned into rows, cells, tables and columns: the readable statement, in numpy float64, of what
csrc/row_grid.hip computes on the device (include/glass_hip_feature_grid.h has the contract in words), and `rows_of` /
`tables_of` / `rows_text`, the host views of the per-word fields the post-processor attaches with POST_PROCESSING.ALIGN_ROWS.

A line is (cx, cy, w, h, a) as the line grouping writes its line boxes.  Everything is widened to float64 first.  Validity,
the page frame P_U, P_V and every line's intervals [ulo, uhi] along the text and [vlo, vhi] down the page are those of the
page order (line_order.py), formula for formula.  Two lines that are disjoint along the text, share enough of their heights
and have like heights are row-mates; the rows are the connected components of that relation, and a row of two or more lines
is multi-cell.  Two lines of different multi-cell rows that overlap along the text and lie close down the page are
column-mates; the columns are the components of that relation and the tables the components of both together.  Every number
is a count of smaller keys: rows by (smallest mv, smallest index), cells by (mu, index), tables by their smallest row,
columns inside a table by (smallest ulo, smallest index).

Known limits: two prose columns whose lines stand at equal heights come out as rows - geometry alone cannot tell them from a
table, so the caller chooses the reading (page_text or rows_text); a cell of several lines is several rows; a spanning cell
inside a multi-cell row joins the columns it covers; lines at angles far from the page's follow the rules, not a human.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional

import numpy as np

from .line_grouping import MAX_WORDS, _frame, _tree_sum

MAX_LINES = MAX_WORDS            # GLASS_ROW_GRID_MAX_K (include/glass_hip_feature_grid.h): lines per image
DEFAULT_PARAMS = {"row_min_overlap": 0.5, "row_min_height_ratio": 0.5, "column_min_overlap": 0.1, "table_max_row_gap": 2.0}
# name -> (lowest, open at the lowest, highest, open at the highest)
_RANGES = {"row_min_overlap": (0.0, True, 1.0, False), "row_min_height_ratio": (0.0, False, 1.0, False),
           "column_min_overlap": (0.0, False, 1.0, True), "table_max_row_gap": (0.0, False, math.inf, False)}


def check_grid_params(row_min_overlap=DEFAULT_PARAMS["row_min_overlap"], row_min_height_ratio=DEFAULT_PARAMS["row_min_height_ratio"],
                      column_min_overlap=DEFAULT_PARAMS["column_min_overlap"],
                      table_max_row_gap=DEFAULT_PARAMS["table_max_row_gap"]) -> Dict[str, float]:
    """the four thresholds as floats; ValueError for one that is no number, not finite or outside its range: row_min_overlap
    in (0, 1], row_min_height_ratio in [0, 1], column_min_overlap in [0, 1), table_max_row_gap >= 0"""
    out = {}
    for name, v in (("row_min_overlap", row_min_overlap), ("row_min_height_ratio", row_min_height_ratio),
                    ("column_min_overlap", column_min_overlap), ("table_max_row_gap", table_max_row_gap)):
        lo, lo_open, hi, hi_open = _RANGES[name]
        try:
            f = float(v)
        except (TypeError, ValueError):
            raise ValueError(f"row_grid: {name}={v!r} is not a number") from None
        if (isinstance(v, bool) or not math.isfinite(f) or f < lo or f > hi or (f == lo and lo_open) or (f == hi and hi_open)):
            raise ValueError(f"row_grid: {name}={v!r}: needs a finite value in {'(' if lo_open else '['}{lo}, {hi}{')' if hi_open else ']'}")
        out[name] = f
    return out


def _components(M: np.ndarray) -> np.ndarray:
    """the smallest index of every node's connected component under the symmetric relation M [n, n]: minimum-label
    propagation over the edge list with pointer jumps until every label is a root, at most n rounds (a path of n nodes needs
    no more without the jumps)"""
    n = len(M)
    lab = np.arange(n)
    a, b = np.nonzero(M)                                             # (symmetric: every edge in both directions)
    for _ in range(n):
        new = lab.copy()
        np.minimum.at(new, a, lab[b])
        while True:
            jump = new[new]
            if np.array_equal(jump, new):
                break
            new = jump
        if np.array_equal(new, lab):
            break
        lab = new
    return lab


def row_grid_host(line_boxes, params: Optional[dict] = None, line_start=None, K: int = MAX_LINES) -> dict:
    """line_boxes [L, 5] float32 (L <= MAX_LINES) -> {"row_id" [L], "row_pos" [L], "table_id" [L], "col_id" [L], "row_order" [L],
    "row_start" [R + 1] (int32), "row_boxes" float32 [R, 5], "row_count" R, "table_boxes" float32 [T, 5], "table_rows" [T],
    "table_cols" [T] (int32), "table_count" T} and, with `line_start` (int [L + 1] or longer, the line grouping's CSR; `K` is
    the padded size the device checks its entries against), "row_first" [L].  `params`: any of DEFAULT_PARAMS' keys."""
    p = check_grid_params(**(params or {}))
    b32 = np.ascontiguousarray(np.asarray(line_boxes, dtype=np.float32).reshape(-1, 5))
    L = len(b32)
    if L > MAX_LINES:
        raise ValueError(f"row_grid: {L} lines (max {MAX_LINES})")
    wide = b32.astype(np.float64)
    valid = np.isfinite(wide).all(axis=1)
    valid &= np.where(valid, (wide[:, 2] > 0) & (wide[:, 3] > 0), False)
    cx, cy, w, h, a = np.where(valid[:, None], wide, 0.0).T
    t = a * np.pi / 180.0
    ux, uy = np.cos(t), -np.sin(t)                                   # u; v = (-uy, ux) = (sin t, cos t)

    # ---- the page frame and the intervals in it: the formulas of the page order
    PU = _frame(_tree_sum(w * ux), _tree_sum(w * uy), _tree_sum(w), (1.0, 0.0))      # (w = 0 for an invalid line)
    PV = (-PU[1], PU[0])
    ax, ay, bx, by = w / 2 * ux, w / 2 * uy, h / 2 * -uy, h / 2 * ux
    pu, pv = [], []
    for su, sv in ((1.0, 1.0), (-1.0, 1.0), (1.0, -1.0), (-1.0, -1.0)):
        px, py = cx + su * ax + sv * bx, cy + su * ay + sv * by
        pu.append(px * PU[0] + py * PU[1])
        pv.append(px * PV[0] + py * PV[1])
    if L:
        ulo, uhi, vlo, vhi = np.min(pu, axis=0), np.max(pu, axis=0), np.min(pv, axis=0), np.max(pv, axis=0)
    else:
        ulo = uhi = vlo = vhi = np.zeros((0,))
    mu, mv = cx * PU[0] + cy * PU[1], cx * PV[0] + cy * PV[1]

    # ---- the relations, [a, b], by line index
    i, j = np.s_[:, None], np.s_[None, :]
    idx = np.arange(L)
    pair = valid[i] & valid[j] & (idx[i] != idx[j])
    ovl = np.minimum(uhi[i], uhi[j]) - np.maximum(ulo[i], ulo[j])
    hmin, hmax = np.minimum(h[i], h[j]), np.maximum(h[i], h[j])
    rowmate = pair & (ovl <= 0)
    rowmate &= (np.minimum(vhi[i], vhi[j]) - np.maximum(vlo[i], vlo[j])
                >= p["row_min_overlap"] * np.minimum(vhi[i] - vlo[i], vhi[j] - vlo[j]))
    rowmate &= hmin >= p["row_min_height_ratio"] * hmax
    row_of = _components(rowmate)                                                  # the row's smallest member
    multi = rowmate.any(axis=1)
    colmate = pair & (ovl > p["column_min_overlap"] * np.minimum(uhi[i] - ulo[i], uhi[j] - ulo[j]))
    colmate &= np.maximum(vlo[i], vlo[j]) - np.minimum(vhi[i], vhi[j]) <= p["table_max_row_gap"] * hmax
    colmate &= multi[i] & multi[j] & (row_of[i] != row_of[j])
    col_of, table_of = _components(colmate), _components(rowmate | colmate)

    # ---- rows: by (smallest mv, smallest index); the invalid lines after them, in index order; cells by (mu, index)
    row_min = np.full((L,), np.inf)
    np.minimum.at(row_min, row_of[valid], mv[valid])
    roots = np.flatnonzero(valid & (row_of == idx))
    roots = roots[np.lexsort((roots, row_min[roots]))]
    number = np.zeros((L,), dtype=np.int64)
    number[roots] = np.arange(len(roots))
    row_id = np.where(valid, number[row_of], len(roots) + np.cumsum(~valid) - 1)
    same = valid[i] & valid[j] & (row_of[i] == row_of[j])
    row_pos = (same & ((mu[j] < mu[i]) | ((mu[j] == mu[i]) & (idx[j] < idx[i])))).sum(axis=1)
    R = len(roots) + int((~valid).sum())
    row_order = np.lexsort((row_pos, row_id))
    row_start = np.concatenate([[0], np.cumsum(np.bincount(row_id, minlength=R))]) if L else np.zeros((1,), dtype=np.int64)
    angle = math.atan2(-PU[1], PU[0]) * 180.0 / math.pi

    def box(members):
        umin, umax, vmin, vmax = ulo[members].min(), uhi[members].max(), vlo[members].min(), vhi[members].max()
        cu, cv = (umin + umax) / 2, (vmin + vmax) / 2
        return np.array([cu * PU[0] + cv * PV[0], cu * PU[1] + cv * PV[1], umax - umin, vmax - vmin, angle]).astype(np.float32)

    row_boxes = np.zeros((R, 5), dtype=np.float32)
    for r in range(R):
        members = row_order[row_start[r]:row_start[r + 1]]
        row_boxes[r] = box(members) if valid[members[0]] else b32[members[0]]

    # ---- tables by their smallest row; columns inside a table by (smallest ulo, smallest index)
    troots = np.flatnonzero(multi & (table_of == idx))
    tmin = np.full((L,), L, dtype=np.int64)
    np.minimum.at(tmin, table_of[multi], row_id[multi])
    troots = troots[np.argsort(tmin[troots], kind="stable")]
    T = len(troots)
    number[troots] = np.arange(T)
    table_id = np.where(multi, number[table_of], -1)
    col_min = np.full((L,), np.inf)
    np.minimum.at(col_min, col_of[multi], ulo[multi])
    croots = np.flatnonzero(multi & (col_of == idx))
    col_id = np.full((L,), -1, dtype=np.int64)
    table_boxes = np.zeros((T, 5), dtype=np.float32)
    table_rows, table_cols = np.zeros((T,), dtype=np.int32), np.zeros((T,), dtype=np.int32)
    for tb in range(T):
        members = np.flatnonzero(multi & (table_id == tb))
        table_boxes[tb] = box(members)
        table_rows[tb] = len(np.unique(row_id[members]))
        mine = croots[table_id[croots] == tb]
        mine = mine[np.lexsort((mine, col_min[mine]))]
        table_cols[tb] = len(mine)
        number[mine] = np.arange(len(mine))
        col_id[members] = number[col_of[members]]

    out = {"row_id": row_id.astype(np.int32), "row_pos": row_pos.astype(np.int32), "table_id": table_id.astype(np.int32),
           "col_id": col_id.astype(np.int32), "row_order": row_order.astype(np.int32), "row_start": row_start.astype(np.int32),
           "row_boxes": row_boxes, "row_count": R, "table_boxes": table_boxes, "table_rows": table_rows, "table_cols": table_cols,
           "table_count": T}
    if line_start is not None:
        ls = np.asarray(line_start).astype(np.int64).reshape(-1)
        if len(ls) < L + 1:
            raise ValueError(f"row_grid: line_start of {len(ls)} entries for {L} lines")
        first, ahead = np.zeros((L,), dtype=np.int32), 0
        for k in row_order:
            first[k] = ahead
            lo, hi = int(ls[k]), int(ls[k + 1])
            ahead += hi - lo if 0 <= lo <= hi <= K else 0                          # (a hostile entry: the line's size is 0)
        out["row_first"] = first
    return out


_FIELDS = ("pred_row_ids", "pred_row_pos", "pred_table_ids", "pred_col_ids", "pred_row_rank", "pred_row_boxes", "pred_table_boxes")


def rows_of(instances) -> List[dict]:
    """The rows of one image's `Instances` as the post-processor leaves them with POST_PROCESSING.ALIGN_ROWS, on the host and in
    row order: [{"box": [cx, cy, w, h, a], "table": the table's number or None, "cells": [{"col": the column's number inside
    the table or None, "words": [indices into `instances`, in reading order], "text" (only where the instances have
    pred_texts)}]}], the cells left to right.  Works on an indexed or filtered `Instances` too: a cell or row whose words were
    all removed is absent, the others keep their order and their numbers."""
    for name in _FIELDS:
        if not instances.has(name):
            raise ValueError(f"rows_of: the instances have no {name} (POST_PROCESSING.ALIGN_ROWS is off)")
    rank, rid, rpos, tid, cid = (instances.get(n).detach().cpu().numpy() for n in
                                 ("pred_row_rank", "pred_row_ids", "pred_row_pos", "pred_table_ids", "pred_col_ids"))
    rboxes = instances.pred_row_boxes.detach().cpu().numpy()
    texts = instances.pred_texts if instances.has("pred_texts") else None
    words = np.arange(len(rank))
    out: List[dict] = []
    last_row = last_cell = None
    for k in (int(k) for k in words[np.lexsort((words, rank))]):
        if last_row is None or rid[k] != last_row:
            out.append({"box": [float(v) for v in rboxes[k]], "table": int(tid[k]) if tid[k] >= 0 else None, "cells": []})
            last_row, last_cell = rid[k], None
        if last_cell is None or rpos[k] != last_cell:
            out[-1]["cells"].append({"col": int(cid[k]) if cid[k] >= 0 else None, "words": []})
            last_cell = rpos[k]
        out[-1]["cells"][-1]["words"].append(k)
    if texts is not None:
        for row in out:
            for cell in row["cells"]:
                cell["text"] = " ".join(texts[k] for k in cell["words"])
    return out


def tables_of(instances) -> List[dict]:
    """The tables of one image's `Instances` (POST_PROCESSING.ALIGN_ROWS, with pred_texts), by table number: [{"box", "n_rows",
    "n_cols", "rows": [[the cell's text, or None where the row has no cell in that column, per column]]}].  Two cells of one
    row in one column are joined by a blank.  On a filtered `Instances` the counts are those of what is left."""
    if not instances.has("pred_texts"):
        raise ValueError("tables_of: the instances have no pred_texts")
    rows = rows_of(instances)
    tboxes = instances.pred_table_boxes.detach().cpu().numpy()
    out: Dict[int, dict] = {}
    for row in rows:
        if row["table"] is None:
            continue
        tb = out.setdefault(row["table"], {"box": [float(v) for v in tboxes[row["cells"][0]["words"][0]]], "n_rows": 0, "n_cols": 0,
                                           "rows": []})
        tb["rows"].append(row["cells"])
        tb["n_cols"] = max([tb["n_cols"]] + [c["col"] + 1 for c in row["cells"]])
    for tb in out.values():
        tb["n_rows"] = len(tb["rows"])
        tb["rows"] = [[" ".join(c["text"] for c in cells if c["col"] == col) if any(c["col"] == col for c in cells) else None
                       for col in range(tb["n_cols"])] for cells in tb["rows"]]
    return [out[k] for k in sorted(out)]


def rows_text(instances, cell_sep: str = "\t") -> str:
    """the page row by row: words joined by blanks, the cells of a row by `cell_sep`, rows by a newline"""
    if not instances.has("pred_texts"):
        raise ValueError("rows_text: the instances have no pred_texts")
    return "\n".join(cell_sep.join(cell["text"] for cell in row["cells"]) for row in rows_of(instances))
