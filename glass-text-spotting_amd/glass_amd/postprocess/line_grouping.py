"""Words of one image grouped into text lines in reading order: the readable statement, in numpy float64, of what
csrc/line_group.hip computes on the device (include/glass_hip_feature_lines.h has the contract in words), and `lines_of`,
the host view of the per-word fields the post-processor attaches with POST_PROCESSING.GROUP_LINES.

A word is (cx, cy, w, h, a): float32, a in degrees, the convention of `boxes_to_polygons`.  Everything is widened to float64
first.  u = (cos t, -sin t) with t = a pi / 180 is the word's reading direction, v = (sin t, cos t) its downward direction.
Words are linked by a symmetric pair rule, the connected components of the links are the lines, words are ordered along their
line's direction, lines down the page, and every line gets its enclosing rotated box.  Top-to-bottom and no more: two columns
interleave row by row.  POST_PROCESSING.ORDER_LINES (line_order.py) orders these lines column by column and cuts them into
blocks; nothing here changes with it.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional

import numpy as np

MAX_WORDS = 1024                 # GLASS_GROUP_LINES_MAX_K (include/glass_hip_feature_lines.h): words per image
DEFAULT_PARAMS = {"max_angle_diff": 15.0, "min_height_ratio": 0.5, "max_offset": 0.5, "max_gap": 1.0}


def check_line_params(max_angle_diff=DEFAULT_PARAMS["max_angle_diff"], min_height_ratio=DEFAULT_PARAMS["min_height_ratio"],
                      max_offset=DEFAULT_PARAMS["max_offset"], max_gap=DEFAULT_PARAMS["max_gap"]) -> Dict[str, float]:
    """the four thresholds as floats; ValueError for one that is no number, not finite, negative, or beyond its range
    (max_angle_diff <= 180 degrees, min_height_ratio <= 1)"""
    out = {}
    for name, v, top in (("max_angle_diff", max_angle_diff, 180.0), ("min_height_ratio", min_height_ratio, 1.0),
                         ("max_offset", max_offset, math.inf), ("max_gap", max_gap, math.inf)):
        try:
            f = float(v)
        except (TypeError, ValueError):
            raise ValueError(f"group_lines: {name}={v!r} is not a number") from None
        if isinstance(v, bool) or not math.isfinite(f) or f < 0 or f > top:
            raise ValueError(f"group_lines: {name}={v!r}: needs a finite value in [0, {top}]")
        out[name] = f
    return out


def _tree_sum(x: np.ndarray) -> float:
    """the sum over a fixed tree of MAX_WORDS slots (slot i + slot i + stride, stride halving), zeros beyond len(x)"""
    s = np.zeros((MAX_WORDS,), dtype=np.float64)
    s[:len(x)] = x
    stride = MAX_WORDS // 2
    while stride:
        s[:stride] = s[:stride] + s[stride:2 * stride]
        stride //= 2
    return float(s[0])


def _frame(Dx: float, Dy: float, Sw: float, fallback):
    nrm = math.sqrt(Dx * Dx + Dy * Dy)
    return (Dx / nrm, Dy / nrm) if nrm > 1e-12 * Sw else fallback


def group_lines_host(boxes, params: Optional[dict] = None) -> dict:
    """boxes [n, 5] float32 (n <= MAX_WORDS) -> {"line_id" [n], "line_pos" [n], "order" [n], "line_start" [L + 1] (int32),
    "line_boxes" float32 [L, 5], "line_count" L}.  `params`: any of DEFAULT_PARAMS' keys."""
    p = check_line_params(**(params or {}))
    b32 = np.ascontiguousarray(np.asarray(boxes, dtype=np.float32).reshape(-1, 5))
    n = len(b32)
    if n > MAX_WORDS:
        raise ValueError(f"group_lines: {n} words (max {MAX_WORDS})")
    wide = b32.astype(np.float64)
    valid = np.isfinite(wide).all(axis=1)
    valid &= np.where(valid, (wide[:, 2] > 0) & (wide[:, 3] > 0), False)
    cx, cy, w, h, a = np.where(valid[:, None], wide, 0.0).T          # (an invalid word takes part in nothing below)
    t = a * np.pi / 180.0
    ux, uy = np.cos(t), -np.sin(t)                                   # u; v = (-uy, ux) = (sin t, cos t)

    # ---- Link(i, j) at [i, j]: d = c_j - c_i
    i, j = np.s_[:, None], np.s_[None, :]
    dx, dy = cx[j] - cx[i], cy[j] - cy[i]
    r = np.fmod(np.abs(a[j] - a[i]), 360.0)
    r = np.where(r > 180.0, 360.0 - r, r)                            # |wrap(a_j - a_i)|, the same bits both ways round
    H, hmin = np.maximum(h[i], h[j]), np.minimum(h[i], h[j])
    half = (w[i] + w[j]) / 2
    link = valid[i] & valid[j] & ~np.eye(n, dtype=bool)
    link &= r <= p["max_angle_diff"]
    link &= hmin >= p["min_height_ratio"] * H
    link &= (np.abs(dx * -uy[i] + dy * ux[i]) <= p["max_offset"] * H) & (np.abs(dx * -uy[j] + dy * ux[j]) <= p["max_offset"] * H)
    link &= (np.abs(dx * ux[i] + dy * uy[i]) - half <= p["max_gap"] * H) & (np.abs(dx * ux[j] + dy * uy[j]) - half <= p["max_gap"] * H)

    # ---- lines: connected components, each named by its smallest index
    label = np.full((n,), -1, dtype=np.int64)
    for seed in range(n):
        if label[seed] >= 0:
            continue
        label[seed] = seed
        frontier = np.array([seed])
        while len(frontier):
            reach = link[frontier].any(axis=0) & (label < 0)
            label[reach] = seed
            frontier = np.flatnonzero(reach)

    # ---- the page frame from all valid words
    PU = _frame(_tree_sum(w * ux), _tree_sum(w * uy), _tree_sum(w), (1.0, 0.0))      # (w = 0 for an invalid word)
    PV = (-PU[1], PU[0])

    # ---- every valid line: frame (sums in index order), order inside, box
    lines = []
    for root in np.flatnonzero(label == np.arange(n)):
        root = int(root)
        if not valid[root]:
            lines.append({"valid": False, "root": root, "words": [root], "box": b32[root].copy()})
            continue
        members = np.flatnonzero(label == root)
        Dx = Dy = Sw = 0.0
        for k in members:
            Dx += w[k] * ux[k]; Dy += w[k] * uy[k]; Sw += w[k]
        U = _frame(float(Dx), float(Dy), float(Sw), (float(ux[root]), float(uy[root])))
        V = (-U[1], U[0])
        proj = cx[members] * U[0] + cy[members] * U[1]
        words = members[np.lexsort((members, proj))]                 # ascending c.U, ties by index
        pu, pv = [], []
        ax, ay = w[members] / 2 * ux[members], w[members] / 2 * uy[members]              # (w / 2) u
        bx, by = h[members] / 2 * -uy[members], h[members] / 2 * ux[members]             # (h / 2) v
        for su, sv in ((1.0, 1.0), (-1.0, 1.0), (1.0, -1.0), (-1.0, -1.0)):
            px, py = cx[members] + su * ax + sv * bx, cy[members] + su * ay + sv * by
            pu.append(px * U[0] + py * U[1])
            pv.append(px * V[0] + py * V[1])
        umin, umax, vmin, vmax = np.min(pu), np.max(pu), np.min(pv), np.max(pv)
        cu, cv = (umin + umax) / 2, (vmin + vmax) / 2
        mx, my = cu * U[0] + cv * V[0], cu * U[1] + cv * V[1]
        box = np.array([mx, my, umax - umin, vmax - vmin, math.atan2(-U[1], U[0]) * 180.0 / math.pi])
        lines.append({"valid": True, "root": root, "words": [int(k) for k in words], "box": box.astype(np.float32),
                      "key": (mx * PV[0] + my * PV[1], mx * PU[0] + my * PU[1], root)})

    # ---- lines down the page (m.P_V, then m.P_U, then smallest index), the invalid words after them in index order
    lines.sort(key=lambda ln: (0,) + ln["key"] if ln["valid"] else (1, ln["root"]))
    L = len(lines)
    out = {"line_id": np.zeros((n,), dtype=np.int32), "line_pos": np.zeros((n,), dtype=np.int32),
           "order": np.zeros((n,), dtype=np.int32), "line_start": np.zeros((L + 1,), dtype=np.int32),
           "line_boxes": np.zeros((L, 5), dtype=np.float32), "line_count": L}
    at = 0
    for l, ln in enumerate(lines):
        out["line_start"][l] = at
        out["line_boxes"][l] = ln["box"]
        for pos, k in enumerate(ln["words"]):
            out["line_id"][k], out["line_pos"][k], out["order"][at] = l, pos, k
            at += 1
    out["line_start"][L] = at
    return out


def lines_of(instances) -> List[dict]:
    """The lines of one image's `Instances` as the post-processor leaves them with POST_PROCESSING.GROUP_LINES, on the host and
    in reading order: [{"box": [cx, cy, w, h, a], "words": [indices into `instances`, in reading order], "text": the words'
    pred_texts joined by a blank (only where the instances have pred_texts)}].  Works on an indexed or filtered `Instances`
    too: a line whose words were all removed is absent, the others keep their order."""
    for name in ("pred_line_ids", "pred_line_pos", "pred_line_boxes"):
        if not instances.has(name):
            raise ValueError(f"lines_of: the instances have no {name} (POST_PROCESSING.GROUP_LINES is off)")
    ids = instances.pred_line_ids.detach().cpu().numpy()
    pos = instances.pred_line_pos.detach().cpu().numpy()
    boxes = instances.pred_line_boxes.detach().cpu().numpy()
    texts = instances.pred_texts if instances.has("pred_texts") else None
    out = []
    for l in sorted(set(ids.tolist())):
        members = np.flatnonzero(ids == l)
        members = [int(k) for k in members[np.lexsort((members, pos[members]))]]
        line = {"box": [float(v) for v in boxes[members[0]]], "words": members}
        if texts is not None:
            line["text"] = " ".join(texts[k] for k in members)
        out.append(line)
    return out
