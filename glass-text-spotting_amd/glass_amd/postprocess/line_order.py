"""Text lines of one image ordered column by column and cut into blocks: the readable statement, in numpy float64, of what
csrc/line_order.hip computes on the device (include/glass_hip_feature_layout.h has the contract in words), and `blocks_of` /
`page_text`, the host views of the per-word fields the post-processor attaches with POST_PROCESSING.ORDER_LINES.

A line is (cx, cy, w, h, a) as the line grouping writes its line boxes.  Everything is widened to float64 first.  The page
frame P_U, P_V is the width-weighted mean direction of the valid lines.  In it every line has an interval [ulo, uhi] along
the text and [vlo, vhi] down the page.  Two lines whose intervals along the text overlap are ordered top to bottom (rule 1);
two that do not overlap are ordered left to right unless a line between them in height overlaps both (rule 2: a header or a
full-width line separates what is above it from what is below).  The order is a topological sort of these edges that always
emits the ready line with the smallest key (mv, mu, index); on a cycle it emits the smallest un-emitted line and counts it
in `forced`.  Blocks are the maximal runs of the order whose neighbours overlap, descend, lie close and have like heights.

Known limits: two pieces of one row that the line grouping left apart (a table) read column by column (row_grid.py,
POST_PROCESSING.ALIGN_ROWS, keeps them together); L-shaped regions and text at angles far from the page's follow the rules,
not a human.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional

import numpy as np

from .line_grouping import MAX_WORDS, _frame, _tree_sum

MAX_LINES = MAX_WORDS            # GLASS_ORDER_LINES_MAX_K (include/glass_hip_feature_layout.h): lines per image
DEFAULT_PARAMS = {"min_overlap": 0.1, "block_max_gap": 0.8, "block_min_height_ratio": 0.7}


def check_order_params(min_overlap=DEFAULT_PARAMS["min_overlap"], block_max_gap=DEFAULT_PARAMS["block_max_gap"],
                       block_min_height_ratio=DEFAULT_PARAMS["block_min_height_ratio"]) -> Dict[str, float]:
    """the three thresholds as floats; ValueError for one that is no number, not finite, negative, or beyond its range
    (min_overlap < 1, block_min_height_ratio <= 1)"""
    out = {}
    for name, v, top, closed in (("min_overlap", min_overlap, 1.0, False), ("block_max_gap", block_max_gap, math.inf, True),
                                 ("block_min_height_ratio", block_min_height_ratio, 1.0, True)):
        try:
            f = float(v)
        except (TypeError, ValueError):
            raise ValueError(f"order_lines: {name}={v!r} is not a number") from None
        if isinstance(v, bool) or not math.isfinite(f) or f < 0 or f > top or (f == top and not closed):
            raise ValueError(f"order_lines: {name}={v!r}: needs a finite value in [0, {top}{']' if closed else ')'}")
        out[name] = f
    return out


def _between_exists(O: np.ndarray, run_lo: np.ndarray, run_hi: np.ndarray) -> np.ndarray:
    """[a, b]: is there a c with O[c, a], O[c, b] and a rank in [run_hi[first], run_lo[second]), first / second the pair in
    rank order - i.e. an mv strictly between theirs.  Bit-packed rows, one row a at a time."""
    V = len(O)
    bits = np.packbits(O, axis=1, bitorder="little")                              # [V, ceil(V / 8)]
    below = np.packbits(np.arange(V)[None, :] < np.arange(V + 1)[:, None], axis=1, bitorder="little")   # below[x]: ranks < x
    ranks = np.arange(V)
    out = np.zeros((V, V), dtype=bool)
    for a in range(V):
        lo = np.where(a < ranks, run_hi[a], run_hi)
        hi = np.where(a < ranks, run_lo, run_lo[a])
        hi = np.maximum(hi, lo)                                                   # (an empty range)
        out[a] = (bits[a][None, :] & bits & below[hi] & ~below[lo]).any(axis=1)
    return out


def order_lines_host(line_boxes, params: Optional[dict] = None, line_start=None, K: int = MAX_LINES) -> dict:
    """line_boxes [L, 5] float32 (L <= MAX_LINES) -> {"page_rank" [L], "page_order" [L], "block_id" [L], "block_start" [B + 1]
    (int32), "block_boxes" float32 [B, 5], "block_count" B, "forced"} and, with `line_start` (int [L + 1] or longer, the line
    grouping's CSR; `K` is the padded size the device checks its entries against), "line_first" [L].  `params`: any of
    DEFAULT_PARAMS' keys."""
    p = check_order_params(**(params or {}))
    b32 = np.ascontiguousarray(np.asarray(line_boxes, dtype=np.float32).reshape(-1, 5))
    L = len(b32)
    if L > MAX_LINES:
        raise ValueError(f"order_lines: {L} lines (max {MAX_LINES})")
    wide = b32.astype(np.float64)
    valid = np.isfinite(wide).all(axis=1)
    valid &= np.where(valid, (wide[:, 2] > 0) & (wide[:, 3] > 0), False)
    cx, cy, w, h, a = np.where(valid[:, None], wide, 0.0).T
    t = a * np.pi / 180.0
    ux, uy = np.cos(t), -np.sin(t)                                   # u; v = (-uy, ux) = (sin t, cos t)

    # ---- the page frame; intervals and keys in it
    PU = _frame(_tree_sum(w * ux), _tree_sum(w * uy), _tree_sum(w), (1.0, 0.0))      # (w = 0 for an invalid line)
    PV = (-PU[1], PU[0])
    ax, ay, bx, by = w / 2 * ux, w / 2 * uy, h / 2 * -uy, h / 2 * ux
    pu, pv = [], []
    for su, sv in ((1.0, 1.0), (-1.0, 1.0), (1.0, -1.0), (-1.0, -1.0)):
        px, py = cx + su * ax + sv * bx, cy + su * ay + sv * by
        pu.append(px * PU[0] + py * PU[1])
        pv.append(px * PV[0] + py * PV[1])
    ulo, uhi, vlo, vhi = np.min(pu, axis=0), np.max(pu, axis=0), np.min(pv, axis=0), np.max(pv, axis=0)
    mu, mv = cx * PU[0] + cy * PU[1], cx * PV[0] + cy * PV[1]

    # ---- the valid lines in key order (mv, mu, index); everything below is indexed by that rank
    vs = np.flatnonzero(valid)
    vs = vs[np.lexsort((vs, mu[vs], mv[vs]))]
    V = len(vs)
    ulo, uhi, vlo, vhi, mu, mv, hh = (x[vs] for x in (ulo, uhi, vlo, vhi, mu, mv, h))
    run_lo, run_hi = np.searchsorted(mv, mv, side="left"), np.searchsorted(mv, mv, side="right")
    i, j = np.s_[:, None], np.s_[None, :]
    O = np.minimum(uhi[i], uhi[j]) - np.maximum(ulo[i], ulo[j]) > p["min_overlap"] * np.minimum(uhi[i] - ulo[i], uhi[j] - ulo[j])
    O &= ~np.eye(V, dtype=bool)
    E = O & (mv[i] < mv[j])                                                        # rule 1
    E |= ~O & ~np.eye(V, dtype=bool) & (mu[i] < mu[j]) & ~_between_exists(O, run_lo, run_hi)      # rule 2

    # ---- the order: the ready line with the smallest key, or on a cycle the smallest un-emitted line
    indeg = E.sum(axis=0)
    left = np.ones((V,), dtype=bool)
    seq, forced = [], 0
    for _ in range(V):
        ready = np.flatnonzero(left & (indeg == 0))
        if len(ready):
            e = int(ready[0])
        else:
            e = int(np.flatnonzero(left)[0])
            forced += 1
        left[e] = False
        indeg = indeg - E[e]
        seq.append(e)

    # ---- blocks: maximal runs of the order
    blocks = []                                                                    # (box float32 [5], members as line indices)
    run: List[int] = []

    def close():
        if run:
            umin, umax, vmin, vmax = ulo[run].min(), uhi[run].max(), vlo[run].min(), vhi[run].max()
            cu, cv = (umin + umax) / 2, (vmin + vmax) / 2
            box = np.array([cu * PU[0] + cv * PV[0], cu * PU[1] + cv * PV[1], umax - umin, vmax - vmin,
                            math.atan2(-PU[1], PU[0]) * 180.0 / math.pi])
            blocks.append((box.astype(np.float32), [int(vs[r]) for r in run]))
    for q in seq:
        if run:
            pr = run[-1]
            H, hmin = max(hh[pr], hh[q]), min(hh[pr], hh[q])
            if not (O[pr, q] and mv[pr] < mv[q] and vlo[q] - vhi[pr] <= p["block_max_gap"] * H
                    and hmin >= p["block_min_height_ratio"] * H):
                close()
                run = []
        run.append(q)
    close()
    for k in np.flatnonzero(~valid):                                               # the invalid lines, in index order
        blocks.append((b32[k].copy(), [int(k)]))

    B = len(blocks)
    out = {"page_rank": np.zeros((L,), dtype=np.int32), "page_order": np.zeros((L,), dtype=np.int32),
           "block_id": np.zeros((L,), dtype=np.int32), "block_start": np.zeros((B + 1,), dtype=np.int32),
           "block_boxes": np.zeros((B, 5), dtype=np.float32), "block_count": B, "forced": forced}
    at = 0
    for bid, (box, members) in enumerate(blocks):
        out["block_start"][bid] = at
        out["block_boxes"][bid] = box
        for k in members:
            out["page_rank"][k], out["page_order"][at], out["block_id"][k] = at, k, bid
            at += 1
    out["block_start"][B] = at
    if line_start is not None:
        ls = np.asarray(line_start).astype(np.int64).reshape(-1)
        if len(ls) < L + 1:
            raise ValueError(f"order_lines: line_start of {len(ls)} entries for {L} lines")
        first, ahead = np.zeros((L,), dtype=np.int32), 0
        for k in out["page_order"]:
            first[k] = ahead
            lo, hi = int(ls[k]), int(ls[k + 1])
            ahead += hi - lo if 0 <= lo <= hi <= K else 0                          # (a hostile entry: the line's size is 0)
        out["line_first"] = first
    return out


def blocks_of(instances) -> List[dict]:
    """The blocks of one image's `Instances` as the post-processor leaves them with POST_PROCESSING.ORDER_LINES, on the host and
    in page order: [{"box": [cx, cy, w, h, a], "lines": [{"box", "words": [indices into `instances`, in reading order], "text"
    (only where the instances have pred_texts)}]}].  Works on an indexed or filtered `Instances` too: a line or block whose
    words were all removed is absent, the others keep their order."""
    for name in ("pred_page_rank", "pred_block_ids", "pred_block_boxes", "pred_line_ids", "pred_line_boxes"):
        if not instances.has(name):
            raise ValueError(f"blocks_of: the instances have no {name} (POST_PROCESSING.ORDER_LINES is off)")
    rank = instances.pred_page_rank.detach().cpu().numpy()
    bids = instances.pred_block_ids.detach().cpu().numpy()
    lids = instances.pred_line_ids.detach().cpu().numpy()
    bboxes = instances.pred_block_boxes.detach().cpu().numpy()
    lboxes = instances.pred_line_boxes.detach().cpu().numpy()
    texts = instances.pred_texts if instances.has("pred_texts") else None
    words = np.arange(len(rank))
    out: List[dict] = []
    last_block = last_line = None
    for k in (int(k) for k in words[np.lexsort((words, rank))]):
        if last_block is None or bids[k] != last_block:
            out.append({"box": [float(v) for v in bboxes[k]], "lines": []})
            last_block, last_line = bids[k], None
        if last_line is None or lids[k] != last_line:
            out[-1]["lines"].append({"box": [float(v) for v in lboxes[k]], "words": []})
            last_line = lids[k]
        out[-1]["lines"][-1]["words"].append(k)
    if texts is not None:
        for block in out:
            for line in block["lines"]:
                line["text"] = " ".join(texts[k] for k in line["words"])
    return out


def page_text(instances) -> str:
    """the page as text: words joined by blanks, lines by a newline, blocks by a blank line, in page order"""
    if not instances.has("pred_texts"):
        raise ValueError("page_text: the instances have no pred_texts")
    return "\n\n".join("\n".join(line["text"] for line in block["lines"]) for block in blocks_of(instances))
