"""Where inside its box every character of a word lies (MODEL.ROI_RECOGNIZER_HEAD.CHAR_BOXES).

Every step of the attention decoder forms a softmax over the T encoder positions of its RoI, and those positions lie evenly
along the width of the box the recogniser pooled.  `glass_forced_attention` returns these rows for a replay of the emitted
symbols, `glass_char_spans` turns them into normalised spans along the box and `glass_char_quads` into quads in the image
(include/glass_hip_feature_chars.h has the contract).  This module holds

  * `char_spans_host`: the statement of the spans in numpy float64, which the kernel is tested against;
  * the packing of a word's rows into ONE float payload [R, L + 1, 3] that takes the path `pred_text_dist` takes through the
    model (`pack_chars`, `unpack_chars`, `attach_chars`);
  * `char_quads(instances)` and `chars_of(instances, text_encoder)`, what a caller reads.

Attention need not be monotone: the spans are defined all the same, and `pred_char_monotone` is the quality signal a caller
filters on.  No character-level evaluation and no character masks are built on top of this.
"""
from __future__ import annotations

import math
from typing import Dict, List

import numpy as np

MAX_STEPS = 64        # CHAR_SPANS_MAX_STEPS / CHAR_SPANS_MAX_COLUMNS of ops.native: the limits of glass_char_spans
MAX_COLUMNS = 64
CHAR_FIELDS = ("pred_char_spans", "pred_char_centres", "pred_char_count", "pred_char_monotone", "pred_char_frames")


def char_spans_host(attention, targets, lengths, eos: int) -> Dict[str, np.ndarray]:
    """The statement of glass_char_spans: attention [R, L, T], targets [R, L] integers, lengths [R] integers ->
    {"spans" float32 [R,L,2], "centres" float32 [R,L], "spreads" float32 [R,L], "count", "monotone", "valid" int32 [R]}.
    Every value is widened to float64, every formula below is float64, the results are rounded to float32 once.

    Word r: len = min(max(lengths[r], 0), L); m = len - 1 if the last of these symbols is `eos`, else len (a symbol is only
    compared, never used as an index).  Column j lies at p_j = (j + 0.5) / T.  For t < m: S = sum_j a_tj, the centre
    c_t = sum_j a_tj p_j / S, the spread s_t = sqrt(sum_j a_tj (p_j - c_t)^2 / S).  A row with S not finite or <= 0, or with an
    entry that is negative or not finite, makes the WORD invalid: count 0, every output zero, valid 0.
    Boundaries b_t = (c_t + c_{t+1}) / 2; the outer edges are mirrored, e_L = c_0 - |b_0 - c_0| and
    e_R = c_{m-1} + |c_{m-1} - b_{m-2}|, and clamped to [0, 1]; m = 1 gives (0, 1).  The span of step t is (min(l, r), max(l, r))
    of its two boundaries.  monotone = 1 iff the centres strictly increase (m <= 1: 1)."""
    att = np.asarray(attention)
    if att.ndim != 3 or not (1 <= att.shape[1] <= MAX_STEPS and 1 <= att.shape[2] <= MAX_COLUMNS):
        raise ValueError(f"char_spans_host: attention {att.shape}: needs [R, L, T] with 1 <= L <= {MAX_STEPS} steps and "
                         f"1 <= T <= {MAX_COLUMNS} columns")
    R, L, T = att.shape
    tg, ln = np.asarray(targets), np.asarray(lengths)
    if tg.shape != (R, L) or ln.shape != (R,):
        raise ValueError(f"char_spans_host: targets {tg.shape} / lengths {ln.shape}: need [{R}, {L}] and [{R}]")
    att = att.astype(np.float64)
    spans = np.zeros((R, L, 2), dtype=np.float32)
    centres = np.zeros((R, L), dtype=np.float32)
    spreads = np.zeros((R, L), dtype=np.float32)
    count = np.zeros((R,), dtype=np.int32)
    monotone = np.zeros((R,), dtype=np.int32)
    valid = np.zeros((R,), dtype=np.int32)
    p = (np.arange(T, dtype=np.float64) + 0.5) / float(T)
    for r in range(R):
        n = min(max(int(ln[r]), 0), L)
        m = n - 1 if n > 0 and int(tg[r, n - 1]) == int(eos) else n
        a = att[r, :m]
        with np.errstate(all="ignore"):
            S = a.sum(axis=1)
            ok = bool(np.all(np.isfinite(a)) and np.all(a >= 0.0) and np.all(np.isfinite(S)) and np.all(S > 0.0))
            if not ok:
                continue
            c = (a * p).sum(axis=1) / S
            d = p[None, :] - c[:, None]
            s = np.sqrt((a * (d * d)).sum(axis=1) / S)
        valid[r], count[r] = 1, m
        monotone[r] = int(bool(np.all(c[1:] > c[:-1])))
        if m == 0:
            continue
        if m == 1:
            left, right = np.array([0.0]), np.array([1.0])
        else:
            b = (c[:-1] + c[1:]) / 2.0
            e_l = min(max(c[0] - abs(b[0] - c[0]), 0.0), 1.0)
            e_r = min(max(c[-1] + abs(c[-1] - b[-1]), 0.0), 1.0)
            left, right = np.concatenate([[e_l], b]), np.concatenate([b, [e_r]])
        spans[r, :m, 0] = np.minimum(left, right)
        spans[r, :m, 1] = np.maximum(left, right)
        centres[r, :m] = c
        spreads[r, :m] = s
    return {"spans": spans, "centres": centres, "spreads": spreads, "count": count, "monotone": monotone, "valid": valid}


def char_quads_host(spans, count, frames) -> np.ndarray:
    """The statement of glass_char_quads in numpy float64: spans [R, L, 2], count [R], frames [R, 5] -> float32 [R, L, 4, 2]."""
    sp, ct, fr = np.asarray(spans, dtype=np.float64), np.asarray(count), np.asarray(frames, dtype=np.float64)
    R, L = sp.shape[:2]
    out = np.zeros((R, L, 4, 2), dtype=np.float64)
    for r in range(R):
        cx, cy, w, h, ang = fr[r]
        if not (np.all(np.isfinite(fr[r])) and w > 0 and h > 0):
            continue
        th = ang * 3.14159265358979323846 / 180.0
        u = np.array([math.cos(th), -math.sin(th)])
        v = np.array([math.sin(th), math.cos(th)])
        for t in range(min(max(int(ct[r]), 0), L)):
            lo, hi = sp[r, t]
            off = ((lo + hi) / 2.0 - 0.5) * w
            mid = np.array([cx, cy]) + off * u
            e, g = (hi - lo) * w / 2.0, h / 2.0
            out[r, t] = [mid - e * u - g * v, mid + e * u - g * v, mid + e * u + g * v, mid - e * u + g * v]
    return out.astype(np.float32)


# ---------------------------------------------------------------------- the payload that travels with the text rows
def pack_chars(chars: dict):
    """what ops.native.char_spans returned -> ONE float32 device tensor [R, L + 1, 3]: rows t < L hold (lo, hi, centre) of step
    t, row L holds (count, monotone, valid) - small integers, exact in float32.  One tensor, so that the ordered compaction
    of detections_finalize (its per-RoI payload slot) and the post-processor's gather move it like `pred_text_dist`."""
    import torch
    spans, centres = chars["spans"], chars["centres"]
    R, L = centres.shape
    out = torch.empty((R, L + 1, 3), dtype=torch.float32, device=spans.device)
    out[:, :L, :2] = spans
    out[:, :L, 2] = centres
    out[:, L, 0] = chars["count"]
    out[:, L, 1] = chars["monotone"]
    out[:, L, 2] = chars["valid"]
    return out


def unpack_chars(packed) -> dict:
    """the inverse of `pack_chars` on any leading shape [..., L + 1, 3] -> the Instances fields (without the frames):
    pred_char_spans [..., L, 2], pred_char_centres [..., L], pred_char_count int64 [...], pred_char_monotone bool [...]"""
    import torch
    L = int(packed.shape[-2]) - 1
    return {"pred_char_spans": packed[..., :L, :2], "pred_char_centres": packed[..., :L, 2],
            "pred_char_count": packed[..., L, 0].to(torch.int64), "pred_char_monotone": packed[..., L, 1] > 0}


def attach_chars(instances, packed, frames) -> None:
    """set the five pred_char_* fields of one image's Instances from its packed rows [Ri, L + 1, 3] and the boxes the
    recogniser pooled [Ri, 5] (copied: the post-processor's merge step may enlarge pred_boxes, the characters' frame stays)"""
    for name, t in unpack_chars(packed).items():
        instances.set(name, t)
    instances.set("pred_char_frames", frames.clone())


# ---------------------------------------------------------------------- what a caller reads
def _need(instances, who: str) -> None:
    missing = [f for f in CHAR_FIELDS if not instances.has(f)]
    if missing:
        raise ValueError(f"{who}: the instances carry no {missing[0]} (set MODEL.ROI_RECOGNIZER_HEAD.CHAR_BOXES True)")


def char_quads(instances):
    """The quads of every character of one image's Instances: float32 device tensor [Ri, L, 4, 2], the four corners of step t
    of word i in the order `boxes_to_polygons` emits for a box, in the pixels of `pred_char_frames`; zeros from the word's
    `pred_char_count` on.  One glass_char_quads call.  ValueError without the pred_char_* fields."""
    import torch
    from ..ops import native as K
    _need(instances, "char_quads")
    spans = instances.pred_char_spans.contiguous()
    count = instances.pred_char_count.to(torch.int32).contiguous()
    return K.char_quads(spans, count, instances.pred_char_frames.contiguous())


def chars_of(instances, text_encoder) -> List[List[dict]]:
    """Per word of one image's Instances, the characters of the decoder steps before the stop:
    [{"char", "quad", "centre", "prob"}] - the class name of the step's arg-max in `pred_text_prob`, its four corners
    [[x, y]] * 4, the image point of its attention centre on the box's axis [x, y], and the step's probability (the maximum of
    its row of `pred_text_prob`).
    The rows align with the DECODER STEPS of `pred_text_prob`, not with a string the writer trimmed afterwards: `pred_texts`
    has its special tokens stripped, so its k-th letter need not be step k; "char" here is the untrimmed class name of the
    step ("[UNK]" included).  A word whose attention rows were invalid has no entries.  One glass_char_quads call and one
    read-back.  ValueError without the pred_char_* fields or without `pred_text_prob`."""
    _need(instances, "chars_of")
    if not instances.has("pred_text_prob"):
        raise ValueError("chars_of: the instances carry no pred_text_prob")
    quads = char_quads(instances).cpu().numpy()
    count = instances.pred_char_count.cpu().numpy()
    centres = instances.pred_char_centres.cpu().numpy().astype(np.float64)
    frames = instances.pred_char_frames.cpu().numpy().astype(np.float64)
    prob, sym = (t.cpu().numpy() for t in instances.pred_text_prob.max(dim=-1))
    names = text_encoder.character
    out = []
    for i in range(len(count)):
        cx, cy, w, _, ang = frames[i]
        th = ang * math.pi / 180.0
        word = []
        for t in range(int(count[i])):
            off = (centres[i, t] - 0.5) * w
            k = int(sym[i, t])
            word.append({"char": names[k] if 0 <= k < len(names) else "", "quad": quads[i, t].tolist(),
                         "centre": [float(cx + off * math.cos(th)), float(cy - off * math.sin(th))], "prob": float(prob[i, t])})
        out.append(word)
    return out
