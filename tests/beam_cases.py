"""Beam search of the attention decoder restated in float64 on the CPU, and the generated cases of the beam-search tests.

`replay` walks reference prediction_aster.py:101-222 (as restated by ASTER_V2.beam_search) with three things pinned down:
  * the decoder step (additive attention, GRU cell, fc) is computed from the state-dict weights in float64, or - `replay_with`
    - taken from a callback, so that a GPU test can drive the arithmetic through the existing kernel
    (`K.attention_decode_step`) while the search itself stays float64 on the host;
  * log-softmax is float64;
  * the top-k is a rule, not `torch.topk`: score descending, then flat index beam*C + class ascending, -inf last in index
    order (a stable sort); the two sorts of the back-tracking follow the same rule over slots.
It returns all k hypotheses, their lengths and per-step scores, and per item the smallest selection gap (k-th selected
candidate against the best one not selected, over all steps) and the smallest gap between neighbouring final scores.
"""
import math
from types import SimpleNamespace

import numpy as np
import torch

PRE = "roi_heads.recognizer_head.decoder."
Q = PRE + "recognizer.decoder."


def decoder_sd(num_classes=97, seed=1234, fc_scale=6.0, bias0=2.0, eos=0):
    """synthetic decoder weights for `num_classes`, with the golden's edits (oracle/make_golden.py --beam): a sharper output
    layer separates the beams, a boosted <eos> bias makes sequences end at different steps"""
    from glass_amd.utils.synth import make_state_dict
    sd = dict(make_state_dict(seed, num_chars=num_classes, parts=("recog",)))
    sd[Q + "fc.weight"] = sd[Q + "fc.weight"] * float(fc_scale)
    sd[Q + "fc.bias"] = sd[Q + "fc.bias"].clone()
    sd[Q + "fc.bias"][eos] += float(bias0)
    return sd


def decoder_cfg(num_classes, max_len):
    """the two keys ASTER_V2 reads, for a decoder of `num_classes` classes and `max_len` steps"""
    rc = SimpleNamespace(CHARACTER_SET=[chr(0x100 + i) for i in range(num_classes - 2)], MAX_WORD_LENGTH=max_len - 1)
    return SimpleNamespace(MODEL=SimpleNamespace(ROI_RECOGNIZER_HEAD=rc))


def rand_x(B, T, seed, D=256):
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    return torch.randn((B, T, D), generator=g, dtype=torch.float32)


# (name, B, k, T, max_len, C, seed): the smallest shapes that cross every boundary of the kernels - B 1 / 3 / 17, every row
# blocking of the step kernels (k 1, 2, 3 -> 4, 4, 5 -> 8, 16) and k == C, T 7 / 32 / 64 (not a multiple of the 4 wavefronts, half,
# full), max_len 1 / 26 / 64, C 5 / 97 / 256 (one, two and four 64-lane pieces), and B*k = 512 rows, where the
# step kernels of the host path take their 2-row blocking.  Seeds: of 100..115 the one with the largest smallest gap in the
# float64 replay (a property of the inputs and the rule alone, computed on the CPU)
CASES = [
    ("b1_k1_t7_l1", 1, 1, 7, 1, 97, 101),
    ("b3_k2_t32_l26", 3, 2, 32, 26, 97, 113),
    ("b17_k5_t64_l64", 17, 5, 64, 64, 97, 108),
    ("b3_k5_t7_l26_c5", 3, 5, 7, 26, 5, 104),
    ("b3_k16_t32_l26_c256", 3, 16, 32, 26, 256, 101),
    ("b32_k16_t7_l6_rows512", 32, 16, 7, 6, 97, 114),
    ("b2_k3_t7_l6_c13", 2, 3, 7, 6, 13, 101),       # the 4-row blocking with one padding row ...
    ("b2_k4_t7_l6_c13", 2, 4, 7, 6, 13, 102),       # ... and full
]


def f64_step(sd, x, xproj):
    """-> step(state [R,D] f64, y_prev [R] long, item [R] long) -> (logits [R,C] f64, state' [R,D] f64): DecoderUnit.forward
    (reference :291-302) with AttentionUnit.forward (:247-266) from the state-dict weights; row r attends over x[item[r]]"""
    w = {n: sd[Q + n].double() for n in ("attention_unit.sEmbed.weight", "attention_unit.sEmbed.bias", "attention_unit.wEmbed.weight",
                                        "attention_unit.wEmbed.bias", "tgt_embedding.weight", "gru.weight_ih_l0", "gru.weight_hh_l0",
                                        "gru.bias_ih_l0", "gru.bias_hh_l0", "fc.weight", "fc.bias")}
    temp = float(sd[Q + "temperature"].reshape(-1)[0]) if (Q + "temperature") in sd else 1.0
    x, xproj = x.double(), xproj.double()

    def step(state, y_prev, item):
        sp = state @ w["attention_unit.sEmbed.weight"].t() + w["attention_unit.sEmbed.bias"]
        e = torch.tanh(sp[:, None, :] + xproj[item]) @ w["attention_unit.wEmbed.weight"].reshape(-1) + w["attention_unit.wEmbed.bias"]
        alpha = torch.softmax(e, dim=1)
        ctx = (alpha[:, :, None] * x[item]).sum(1)
        inp = torch.cat([w["tgt_embedding.weight"][y_prev], ctx], 1)
        gi = inp @ w["gru.weight_ih_l0"].t() + w["gru.bias_ih_l0"]
        gh = state @ w["gru.weight_hh_l0"].t() + w["gru.bias_hh_l0"]
        i_r, i_z, i_n = gi.chunk(3, 1)
        h_r, h_z, h_n = gh.chunk(3, 1)
        r, z = torch.sigmoid(i_r + h_r), torch.sigmoid(i_z + h_z)
        n = torch.tanh(i_n + r * h_n)
        h = (1.0 - z) * n + z * state
        return (h @ w["fc.weight"].t() + w["fc.bias"]) * temp, h
    return step


def xproj_f64(sd, x):
    return x.double() @ sd[Q + "attention_unit.xEmbed.weight"].double().reshape(256, 256).t() + sd[Q + "attention_unit.xEmbed.bias"].double()


def order(v):
    """indices of v [n] by value descending, then index ascending; -inf last in index order"""
    return torch.sort(-v, stable=True).indices


def backtrack(sc, pr, sy, eos):
    """the reference's back-tracking (:161-222) on decision tables sc / pr / sy [L,B,k] (pr = predecessor SLOT 0..k-1).
    -> symbols [B,k,L], scores [B,k], lengths [B,k], step_scores [B,k,L] (the score after step t along the hypothesis's own
    ancestor chain; meaningful for t < length), all k hypotheses in final order."""
    L, B, k = sc.shape
    sym = torch.zeros((B, k, L), dtype=torch.long)
    scores = torch.zeros((B, k), dtype=torch.float64)
    lengths = torch.zeros((B, k), dtype=torch.long)
    steps = torch.zeros((B, k, L), dtype=torch.float64)
    for b in range(B):
        o = order(sc[L - 1, b])
        s = sc[L - 1, b][o].clone()
        tp = o.clone()
        ln = [L] * k
        found = 0
        p_sym = torch.zeros((L, k), dtype=torch.long)
        p_sc = torch.zeros((L, k), dtype=torch.float64)
        for t in range(L - 1, -1, -1):
            cur, cur_sc = sy[t, b][tp].clone(), sc[t, b][tp].clone()
            tp = pr[t, b][tp].clone()
            for j in range(k - 1, -1, -1):
                if int(sy[t, b, j]) == eos:
                    res = k - (found % k) - 1
                    found += 1
                    tp[res], cur[res], cur_sc[res] = pr[t, b, j], sy[t, b, j], sc[t, b, j]
                    s[res] = sc[t, b, j]
                    ln[res] = t + 1
            p_sym[t], p_sc[t] = cur, cur_sc
        o = order(s)
        sym[b], steps[b] = p_sym[:, o].t(), p_sc[:, o].t()
        scores[b], lengths[b] = s[o], torch.tensor(ln)[o]
    return sym, scores, lengths, steps


def replay_with(step, state, B, k, C, L, eos=0):
    """the search with the decoder step from a callback: step(state [B*k,...], y_prev long [B*k]) -> (logits [B*k,C] (any
    float dtype / device), state'); states are gathered with index_select on the state's own device.
    -> dict: symbols, scores, lengths, step_scores (see backtrack), sel_gap [B], score_gap [B], tables (sc, pr, sy)."""
    run = torch.full((B, k), -math.inf, dtype=torch.float64)
    run[:, 0] = 0.0
    y_prev = torch.zeros((B * k,), dtype=torch.long)
    sc = torch.zeros((L, B, k), dtype=torch.float64)
    pr = torch.zeros((L, B, k), dtype=torch.long)
    sy = torch.zeros((L, B, k), dtype=torch.long)
    sel_gap = torch.full((B,), math.inf, dtype=torch.float64)
    for t in range(L):
        logits, state = step(state, y_prev)
        cand = (run.view(B, k, 1) + torch.log_softmax(logits.detach().cpu().double().view(B, k, C), dim=2)).view(B, k * C)
        for b in range(B):
            o = order(cand[b])
            sel = o[:k]
            sc[t, b], pr[t, b], sy[t, b] = cand[b][sel], sel // C, sel % C
            if k < k * C:
                last, nxt = float(cand[b][o[k - 1]]), float(cand[b][o[k]])
                if nxt > -math.inf:
                    sel_gap[b] = min(float(sel_gap[b]), last - nxt)
        flat = (pr[t] + torch.arange(B).view(B, 1) * k).view(-1)
        state = state.index_select(0, flat.to(state.device))
        y_prev = sy[t].reshape(-1).clone()
        run = sc[t].masked_fill(sy[t] == eos, -math.inf)
    sym, scores, lengths, steps = backtrack(sc, pr, sy, eos)
    score_gap = torch.full((B,), math.inf, dtype=torch.float64)
    for b in range(B):
        for i in range(k - 1):
            # an exact tie of two identical hypotheses is no near-tie: a sequence that ends at the last step is both a last-step
            # beam and an ended sequence (the reference lists it twice), from ONE table entry - equal in every arithmetic
            same = (scores[b, i] == scores[b, i + 1] and lengths[b, i] == lengths[b, i + 1]
                    and torch.equal(sym[b, i, :lengths[b, i]], sym[b, i + 1, :lengths[b, i]]))
            if scores[b, i + 1] > -math.inf and not same:
                score_gap[b] = min(float(score_gap[b]), float(scores[b, i] - scores[b, i + 1]))
    return {"symbols": sym, "scores": scores, "lengths": lengths, "step_scores": steps, "sel_gap": sel_gap, "score_gap": score_gap,
            "tables": (sc, pr, sy)}


def replay(sd, x, k, C, L, eos=0):
    """the search in float64 from the state-dict weights: x [B,T,D] float32"""
    B = x.shape[0]
    f = f64_step(sd, x, xproj_f64(sd, x))
    item = torch.arange(B).repeat_interleave(k)
    return replay_with(lambda state, y: f(state, y, item), torch.zeros((B * k, 256), dtype=torch.float64), B, k, C, L, eos)


def path_rows(symbols, step_scores, length, score, C):
    """path rows [L,C] of ONE hypothesis: row t < length is zero except exp(score_t - score_{t-1}) (score_{-1} = 0) at
    symbols[t]; rows t >= length, and every row of a hypothesis whose score is -inf, are zero"""
    L = len(symbols)
    rows = np.zeros((L, C), dtype=np.float64)
    if not float(score) > -math.inf:
        return rows
    prev = 0.0
    for t in range(int(length)):
        rows[t, int(symbols[t])] = math.exp(float(step_scores[t]) - prev)
        prev = float(step_scores[t])
    return rows
