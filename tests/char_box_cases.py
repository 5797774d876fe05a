"""Cases and checkers of the character boxes (include/glass_hip_feature_chars.h), shared by tests/test_char_boxes.py (CPU) and
tests/test_gpu_char_boxes.py.

  * `reference`: an independent plain-Python checker of the spans - per-step loops, `fractions.Fraction` for the sums, the
    centres and the boundaries, so that on attention given as dyadic rationals (every float32 is one) the centres, the
    boundaries, the count and the three flags are EXACT; only the square root of the spread is taken in float64.
  * `all_cases`: the hand cases and the seeded ones.  A seeded case is kept only if all consecutive centres differ by at least
    1e-9, so no `monotone` flag hangs on a rounding; `SEEDS_TRIED` / `SEEDS_REJECTED` count them.
  * `forced_attention_f64`: the float64 forced replay of tests/forced_cases.py::forced_f64 (the same step arithmetic, spelt out
    here because the step of beam_cases.py does not return its attention weights) with the rows it attends by.
"""
import math
from fractions import Fraction

import numpy as np
import torch

import beam_cases as BC
import forced_cases as FC

EOS = 1
INT_FIELDS = ("count", "monotone", "valid")
MIN_GAP = 1e-9


def reference(attention, targets, lengths, eos):
    """attention float32 [R,L,T], targets [R,L], lengths [R] -> {"spans", "centres" (Fractions), "spreads" (floats), "count",
    "monotone", "valid", "min_gap"}: lists per word, rows up to L (zeros from the count on)"""
    att = np.asarray(attention, dtype=np.float32)
    R, L, T = att.shape
    out = {k: [] for k in ("spans", "centres", "spreads", "count", "monotone", "valid")}
    min_gap = math.inf
    for r in range(R):
        n = int(lengths[r])
        n = 0 if n < 0 else L if n > L else n
        m = n
        if n > 0 and int(targets[r][n - 1]) == eos:
            m = n - 1
        cen, spr, ok = [], [], True
        for t in range(m):
            row = [float(v) for v in att[r, t]]
            if any((not math.isfinite(v)) or v < 0.0 for v in row):
                ok = False
                break
            fr = [Fraction(v) for v in row]
            S = Fraction(0)
            for v in fr:
                S += v
            if S <= 0:
                ok = False
                break
            num = Fraction(0)
            for j, v in enumerate(fr):
                num += v * Fraction(2 * j + 1, 2 * T)
            c = num / S
            var = Fraction(0)
            for j, v in enumerate(fr):
                var += v * (Fraction(2 * j + 1, 2 * T) - c) ** 2
            cen.append(c)
            spr.append(math.sqrt(float(var / S)))
        zero = Fraction(0)
        if not ok:
            out["spans"].append([(zero, zero)] * L); out["centres"].append([zero] * L); out["spreads"].append([0.0] * L)
            out["count"].append(0); out["monotone"].append(0); out["valid"].append(0)
            continue
        mono = 1
        for t in range(m - 1):
            if not cen[t + 1] > cen[t]:
                mono = 0
            min_gap = min(min_gap, abs(float(cen[t + 1] - cen[t])))
        spans = []
        for t in range(m):
            if m == 1:
                spans.append((Fraction(0), Fraction(1)))
                continue
            if t == 0:
                b0 = (cen[0] + cen[1]) / 2
                left = min(max(cen[0] - abs(b0 - cen[0]), Fraction(0)), Fraction(1))
            else:
                left = (cen[t - 1] + cen[t]) / 2
            if t == m - 1:
                bl = (cen[m - 2] + cen[m - 1]) / 2
                right = min(max(cen[m - 1] + abs(cen[m - 1] - bl), Fraction(0)), Fraction(1))
            else:
                right = (cen[t] + cen[t + 1]) / 2
            spans.append((min(left, right), max(left, right)))
        pad = L - m
        out["spans"].append(spans + [(zero, zero)] * pad); out["centres"].append(cen + [zero] * pad)
        out["spreads"].append(spr + [0.0] * pad)
        out["count"].append(m); out["monotone"].append(mono); out["valid"].append(1)
    out["min_gap"] = min_gap
    return out


def ulps32(a, b):
    """distance of two float32 arrays in units in the last place, elementwise (both finite; +0 and -0 are 0 apart)"""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7fffffff), ia)
    ib = np.where(ib < 0, -(ib & 0x7fffffff), ib)
    return np.abs(ia - ib)


def f32(x):
    """a Fraction or float rounded to float32 through its correctly rounded float64"""
    return np.float32(float(x))


# ---------------------------------------------------------------------- cases
def _onehot(T, cols, scale=1.0):
    a = np.zeros((len(cols), T), dtype=np.float32)
    for t, j in enumerate(cols):
        a[t, j] = scale
    return a


def _word(rows, L, symbols=None, stop=True, length=None):
    """rows [m,T] -> (attention [L,T], targets [L], length): m character steps, then (with `stop`) the stop symbol"""
    m, T = rows.shape
    att = np.zeros((L, T), dtype=np.float32)
    att[:m] = rows
    tg = np.full((L,), 5, dtype=np.int32)
    if symbols is not None:
        tg[:m] = symbols
    n = m
    if stop and m < L:
        tg[m] = EOS
        att[m, :] = 1.0 / T                      # the stop's own attention row: never read
        n = m + 1
    return att, tg, n if length is None else length


def _batch(words):
    return (np.stack([w[0] for w in words]), np.stack([w[1] for w in words]), np.asarray([w[2] for w in words], dtype=np.int32))


def hand_cases():
    """[(name, attention, targets, lengths)]"""
    cases = []
    L, T = 8, 16
    cases.append(("one-hot rows", *_batch([_word(_onehot(T, [1, 4, 9, 15]), L)])))
    two = np.zeros((2, T), dtype=np.float32); two[0, [2, 6]] = 0.5; two[1, [8, 12]] = 0.25
    cases.append(("two equal peaks", *_batch([_word(two, L)])))
    cases.append(("a uniform row", *_batch([_word(np.full((3, T), 1.0 / T, dtype=np.float32) * np.array([[1], [2], [0.5]], dtype=np.float32), L)])))
    cases.append(("a non-monotone word", *_batch([_word(_onehot(T, [3, 10, 6, 12]), L)])))
    cases.append(("two steps with the same centre", *_batch([_word(_onehot(T, [3, 7, 7, 12]), L), _word(_onehot(T, [7, 7]), L)])))
    cases.append(("m = 0, 1, 2, L", *_batch([_word(_onehot(T, []), L), _word(_onehot(T, [5]), L), _word(_onehot(T, [5, 9]), L),
                                             _word(_onehot(T, list(range(0, 16, 2))), L)])))
    cases.append(("a word without a stop symbol", *_batch([_word(_onehot(T, [2, 5, 8]), L, stop=False)])))
    cases.append(("the stop at step 0", *_batch([_word(_onehot(T, []), L), _word(_onehot(T, [4, 8]), L)])))
    cases.append(("lengths outside 0..L", *_batch([_word(_onehot(T, [1, 2, 3]), L, length=-3),
                                                   _word(_onehot(T, list(range(8))), L, stop=False, length=L + 7)])))
    cases.append(("edges mirrored beyond the box", *_batch([_word(_onehot(T, [0, 15]), L), _word(_onehot(T, [15, 0]), L)])))
    for t_ in (1, 2, 63, 64):
        g = np.random.RandomState(t_)
        rows = (g.randint(0, 1 << 12, size=(5, t_)).astype(np.float32) + 1.0) / float(1 << 12)
        cases.append((f"T = {t_}", *_batch([_word(rows, L), _word(_onehot(t_, [0, t_ - 1, t_ // 2]), L)])))
    bad = []
    for k, poison in enumerate((np.nan, -0.25, np.inf, None)):
        rows = _onehot(T, [2, 6, 11])
        if poison is None:
            rows[1, :] = 0.0                                             # an all-zero row
        else:
            rows[1, 3] = poison
        bad += [_word(_onehot(T, [1 + k, 9]), L), _word(rows, L)]
    bad.append(_word(_onehot(T, [4, 12]), L))
    cases.append(("a NaN, a negative, an infinite and an all-zero row", *_batch(bad)))
    junk = _word(_onehot(T, [2, 9]), L)
    junk[0][4:] = np.nan                                                 # rows beyond the count are never read
    cases.append(("poison beyond the count", *_batch([junk])))
    return cases


SEEDS = list(range(20))
SEEDS_TRIED = SEEDS_REJECTED = 0
_ALL = None


def seeded_case(seed):
    g = np.random.RandomState(1000 + seed)
    R = (1, 63, 64, 65)[seed] if seed < 4 else int(g.randint(2, 40))
    L, T = (26, 64, 1, 2)[seed % 4], (32, 64, 7, 13)[(seed // 2) % 4]        # (T = 1 has one centre only: a hand case)
    att = np.zeros((R, L, T), dtype=np.float32)
    tg = g.randint(2, 90, size=(R, L)).astype(np.int32)
    ln = np.zeros((R,), dtype=np.int32)
    for r in range(R):
        m = int(g.randint(0, L + 1))
        # a peak that walks along the box with some noise and jitter, as dyadic rationals k / 2^12
        pos = np.sort(g.uniform(0, T, size=m)) if g.rand() < 0.8 else g.uniform(0, T, size=m)
        j = np.arange(T)[None, :]
        rows = np.exp(-0.5 * ((j - pos[:, None]) / g.uniform(0.6, 3.0)) ** 2) + 0.02 * g.rand(m, T)
        rows = rows / rows.sum(1, keepdims=True)
        att[r, :m] = np.floor(rows * 4096.0 + 1.0) / 4096.0
        if m < L and g.rand() < 0.8:
            tg[r, m] = EOS
            att[r, m] = 1.0 / T
            ln[r] = m + 1
        else:
            ln[r] = m
    return f"seed {seed}", att, tg, ln


def all_cases():
    """[(name, attention, targets, lengths, reference)] - built once"""
    global _ALL, SEEDS_TRIED, SEEDS_REJECTED
    if _ALL is None:
        out = [(n, a, t, ln, reference(a, t, ln, EOS)) for n, a, t, ln in hand_cases()]
        for seed in SEEDS:
            n, a, t, ln = seeded_case(seed)
            ref = reference(a, t, ln, EOS)
            SEEDS_TRIED += 1
            if ref["min_gap"] < MIN_GAP:
                SEEDS_REJECTED += 1
                continue
            out.append((n, a, t, ln, ref))
        _ALL = out
    return _ALL


def assert_matches_reference(got, ref, name, L):
    """host or device result (numpy arrays) against the exact reference: integers exact, floats within one float32 ulp"""
    for k in INT_FIELDS:
        assert got[k].dtype == np.int32 and got[k].tolist() == ref[k], (name, k, got[k].tolist(), ref[k])
    want_sp = np.array([[[f32(lo), f32(hi)] for lo, hi in w] for w in ref["spans"]], dtype=np.float32).reshape(-1, L, 2)
    want_c = np.array([[f32(c) for c in w] for w in ref["centres"]], dtype=np.float32).reshape(-1, L)
    want_s = np.array(ref["spreads"], dtype=np.float32).reshape(-1, L)
    worst = 0
    for k, want in (("spans", want_sp), ("centres", want_c), ("spreads", want_s)):
        assert got[k].dtype == np.float32 and got[k].shape == want.shape, (name, k)
        assert np.all(np.isfinite(got[k])), (name, k)
        d = int(ulps32(got[k], want).max()) if want.size else 0
        worst = max(worst, d)
        assert d <= 1, (name, k, d)
    return worst


def assert_same(got, want, name):
    """device result against the host statement on the same rows: integers exact, floats within one float32 ulp"""
    worst = 0
    for k in INT_FIELDS:
        assert np.array_equal(got[k], want[k]), (name, k)
    for k in ("spans", "centres", "spreads"):
        assert got[k].shape == want[k].shape and np.all(np.isfinite(got[k])), (name, k)
        d = int(ulps32(got[k], want[k]).max()) if want[k].size else 0
        worst = max(worst, d)
        assert d <= 1, (name, k, d)
    return worst


# ---------------------------------------------------------------------- the float64 replay with its attention rows
def forced_attention_f64(sd, x, targets, lengths=None, eos=0):
    """tests/forced_cases.py::forced_f64 with the attention rows: x [B,T,D] float32, targets [B,n,L] long in [0,C), lengths
    [B,n] or None -> float64 attention [B,n,L,T]: row t = the softmax that formed the context of step t (the GRU input of
    step t is [emb(y_{t-1}) | alpha_t . x], y_{-1} = 0), zero from the effective length on.  The step is beam_cases.f64_step's
    arithmetic, line for line."""
    B, n, L = targets.shape
    T = x.shape[1]
    Q = BC.Q
    w = {k: sd[Q + k].double() for k in ("attention_unit.sEmbed.weight", "attention_unit.sEmbed.bias", "attention_unit.wEmbed.weight",
                                         "attention_unit.wEmbed.bias", "tgt_embedding.weight", "gru.weight_ih_l0", "gru.weight_hh_l0",
                                         "gru.bias_ih_l0", "gru.bias_hh_l0")}
    xd, xproj = x.double(), BC.xproj_f64(sd, x)
    item = torch.arange(B).repeat_interleave(n)
    ln = FC.effective_lengths(targets, lengths, eos).reshape(-1)
    state = torch.zeros((B * n, 256), dtype=torch.float64)
    y_prev = torch.zeros((B * n,), dtype=torch.long)
    tg = targets.reshape(B * n, L)
    rows = []
    for t in range(L):
        sp = state @ w["attention_unit.sEmbed.weight"].t() + w["attention_unit.sEmbed.bias"]
        e = torch.tanh(sp[:, None, :] + xproj[item]) @ w["attention_unit.wEmbed.weight"].reshape(-1) + w["attention_unit.wEmbed.bias"]
        alpha = torch.softmax(e, dim=1)
        rows.append(torch.where((t < ln)[:, None], alpha, torch.zeros((), dtype=torch.float64)))
        ctx = (alpha[:, :, None] * xd[item]).sum(1)
        inp = torch.cat([w["tgt_embedding.weight"][y_prev], ctx], 1)
        gi = inp @ w["gru.weight_ih_l0"].t() + w["gru.bias_ih_l0"]
        gh = state @ w["gru.weight_hh_l0"].t() + w["gru.bias_hh_l0"]
        i_r, i_z, i_n = gi.chunk(3, 1)
        h_r, h_z, h_n = gh.chunk(3, 1)
        r, z = torch.sigmoid(i_r + h_r), torch.sigmoid(i_z + h_z)
        state = (1.0 - z) * torch.tanh(i_n + r * h_n) + z * state
        y_prev = tg[:, t]
    return torch.stack(rows, 1).view(B, n, L, T)
