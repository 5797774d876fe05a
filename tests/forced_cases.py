"""Forced decoding of the attention decoder (the emitted symbols given, not chosen) restated in float64 on the CPU, and the
generated cases of the forced-decoding tests.

`forced_f64` runs `beam_cases.f64_step` (DecoderUnit.forward, reference prediction_aster.py:291-302, from the state-dict
weights) on n sequences per item: state zero, y_prev = 0 at step 0 and targets[t-1] after it, float64 log-softmax, the
records of step t < length, zeros from the length on.  The length of a sequence is `lengths` where given, else the position
of its first <eos> plus one, else L.

`case_data(case)` builds, once per case of `beam_cases.CASES` (the smallest shapes that cross the kernels' boundaries: B 1 / 3
/ 17, every row blocking n 1, 2, 3 -> 4, 4, 5 -> 8, 16, T 7 / 32 / 64, L 1 / 26 / 64, C 5 / 97 / 256, 512 state rows), the inputs and three
target sets with their float64 results:
  "hyp"      (a) the k hypotheses and lengths of the float64 beam search `beam_cases.replay`;
  "perturb"  (b) seeded perturbations of them, lengths left to the first <eos>: per sequence, in turn, one symbol below the
             length replaced by another class, the stop removed (every <eos> replaced: the sequence runs all L steps), a stop
             put at step 0, and the hypothesis unchanged;
  "lengths"  (c) the hypotheses' symbols with explicit seeded lengths in 0..L that include 0 and L.
Nothing here is changed after it was built: the tests share it.
"""
import numpy as np
import torch

import beam_cases as BC

SETS = ("hyp", "perturb", "lengths")


def effective_lengths(targets, lengths, eos):
    """targets [B,n,L] long, lengths [B,n] long or None -> [B,n] long"""
    B, n, L = targets.shape
    if lengths is not None:
        return lengths.clamp(0, L).clone()
    is_eos = targets == eos
    first = torch.where(is_eos.any(2), is_eos.int().argmax(2) + 1, torch.full((B, n), L))
    return first.long()


def forced_f64(sd, x, targets, lengths=None, eos=0):
    """x [B,T,D] float32, targets [B,n,L] long in [0,C), lengths [B,n] or None -> dict of float64 / long tensors: step_logp
    [B,n,L], scores [B,n] (sum over t < length), lengths [B,n], probs and logits [B,n,L,C] (zero from the length on)"""
    B, n, L = targets.shape
    step = BC.f64_step(sd, x, BC.xproj_f64(sd, x))
    item = torch.arange(B).repeat_interleave(n)
    ln = effective_lengths(targets, lengths, eos)
    state = torch.zeros((B * n, 256), dtype=torch.float64)
    y_prev = torch.zeros((B * n,), dtype=torch.long)
    tg = targets.reshape(B * n, L)
    out_lp, out_p, out_l = [], [], []
    for t in range(L):
        logits, state = step(state, y_prev, item)
        lsm = torch.log_softmax(logits, dim=1)
        live = (t < ln.reshape(-1))
        out_lp.append(torch.where(live, lsm.gather(1, tg[:, t:t + 1]).squeeze(1), torch.zeros(())))
        out_p.append(torch.where(live[:, None], lsm.exp(), torch.zeros(())))
        out_l.append(torch.where(live[:, None], logits, torch.zeros(())))
        y_prev = tg[:, t]
    C = out_p[0].shape[1]
    step_logp = torch.stack(out_lp, 1).view(B, n, L)
    return {"step_logp": step_logp, "scores": step_logp.sum(2), "lengths": ln,
            "probs": torch.stack(out_p, 1).view(B, n, L, C), "logits": torch.stack(out_l, 1).view(B, n, L, C)}


def perturb(symbols, lengths, C, eos, seed):
    """set (b): symbols [B,n,L] long, lengths [B,n] of the hypotheses -> perturbed targets [B,n,L] (lengths: first <eos>)"""
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    B, n, L = symbols.shape
    out = symbols.clone()
    other = [c for c in range(C) if c != eos]

    def pick(avoid):
        c = int(torch.randint(0, C, (1,), generator=g))
        return c if c != avoid else (c + 1) % C
    for i in range(B * n):
        b, j = divmod(i, n)
        kind = i % 4
        if kind == 0:                                   # one symbol replaced
            t = int(torch.randint(0, max(int(lengths[b, j]), 1), (1,), generator=g))
            out[b, j, t] = pick(int(out[b, j, t]))
        elif kind == 1 and other:                       # the stop removed
            for t in range(L):
                if int(out[b, j, t]) == eos:
                    out[b, j, t] = other[int(torch.randint(0, len(other), (1,), generator=g))]
        elif kind == 2:                                 # a stop at step 0
            out[b, j, 0] = eos
    return out


def seeded_lengths(B, n, L, seed):
    """set (c): lengths [B,n] in 0..L that include 0 and L (a single sequence: L)"""
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    ln = torch.randint(0, L + 1, (B * n,), generator=g)
    ln[-1] = L
    if B * n > 1:
        ln[0] = 0
    return ln.view(B, n)


_DATA = {}


def case_data(case, eos=0):
    """-> dict: sd, x [B,T,D] float32 (CPU), replay (beam_cases.replay), sets {name: (targets long [B,n,L], lengths | None)},
    f64 {name: forced_f64 result}"""
    if case[0] not in _DATA:
        name, B, k, T, L, C, seed = case
        sd = BC.decoder_sd(C, eos=eos)
        x = BC.rand_x(B, T, seed)
        rep = BC.replay(sd, x, k, C, L, eos)
        sym, ln = rep["symbols"], rep["lengths"]
        sets = {"hyp": (sym, ln), "perturb": (perturb(sym, ln, C, eos, seed + 1000), None),
                "lengths": (sym, seeded_lengths(B, k, L, seed + 2000))}
        f64 = {s: forced_f64(sd, x, t, l, eos) for s, (t, l) in sets.items()}
        _DATA[case[0]] = {"sd": sd, "x": x, "replay": rep, "sets": sets, "f64": f64}
    return _DATA[case[0]]


def f32_sequential_sum(step_logp, lengths):
    """the contract of out_scores: fl32(score_{t-1} + step_logp[t]) in step order from 0 over t < length, numpy float32"""
    lp = np.asarray(step_logp, dtype=np.float32)
    ln = np.asarray(lengths)
    out = np.zeros(ln.shape, dtype=np.float32)
    for idx in np.ndindex(*ln.shape):
        s = np.float32(0.0)
        for t in range(int(ln[idx])):
            s = np.float32(s + lp[idx + (t,)])
        out[idx] = s
    return out
