"""Inputs of tests/test_gpu_recognition_edges.py, built on the CPU (no GPU needed: the seeds below were picked by running
this module alone), with their float64 references (tests/recognition_ref.py) and the error of the fp32 evaluation of the same
formulas on the very same inputs - the figure each GPU bound is derived from:

    bound = min(max(4 x fp32 error, 1e-6), the project's bound of the stage)

4 x covers another summation order (MFMA tiles, wavefront trees) and the hardware exp / rcp (2e-7 absolute); the floor is a few
fp32 roundings of an O(1) value; the project's bounds are 1e-4 for BiLSTM / decoder outputs and 1e-3 elsewhere."""
import functools

import torch

import recognition_ref as RR

F32 = torch.float32
FLOOR = 1e-6


def bound(err32, project):
    return min(max(4.0 * err32, FLOOR), project)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ================================================================================================ fusion attention
FUSION_KINDS = ("randn", "peaked", "uniform_head", "flat_hid")
FUSION_PROJECT_BOUND = 1e-3


def fusion_weights(seed, flat_b1=False):
    g = _gen(seed)
    r = lambda *s: torch.randn(s, generator=g)
    w = {"w_mask": r(64) * 0.2, "b_mask": r(1) * 0.1, "w1": r(256, 512) / 16, "b1": r(256) * 0.1, "ln_g": 1 + r(256) * 0.3,
         "ln_b": r(256) * 0.1, "w2": r(512, 256) / 11, "b2": r(512) * 0.1}
    if flat_b1:
        w["b1"] = torch.full((256,), 0.3)
    return w


def _fusion_ref(x, w, dtype=RR.F64):
    return RR.gc_attention(x, w["w_mask"], w["b_mask"], w["w1"], w["b1"], w["ln_g"], w["ln_b"], w["w2"], w["b2"], dtype=dtype)


@functools.lru_cache(maxsize=None)
def fusion_case(kind, R):
    """-> dict x [R, 256, 512] float32, w, want (float64), mid (float64 intermediates), err32.
    peaked:       the slab scaled so that the largest mask logit is 60 in magnitude (near one-hot softmax over positions)
    uniform_head: heads 2 and 5 (one in each channel half the kernel's lanes split) hold the same vector at all 256
                  positions: equal logits, softmax exactly 1/256
    flat_hid:     b1 constant and the slab scaled so that the variance of hid is ~1e-5, the LayerNorm's epsilon"""
    seed = 40 + FUSION_KINDS.index(kind) * 10 + R
    w = fusion_weights(seed, flat_b1=kind == "flat_hid")
    x = torch.randn((R, 256, 512), generator=_gen(seed + 1))
    if kind == "peaked":
        x = x * (60.0 / float(_fusion_ref(x, w)[1]["logit"].abs().max()))
    elif kind == "uniform_head":
        for h in (2, 5):
            x[:, :, 64 * h:64 * h + 64] = x[:, :1, 64 * h:64 * h + 64]
    elif kind == "flat_hid":
        x = x * 0.04
        for _ in range(2):
            hid = _fusion_ref(x, w)[1]["hid"]
            x = x * float(torch.sqrt(1e-5 / hid.var(1, unbiased=False).mean()))
    x = x.contiguous()
    want, mid = _fusion_ref(x, w)
    err32 = float((_fusion_ref(x, w, F32)[0].double() - want).abs().max())
    return {"x": x, "w": w, "want": want, "mid": mid, "err32": err32}


# ================================================================================================ BiLSTM recurrence
LSTM_SHAPES = ((1, 1), (1, 2), (17, 3), (16, 32), (33, 32))
LSTM_KINDS = ("s1.5", "s30", "grow", "mean")
LSTM_PROJECT_BOUND = 1e-4


def lstm_whh(seed=7):
    return (torch.randn((2, 1024, 256), generator=_gen(seed)) * 0.08).contiguous()


@functools.lru_cache(maxsize=None)
def lstm_case(R, T, kind):
    """xg [R, T, 2, 1024] gate pre-activations (i, f, g, o):
    s1.5: randn x 1.5 (the scale of the existing tests);  s30: randn x 30, every gate saturated;
    grow: input and forget gates pushed to +8 and the candidate to +3, so c grows by ~1 per step towards T and tanh(c) saturates;
    mean: randn x 1.5 + 0.7, a nonzero mean"""
    seed = 500 + 37 * R + T + 1000 * LSTM_KINDS.index(kind)
    xg = torch.randn((R, T, 2, 1024), generator=_gen(seed))
    if kind == "s30":
        xg = xg * 30
    elif kind == "grow":
        xg = xg * 0.5
        xg[..., 0:512] += 8.0
        xg[..., 512:768] += 3.0
    else:
        xg = xg * 1.5 + (0.7 if kind == "mean" else 0.0)
    xg = xg.contiguous()
    whh = lstm_whh()
    want = RR.bilstm(xg, whh)
    err32 = float((RR.bilstm(xg, whh, dtype=F32).double() - want).abs().max())
    cmax = max(float(RR.lstm_direction(xg[:, :, d], whh[d], bool(d))[1].abs().max()) for d in (0, 1))
    return {"xg": xg, "whh": whh, "want": want, "err32": err32, "cmax": cmax}


# ================================================================================================ decoder step
# (T, C, R): every T in {1, 2, 15, 16, 17, 32, 33, 63, 64}, every C in {1, 2, 63, 64, 65, 97, 128, 129, 255, 256}, R in {1, 5, 17}
STEP_SHAPES = ((1, 1, 1), (2, 2, 5), (15, 63, 17), (16, 64, 1), (17, 65, 5), (32, 97, 17), (33, 128, 1), (63, 129, 5),
               (64, 255, 17), (64, 256, 5))
STEP_KINDS = ("plain", "y_edges", "h_saturating", "logits80", "temperature")
STEP_VARIANT_SHAPES = ((17, 65, 5), (32, 97, 17), (64, 256, 5))
STEP_TAIL_SHAPES = ((8, 97, 513), (8, 97, 1027))        # dec_fc_att_kernel<2> with nr = 1 in the last workgroup, <4> with nr = 3
DEC_PROJECT_BOUND = 1e-4


@functools.lru_cache(maxsize=None)
def step_case(T, C, R, kind="plain"):
    """teacher-forced inputs of ONE decoder step: x, xproj [R, T, 256], h [R, 256], y_prev [R]
    y_edges:      y_prev cycles through 0, C - 1, -1 (clamped to 0), C (clamped to C - 1)
    h_saturating: h x 24: |sEmbed(h) + xproj| is above 9 for about half of the elements, where 1 - tanh is below one fp32 rounding
                  and tanh_fast must saturate cleanly (exp(2x) up to inf)
    logits80:     fc weight and bias scaled so that the largest logit is 80 in magnitude
    temperature:  0.6"""
    seed = 7000 + 13 * T + 3 * C + R + 100000 * STEP_KINDS.index(kind)
    plain = RR.make_decoder_plain(C, seed, temperature=0.6 if kind == "temperature" else 1.0)
    g = _gen(seed + 1)
    x = torch.randn((R, T, 256), generator=g)
    h = torch.tanh(torch.randn((R, 256), generator=g))
    y = torch.randint(0, C, (R,), generator=g, dtype=torch.int32)
    if kind == "y_edges":
        y = torch.tensor([0, C - 1, -1, C], dtype=torch.int32).repeat(R // 4 + 1)[:R].contiguous()
    if kind == "h_saturating":
        h = h * 24
    xp = RR.xproj_of(x, plain)
    if kind == "logits80":
        s = 80.0 / float(RR.decoder_step(x, xp, h, y, plain)[0].abs().max())
        plain["fcW"], plain["fcB"] = plain["fcW"] * s, plain["fcB"] * s
    want = RR.decoder_step(x, xp, h, y, plain)
    got32 = RR.decoder_step(x, xp, h, y, plain, dtype=F32)
    err32 = [float((a.double() - b).abs().max()) for a, b in zip(got32, want)]
    return {"x": x, "xproj": xp, "h": h.contiguous(), "y": y, "plain": plain, "want": want, "err32": err32,
            "sat": float(((h.double() @ plain["sW"].double().t() + plain["sB"].double()).unsqueeze(1) + xp.double()).abs().gt(9).double().mean())}


# ================================================================================================ greedy decode
# (T, C, max_len, tie): tie = None | (a, b): fc rows and biases of classes a and b are identical (bit-equal probabilities, the
# first index must win; 3 and 70 sit in different 64-lane slots of the soft-max wavefront) | "uniform": fc weight zero and the
# bias constant, every class of every row equal, arg-max 0.  GREEDY_SEED was checked on the CPU: with it the float64 reference's gap
# between the winning tie group and the best class outside it exceeds GREEDY_GAP at every live step of every RoI of every case
# (the smallest is 5.3e-4), and the constructed ties win 25, 56 and 9 live steps of their cases.
GREEDY_BOTH = ((32, 97, 26, None), (32, 97, 26, (3, 70)), (32, 128, 26, (5, 9)), (7, 40, 3, None), (7, 40, 3, "uniform"), (1, 2, 1, None),
               (32, 97, 1, None), (32, 97, 2, None))
GREEDY_STEP_ONLY = ((33, 97, 26, None), (64, 256, 5, (3, 70)), (32, 129, 4, None))
GREEDY_GAP = 1e-4
GREEDY_POOL = 96
GREEDY_SEED = 0
TIE_BUMP = 4.0


def _greedy_plain(C, seed, tie):
    plain = RR.make_decoder_plain(C, seed)
    if tie == "uniform":
        plain["fcW"] = torch.zeros_like(plain["fcW"])
        plain["fcB"] = torch.full_like(plain["fcB"], 0.25)
    elif tie is not None:
        a, b = tie
        plain["fcW"][a] = plain["fcW"][b]
        plain["fcB"][a] = plain["fcB"][b] = float(plain["fcB"].max()) + TIE_BUMP
    return plain


@functools.lru_cache(maxsize=None)
def greedy_case(T, C, L, tie):
    """R <= 40 RoIs in three images, drawn from a pool of GREEDY_POOL random RoIs decoded one by one in float64: eos = the class
    the pool emits most often in its first two steps; image 0 = RoIs that emit eos within those steps (the image breaks early and
    its later rows are zero), image 2 holds a RoI that never emits eos (the image never breaks), image 1 = the next of the pool."""
    seed = GREEDY_SEED
    plain = _greedy_plain(C, 9000 + seed, tie)
    pool = torch.randn((GREEDY_POOL, T, 256), generator=_gen(9500 + seed))
    one = RR.greedy_decode(pool, RR.xproj_of(pool, plain), plain, torch.arange(GREEDY_POOL), L, eos=-1)["pred"]
    head = one[:, :min(2, L)]
    if tie == "uniform":
        eos, early, never = 1, [], [0, 1, 2]                          # every row emits 0: nothing ever breaks
    else:
        eos = int(torch.bincount(head.reshape(-1), minlength=C).argmax())
        early = [i for i in range(GREEDY_POOL) if bool((head[i] == eos).any())][:6]
        never = [i for i in range(GREEDY_POOL) if not bool((one[i] == eos).any())][:3]
    used = set(early) | set(never)
    rest = [i for i in range(GREEDY_POOL) if i not in used]
    n1 = 37 - len(early) - len(never) - 10
    img1, img2 = rest[:n1], never + rest[n1:n1 + 10]
    idx = early + img1 + img2
    roi_image = torch.tensor([0] * len(early) + [1] * len(img1) + [2] * len(img2), dtype=torch.int32)
    x = pool[idx].contiguous()
    xp = RR.xproj_of(x, plain)
    want = RR.greedy_decode(x, xp, plain, roi_image, L, eos)
    got32 = RR.greedy_decode(x, xp, plain, roi_image, L, eos, dtype=F32)
    same_path = torch.equal(got32["pred"], want["pred"])
    err32 = float((got32["probs"].double() - want["probs"]).abs().max())
    return {"x": x, "xproj": xp, "plain": plain, "roi_image": roi_image, "eos": eos, "want": want, "err32": err32,
            "same_path32": same_path, "n_early": len(early), "n_never": len(never), "seed": seed}


# ================================================================================================ non-finite contract
POISONS = {"nan": float("nan"), "inf": float("inf"), "1e30": 1e30}
POISON_R, POISON_ROI = 20, 5
POISON_IMAGES = [0] * 5 + [1] + [2] * 14             # the poisoned RoI is alone in its image
