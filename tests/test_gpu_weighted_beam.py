"""GPU: the weighted-pattern device beam search (glass_beam_search_wdfa, ASTER_V2.beam_decode(pattern=WeightedPattern,
weight_scale=...), RecognizerRCNNHeadV3.set_pattern(..., weight_scale), MODEL.ROI_RECOGNIZER_HEAD.DECODE_LENGTH_BONUS,
inference_on_dataset(pattern=...)): bit-equal to the unweighted search with zero weights or scale 0, against the float64 weighted
replay of tests/weighted_pattern_cases.py, against forced decoding, and through the head, the runner and the driver."""
import os
import re

import numpy as np
import pytest
import torch

import beam_cases as BC
import lexicon_beam_cases as LC
import pattern_cases as PC
import test_gpu_beam_search as G
import test_gpu_lexicon_beam as GL
import test_gpu_pattern_beam as GP
import weighted_pattern_cases as WC

pytestmark = pytest.mark.gpu

ROOT = LC.ROOT
# the constants of tests/test_gpu_beam_search.py, measured there for this step arithmetic
MARGIN, TOL = G.MARGIN, G.TOL
assert (MARGIN, TOL) == (WC.MARGIN, WC.TOL)
FIELDS = ("symbols", "scores", "lengths", "path_probs", "words", "model_scores")
_bits = GP._bits


def _arbitrary_lm():
    from glass_amd.evaluation.weighted_pattern import CharNgramLM
    return CharNgramLM.estimate(WC.MIX_WORDS + ["AB12", "-a", "B0"], order=2)


# ------------------------------------------------------------------ 1. no weight, no difference
@pytest.mark.parametrize("name", list(PC.CASES))
def test_zero_weights_and_zero_scale_are_bit_equal_to_the_unweighted_search(name):
    """all-zero weights, and arbitrary weights (a bigram model crossed with the pattern, a bonus) under weight_scale = 0:
    symbols, lengths, tags, model scores and path rows bit-equal to glass_beam_search_dfa, scores bit-equal to model_scores"""
    r = GP._run(name)
    d, want = r["d"], r["cpu"]
    zero = r["pat"].weighted()
    mixed = r["pat"].weighted(lm=_arbitrary_lm(), length_bonus=-0.37)
    empty = bool((r["pat"].start < 0).all())              # no start state: the product has the one state of an empty automaton
    assert not zero.weight64.any() and (mixed.weight64.any() or empty) and (mixed.num_states >= r["pat"].num_states or empty)
    for what, pat, scale in (("zero weights", zero, 1.0), ("scale 0", mixed, 0.0)):
        got = r["dec"].beam_decode(r["x"], d["k"], d["eos"], path_probs=True, pattern=pat, segments=r["seg"], weight_scale=scale)
        for n in ("symbols", "lengths", "path_probs", "words"):
            a, b = _bits(getattr(got, n)), _bits(want[n])
            assert a.dtype == b.dtype and torch.equal(a, b), (name, what, n)
        assert torch.equal(_bits(got.model_scores), _bits(want["scores"])), (name, what)
        assert torch.equal(_bits(got.scores), _bits(got.model_scores)), (name, what)


# ------------------------------------------------------------------ 2. weighted cases against the float64 replay
_RUNS = {}


def _run(name):
    if name not in _RUNS:
        d = WC.case_data(name)
        dec = G._decoder(d["sd"], d["C"], d["L"])
        x = d["x"].to(G._dev())
        base, pat = WC.build_pattern(d, G._dev())
        seg = torch.tensor(WC.item_segments(d), dtype=torch.int32).to(G._dev())      # a device tensor: passed through unchecked
        got = dec.beam_decode(x, d["k"], d["eos"], path_probs=True, pattern=pat, segments=seg, weight_scale=d["scale"])
        _RUNS[name] = dict(d=d, dec=dec, x=x, base=base, pat=pat, seg=seg, got=got, cpu={n: getattr(got, n).cpu() for n in FIELDS})
    return _RUNS[name]


def _fused_bound(d):
    """per hypothesis: TOL + the float32 accumulation bound of its fused score (weighted_pattern_cases.weight_bound)"""
    W = d["f64"]["W"].numpy()
    return TOL + 2.0 * (d["L"] + 1) * 2.0 ** -23 * np.maximum(1.0, W)


@pytest.mark.parametrize("name", list(WC.CASES))
def test_weighted_cases_against_the_float64_replay(name):
    """symbols, lengths and tags exact; model scores and path rows within TOL; fused scores within
    TOL + 2 (L + 1) 2^-23 max(1, W), W = the largest |scale * a| or |fused| along the hypothesis in the replay (the float32
    accumulation bound, derived and not tuned).  No item is excluded.
    Measured on an MI355X, per case: largest |d model score| | largest |d fused score| of the device search vs the float64 replay
    | smallest bound | states
      k1_lm_c13_l4          2.1e-6 | 1.9e-6 | 1.14e-4 | 7       trigram_ab_l5_k5      3.8e-6 | 3.4e-6 | 1.16e-4 | 7
      bonus_longest_l6_k4   1.0e-5 | 1.0e-5 | 1.15e-4 | 2       bonus_negative_l5_k3  4.8e-6 | 4.8e-6 | 1.10e-4 | 2
      priors_reverse_k3     3.3e-6 | 3.3e-6 | 1.27e-4 | 10      priors_twins_ci_k4    2.8e-6 | 2.8e-6 | 1.12e-4 | 5
      two_segments_start_w  3.2e-6 | 2.7e-6 | 1.20e-4 | 16      rows512_b32_k16       1.6e-5 | 1.7e-5 | 1.09e-4 | 73
      c256_identity         4.0e-6 | 4.2e-6 | 1.31e-4 | 11      t64                   1.8e-6 | 2.2e-6 | 1.13e-4 | 10
      l64_a63               7.7e-7 | 8.1e-7 | 2.05e-4 | 64      exhaustive_k4         3.8e-6 | 3.7e-6 | 1.14e-4 | 6"""
    r = _run(name)
    d, got = r["d"], r["cpu"]
    f64, B, k, L, C = d["f64"], d["B"], d["k"], d["L"], d["C"]
    fin = torch.isfinite(f64["scores"])
    dm = G._absdiff(got["model_scores"], f64["model_scores"])
    df = np.where(fin.numpy(), np.abs(got["scores"].double().numpy() - np.where(fin.numpy(), f64["scores"].numpy(), 0.0)), 0.0)
    bound = _fused_bound(d)
    print(f"[weighted] {name}: device vs float64 replay: model {dm:.3e}, fused {float(df.max()):.3e} (bound {float(bound[fin.numpy()].min()) if fin.any() else TOL:.3e}); "
          f"{r['pat'].num_states} states, F {r['pat'].num_fold}, {r['pat'].nbytes} bytes, built in {r['pat'].build_seconds:.3f} s")
    assert got["symbols"].shape == (B, k, L) and got["scores"].shape == got["model_scores"].shape == got["lengths"].shape == (B, k)
    assert got["path_probs"].shape == (B, L, C) and got["words"].dtype == torch.int32 and got["model_scores"].dtype == torch.float32
    assert torch.equal(got["symbols"].long(), f64["symbols"]), name
    assert torch.equal(got["lengths"].long(), f64["lengths"]), name
    for n in ("scores", "model_scores"):
        assert (torch.isneginf(got[n]) == ~fin).all() and not torch.isnan(got[n]).any(), n
    if d["lexicon"] is None:
        assert torch.equal(got["words"].long(), torch.where(fin, 0, -1)), "tags: 0 for a regex, -1 for an absent hypothesis"
    else:
        assert torch.equal(got["words"].long(), f64["words"]), "tags: the first word that ends at the state"
    assert dm < TOL
    assert (df <= bound).all(), (name, float(df.max()))
    for b in range(B):
        want = BC.path_rows(f64["symbols"][b, 0], f64["step_scores"][b, 0], f64["lengths"][b, 0], f64["model_scores"][b, 0], C)
        rows = got["path_probs"][b].double().numpy()
        assert ((rows != 0) == (want != 0)).all(), (name, b)
        assert float(np.abs(rows - want).max()) < TOL, (name, b)
        if fin[b, 0]:                       # the rows are the MODEL's conditional probabilities: their product is exp(model score)
            assert np.prod(rows[rows != 0]) == pytest.approx(np.exp(float(got["model_scores"][b, 0])), rel=1e-4)
    if name == "two_segments_start_w":
        assert not fin[2].any() and not fin[3].any() and not got["path_probs"][2:4].any()
    if name == "l64_a63":
        assert (got["lengths"][:, 0] == 64).all()
    if name == WC.LONGEST:
        assert (got["lengths"][:, 0] == L).all()


def test_the_prior_reverses_the_first_choice():
    r = _run(WC.REVERSING)
    d = r["d"]
    plain = r["dec"].beam_decode(r["x"], d["k"], d["eos"], pattern=r["base"], segments=r["seg"])
    mine, theirs = r["cpu"]["symbols"][:, 0], plain.symbols[:, 0].cpu()
    changed = [b for b in range(d["B"]) if not torch.equal(mine[b], theirs[b])]
    assert changed, "the prior changes no item's best hypothesis"
    assert torch.equal(mine.long(), d["f64"]["symbols"][:, 0])
    u = WC.unweighted_replay(d)
    assert torch.equal(theirs.long(), u["symbols"][:, 0])
    print(f"[weighted] {WC.REVERSING}: items {changed} change their best word: "
          f"{[WC.text_of(theirs[b], plain.lengths[b, 0], d['characters']) for b in changed]} -> "
          f"{[WC.text_of(mine[b], r['cpu']['lengths'][b, 0], d['characters']) for b in changed]}")


# ------------------------------------------------------------------ 3. exhaustive
@pytest.mark.parametrize("name", list(WC.EXHAUSTIVE))
def test_exhaustive_against_forced_decoding(name):
    """at most k words, each shorter than L - 1: every word of the language is returned; model_scores are `ASTER_V2.score` of
    the word, scores that plus scale * (the weight of the word), the order is by fused score"""
    r = _run(name)
    d, got = r["d"], r["cpu"]
    fin = torch.isfinite(got["scores"])
    words = d["words"][None]
    forced = r["dec"].score(r["x"], r["got"].symbols, r["got"].lengths, eos=d["eos"])
    fs = forced.scores.cpu()
    bound = _fused_bound(d)
    for b in range(d["B"]):
        n = int(fin[b].sum())
        assert fin[b, :n].all() and n == len(words)
        texts = [WC.text_of(got["symbols"][b, i], got["lengths"][b, i], d["characters"]) for i in range(n)]
        assert sorted(texts) == sorted(words)
        assert torch.equal(got["scores"][b, :n], got["scores"][b, :n].sort(descending=True).values), "best first, by fused score"
        for i, w in enumerate(texts):
            assert float(got["model_scores"][b, i]) == pytest.approx(float(fs[b, i]), abs=TOL)
            want = float(fs[b, i]) + d["scale"] * d["weights"][None].total(w)
            assert abs(float(got["scores"][b, i]) - want) <= bound[b, i], (b, w)
    assert not torch.equal(got["scores"][fin], got["model_scores"][fin])
    print(f"[weighted] {name}: model scores vs forced decoding max |d| {G._absdiff(got['model_scores'][fin], fs[fin]):.3e}")


# ------------------------------------------------------------------ 4. the step kernel as the replay's step
@pytest.mark.parametrize("name", ["trigram_ab_l5_k5", "priors_reverse_k3", "two_segments_start_w"])
def test_against_the_kernel_driven_replay(name):
    """the weighted replay with every step's logits from `K.attention_decode_step` on inflated inputs: symbols exact"""
    from glass_amd.ops import native as K
    r = _run(name)
    d, dec, x = r["d"], r["dec"], r["x"]
    B, k, T, L, C, eos = (d[n] for n in ("B", "k", "T", "L", "C", "eos"))
    xproj = K.linear(x.view(B * T, 256), dec.w["xW"], dec.w["xB"]).view(B, T, 256)
    xi = x.unsqueeze(1).expand(B, k, T, 256).reshape(B * k, T, 256).contiguous()
    xpi = xproj.unsqueeze(1).expand(B, k, T, 256).reshape(B * k, T, 256).contiguous()

    def step(state, y_prev):
        logits, _, state = K.attention_decode_step(xi, xpi, dec.w, state, y_prev.to(torch.int32).to(x.device), C)
        return logits, state
    drv = WC.replay_with(step, torch.zeros((B * k, 256), dtype=torch.float32, device=x.device), B, k, C, L, eos, d["keys"],
                         d["item_roots"], d["item_weights"], d["scale"])
    got = r["cpu"]
    assert torch.equal(got["symbols"].long(), drv["symbols"]) and torch.equal(got["lengths"].long(), drv["lengths"])
    assert G._absdiff(got["model_scores"], drv["model_scores"]) < TOL
    print(f"[weighted] {name}: vs the kernel-driven replay: model {G._absdiff(got['model_scores'], drv['model_scores']):.3e}, "
          f"fused {G._absdiff(got['scores'], drv['scores']):.3e}")


# ------------------------------------------------------------------ 5. repeated runs, distributions, the empty batch
def test_two_runs_are_bit_identical():
    r = _run("rows512_b32_k16")
    d = r["d"]
    again = r["dec"].beam_decode(r["x"], d["k"], d["eos"], path_probs=True, pattern=r["pat"], segments=r["seg"], weight_scale=d["scale"])
    for n in FIELDS:
        assert torch.equal(_bits(getattr(again, n)), _bits(r["cpu"][n])), n


def test_distributions_empty_batch_and_refusals():
    from glass_amd.evaluation.lexicon import LexiconTrie
    r = _run("two_segments_start_w")
    d, dec = r["d"], r["dec"]
    out = dec.beam_decode(r["x"], d["k"], d["eos"], path_probs=True, distributions="best", pattern=r["pat"], segments=r["seg"],
                          weight_scale=d["scale"])
    assert torch.equal(out.words, r["got"].words) and torch.equal(out.scores, r["got"].scores)
    assert out.distributions.shape == (d["B"], d["L"], d["C"])
    want = dec.score(r["x"], out.symbols[:, 0].contiguous(), out.lengths[:, 0].contiguous(), eos=d["eos"], probs=True).probs
    assert torch.equal(out.distributions, want) and not out.distributions[2:4].any() and out.distributions[0].any()
    every = dec.beam_decode(r["x"], d["k"], d["eos"], distributions="all", pattern=r["pat"], segments=r["seg"], weight_scale=d["scale"])
    assert every.distributions.shape == (d["B"], d["k"], d["L"], d["C"]) and torch.equal(every.distributions[:, 0], want)
    e = dec.beam_decode(torch.zeros((0, 7, 256), device=r["x"].device), 3, d["eos"], path_probs=True, pattern=r["pat"],
                        segments=torch.zeros((0,), dtype=torch.int32, device=r["x"].device))
    assert e.symbols.shape == (0, 3, d["L"]) and e.words.shape == (0, 3) and e.path_probs.shape == (0, d["L"], d["C"])
    assert e.model_scores.shape == e.scores.shape == (0, 3)
    trie = LexiconTrie(["ab"], d["characters"], d["L"], d["eos"], case_insensitive=False, device=G._dev())
    with pytest.raises(ValueError, match="lexicon and pattern"):
        dec.beam_decode(r["x"], d["k"], d["eos"], lexicon=trie, pattern=r["pat"])


# ------------------------------------------------------------------ 6. the recognizer head, the runner and the driver
REGEX = GP.REGEX
# a bonus that outweighs what a character costs under the synthetic model (about log 97 where it is near uniform): the longest
# string of the regex wins, so the weighted rows differ from the unweighted ones
BONUS, SCALE = 12.0, 0.8


def test_head_set_pattern_with_weights():
    """the rows a weighted search hands on are the model's conditional probabilities: the product of a RoI's non-zero entries is
    exp(model score), not the fused score"""
    from glass_amd.evaluation.pattern import DecodePattern
    x, roi_image = GP._features()
    h = GL._head(["MODEL.ROI_RECOGNIZER_HEAD.BEAM_WIDTH", 3])
    base = DecodePattern(REGEX, h.text_encoder, h.decoder.max_word_len, h.beam_eos, device=G._dev())
    wp = base.weighted(length_bonus=BONUS)
    h.set_pattern(base)
    unweighted = h.forward_nhwc(x, roi_image, 2)
    h.set_pattern(wp, weight_scale=SCALE)
    p = h.forward_nhwc(x, roi_image, 2)
    enc = h.encoder.forward_nhwc(h.backbone.forward_nhwc(x), rnn="steps")
    r = h.decoder.beam_decode(enc, 3, h.beam_eos, path_probs=True, pattern=wp, weight_scale=SCALE)
    assert torch.equal(p, r.path_probs) and not torch.equal(p, unweighted)
    texts, scores = G._decode_rows(h, p)
    model, fused = r.model_scores[:, 0].cpu().double().numpy(), r.scores[:, 0].cpu().double().numpy()
    print(f"[weighted] head: {texts} {scores.tolist()} model {model.tolist()} fused {fused.tolist()}")
    assert all(re.fullmatch(REGEX, t) for t in texts), texts
    rows = p.cpu().double().numpy()
    prod = np.array([np.prod(q[q != 0]) for q in rows])
    assert (np.abs(prod - np.exp(model)) <= 1e-4 * np.exp(model)).all()
    assert (np.abs(scores - np.exp(model)) <= 1e-4 * np.exp(model)).all()
    want = model + SCALE * BONUS * np.array([len(t) for t in texts])
    assert float(np.abs(fused - want).max()) < TOL + 2 * 27 * 2.0 ** -23 * max(1.0, float(np.abs(fused).max()), SCALE * BONUS * 5)
    assert (np.abs(fused - model) > 1.0).all()                                       # and it is not the fused score
    # ---- scale 0: the unweighted search's rows, bit for bit; None switches everything off
    h.set_pattern(wp, weight_scale=0.0)
    assert torch.equal(h.forward_nhwc(x, roi_image, 2), unweighted)
    h.set_pattern(None)
    assert h.pattern is None and h.weight_scale == 1.0
    # ---- the config key builds the same pattern at construction
    hc = GL._head(["MODEL.ROI_RECOGNIZER_HEAD.BEAM_WIDTH", 3, "MODEL.ROI_RECOGNIZER_HEAD.DECODE_PATTERN", REGEX,
                   "MODEL.ROI_RECOGNIZER_HEAD.DECODE_LENGTH_BONUS", BONUS])
    assert np.array_equal(hc.pattern.trans, wp.trans) and hc.weight_scale == 1.0
    h.set_pattern(wp)
    assert torch.equal(hc.forward_nhwc(x, roi_image, 2), h.forward_nhwc(x, roi_image, 2))


def test_runner_and_driver_with_a_weighted_pattern():
    """DECODE_LENGTH_BONUS through GlassRunner's opts gives the rows of set_pattern(weighted); 0.0 changes nothing;
    inference_on_dataset(pattern=weighted) switches the head and hands it back; run_tiled takes a one-segment weighted pattern"""
    from glass_amd.config import get_glass_cfg
    from glass_amd.data import DatasetMapper
    from glass_amd.evaluation import inference_on_dataset
    from glass_amd.evaluation.pattern import DecodePattern
    from glass_amd.inference.glass_runner import GlassRunner
    from glass_amd.utils.synth import make_image, make_state_dict
    img = make_image(3, 160, 224).numpy()
    base = ["MODEL.DEVICE", "cuda:0", "INPUT.MIN_SIZE_TEST", 160, "INPUT.MAX_SIZE_TEST", 200, "POST_PROCESSING.TEXT_THRESHOLD", 0.0,
            "MODEL.ROI_RECOGNIZER_HEAD.BEAM_WIDTH", 3, "MODEL.ROI_RECOGNIZER_HEAD.DECODE_PATTERN", REGEX]
    path = os.path.join(ROOT, "configs", "glass_icdar15_mi355x.yaml")
    sd = make_state_dict(1234)
    with_key, by_hand, zero_key = (GlassRunner(None, path, opts=base + extra, state_dict=sd, post_process=True)
                                   for extra in (["MODEL.ROI_RECOGNIZER_HEAD.DECODE_LENGTH_BONUS", BONUS], [],
                                                 ["MODEL.ROI_RECOGNIZER_HEAD.DECODE_LENGTH_BONUS", 0.0]))
    h = by_hand.model.roi_heads.recognizer_head
    assert type(h.pattern) is DecodePattern and type(zero_key.model.roi_heads.recognizer_head.pattern) is DecodePattern
    plain = by_hand(img)
    assert len(plain) > 0
    GP._same_instances(zero_key(img), plain, "DECODE_LENGTH_BONUS 0.0")
    wp = h.pattern.weighted(length_bonus=BONUS)
    unweighted_pattern = h.pattern
    h.set_pattern(wp)
    keyed = with_key(img)
    GP._same_instances(keyed, by_hand(img), "DECODE_LENGTH_BONUS against set_pattern")
    assert not torch.equal(keyed.pred_text_prob, plain.pred_text_prob)
    assert keyed.has("pred_texts") and all(re.fullmatch(REGEX, t) for t in keyed.pred_texts), keyed.pred_texts
    assert sum(len(t) for t in keyed.pred_texts) >= sum(len(t) for t in plain.pred_texts), "the bonus shortens the words"
    tiled = by_hand.run_tiled(img, tile=128, overlap=64, border=8)                   # one segment: accepted
    assert len(tiled) > 0 and all(re.fullmatch(REGEX, t) for t in tiled.pred_texts)
    # ---- the driver
    cfg, model = GP._model()
    head = model.roi_heads.recognizer_head
    rx = {"img_0.jpg": r"\d{2,4}", "img_1.jpg": REGEX}
    pat = DecodePattern(rx, head.text_encoder, head.decoder.max_word_len, head.beam_eos, device=G._dev())
    wpat = pat.weighted(length_bonus=BONUS)
    dds = [{"file_name": f"img_{i}.jpg", "image": make_image(i, 96, 128).numpy(), "annotations": []} for i in range(2)]
    mapper = DatasetMapper(cfg, device="cuda:0", fused=True)
    head.set_pattern(DecodePattern(REGEX, head.text_encoder, head.decoder.max_word_len, head.beam_eos, device=G._dev())
                     .weighted(length_bonus=0.5), weight_scale=0.25)
    mine = head.pattern
    unweighted = inference_on_dataset(model, dds, mapper, batch_size=8, pattern=pat, pattern_key=lambda inp: inp["file_name"])
    outs = inference_on_dataset(model, dds, mapper, batch_size=8, pattern=wpat, pattern_key=lambda inp: inp["file_name"])
    assert head.pattern is mine and head.weight_scale == 0.25 and head.image_segments is None       # handed back as it was
    survived = longer = 0
    for dd, o, u in zip(dds, outs, unweighted):
        inst = o["instances"]
        if len(inst):
            texts, _ = G._decode_rows(head, inst.pred_text_prob)
            print(f"[weighted] driver: {dd['file_name']}: {texts}")
            assert all(re.fullmatch(rx[dd["file_name"]], t) for t in texts), (dd["file_name"], texts)
            survived += len(texts)
            longer += int(not torch.equal(inst.pred_text_prob, u["instances"].pred_text_prob)) if len(inst) == len(u["instances"]) else 1
    assert survived > 0 and longer > 0, "no word survived, or the weights changed none: the case checks nothing"
    assert unweighted_pattern is not wp and type(unweighted_pattern) is DecodePattern
