"""GPU: the pattern-constrained device beam search (glass_beam_search_dfa, ASTER_V2.beam_decode(pattern=...),
RecognizerRCNNHeadV3.set_pattern, MODEL.ROI_RECOGNIZER_HEAD.DECODE_PATTERN, inference_on_dataset(pattern=...)): bit-equal to the
lexicon search on a trie turned into a DFA, against the float64 replay of tests/lexicon_beam_cases.py on the ENUMERATED
language of every regex case (tests/pattern_cases.py), against forced decoding, and through the head and the driver."""
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

pytestmark = pytest.mark.gpu

ROOT = LC.ROOT
# the constants of tests/test_gpu_beam_search.py, measured there for this step arithmetic
MARGIN, TOL = G.MARGIN, G.TOL
assert (MARGIN, TOL) == (PC.MARGIN, PC.TOL)
FIELDS = ("symbols", "scores", "lengths", "path_probs", "words")


def _bits(t):
    return t.cpu().contiguous().view(torch.int32) if t.dtype == torch.float32 else t.cpu()


def _pattern(d, **kw):
    from glass_amd.evaluation.pattern import DecodePattern
    return DecodePattern(d["patterns"], d["characters"], d["L"], d["eos"], case_insensitive=d["ci"], device=G._dev(), **kw)


# ------------------------------------------------------------------ 1. a trie as a DFA
@pytest.mark.parametrize("name", list(LC.CASES))
def test_trie_as_dfa_is_bit_equal_to_the_lexicon_search(name):
    """the masks are identical by construction: symbols, lengths and words equal, scores and path rows bit-equal"""
    from glass_amd.evaluation.pattern import DecodePattern
    r = GL._run(name)
    d = r["d"]
    pat = DecodePattern.from_trie(r["trie"])
    assert pat.tensors["next"].device == r["x"].device and pat.num_states == r["trie"].num_nodes
    got = r["dec"].beam_decode(r["x"], d["k"], d["eos"], path_probs=True, pattern=pat, segments=r["seg"])
    for n in FIELDS:
        a, b = _bits(getattr(got, n)), _bits(getattr(r["got"], n))
        assert a.dtype == b.dtype and torch.equal(a, b), (name, n)


# ------------------------------------------------------------------ 2. regex cases against the float64 replay
_RUNS = {}


def _run(name):
    if name not in _RUNS:
        d = PC.case_data(name)
        dec = G._decoder(d["sd"], d["C"], d["L"])
        x = d["x"].to(G._dev())
        pat = _pattern(d)
        seg = torch.tensor(PC.item_segments(d), dtype=torch.int32).to(G._dev())      # a device tensor: passed through unchecked
        got = dec.beam_decode(x, d["k"], d["eos"], path_probs=True, pattern=pat, segments=seg)
        _RUNS[name] = dict(d=d, dec=dec, x=x, pat=pat, seg=seg, got=got, cpu={n: getattr(got, n).cpu() for n in FIELDS})
    return _RUNS[name]


@pytest.mark.parametrize("name", list(PC.CASES))
def test_regex_cases_against_the_float64_replay(name):
    """symbols and lengths exact, scores and path rows within TOL, tags 0 / -1; no item is excluded.
    Measured on an MI355X, per case: smallest gap (selection or completion, float64 replay) | largest |dscore| of the device
    search vs the float64 replay | states
      greedy_k1_c13_l4        2.7e+0 | 2.1e-6 | 2        digits_l4_k5       7.9e-2 | 3.7e-6 | 2
      too_long_for_l4         -      | 0      | 5        plates_c97_l26_t32_k3  3.4e-3 | 3.4e-6 | 6
      shared_prefix_k4        1.0e+0 | 4.8e-6 | 4        star_k4            9.7e-2 | 4.8e-6 | 2
      rows512_b32_k16         2.7e-3 | 1.2e-5 | 2        c256_identity      7.5e-2 | 1.2e-5 | 3
      t64                     1.1e+0 | 1.8e-6 | 4        l64_a63            -      | 7.7e-7 | 64
      two_segments            1.2e-2 | 3.7e-6 | 5        exhaustive_k4      3.1e-1 | 3.8e-6 | 4"""
    r = _run(name)
    d, got = r["d"], r["cpu"]
    f64, B, k, L, C = d["f64"], d["B"], d["k"], d["L"], d["C"]
    gap = min(float(f64["sel_gap"].min()), float(f64["done_gap"].min()))
    print(f"[pattern] {name}: smallest gap {gap:.3e}; device vs float64 replay {G._absdiff(got['scores'], f64['scores']):.3e}; "
          f"{r['pat'].num_states} states, F {r['pat'].num_fold}, {r['pat'].nbytes} bytes, built in {r['pat'].build_seconds:.3f} s")
    assert gap > MARGIN, "a near-tie: choose another seed for this case, do not relax the margin"
    assert got["symbols"].shape == (B, k, L) and got["scores"].shape == got["lengths"].shape == got["words"].shape == (B, k)
    assert got["path_probs"].shape == (B, L, C) and got["words"].dtype == torch.int32
    assert torch.equal(got["symbols"].long(), f64["symbols"]), name
    assert torch.equal(got["lengths"].long(), f64["lengths"]), name
    fin = torch.isfinite(f64["scores"])
    assert (torch.isneginf(got["scores"]) == ~fin).all() and not torch.isnan(got["scores"]).any()
    assert torch.equal(got["words"].long(), torch.where(fin, 0, -1)), "tags: 0 for a regex, -1 for an absent hypothesis"
    assert G._absdiff(got["scores"], f64["scores"]) < TOL
    for b in range(B):
        want = BC.path_rows(f64["symbols"][b, 0], f64["step_scores"][b, 0], f64["lengths"][b, 0], f64["scores"][b, 0], C)
        rows = got["path_probs"][b].double().numpy()
        assert ((rows != 0) == (want != 0)).all(), (name, b)
        assert float(np.abs(rows - want).max()) < TOL, (name, b)
    if name == "too_long_for_l4":
        assert not fin.any() and not got["lengths"].any() and not got["path_probs"].any()
    if name == "two_segments":
        assert not fin[2].any() and not fin[3].any() and not got["path_probs"][2:4].any()
    if name == "l64_a63":
        assert r["pat"].dist[r["pat"].start[0]] == 63 and (got["lengths"][:, 0] == 64).all()


# ------------------------------------------------------------------ 3. exhaustive
@pytest.mark.parametrize("name", list(PC.EXHAUSTIVE))
def test_exhaustive_against_forced_decoding(name):
    """at most k words, each shorter than L - 1: the finite hypotheses are exactly the language, their scores those of
    `ASTER_V2.score` on word + eos"""
    r = _run(name)
    d, got = r["d"], r["cpu"]
    fin = torch.isfinite(got["scores"])
    words = d["words"][None]
    for b in range(d["B"]):
        n = int(fin[b].sum())
        assert fin[b, :n].all() and n == len(words)
        texts = [PC.text_of(got["symbols"][b, i], got["lengths"][b, i], d["characters"]) for i in range(n)]
        assert sorted(texts) == sorted(words)
        for i, w in enumerate(texts):
            assert got["symbols"][b, i].tolist() == [d["characters"].index(c) for c in w] + [d["eos"]] * (d["L"] - len(w))
    forced = r["dec"].score(r["x"], r["got"].symbols, r["got"].lengths, eos=d["eos"])
    fs = forced.scores.cpu()
    diff = G._absdiff(got["scores"][fin], fs[fin])
    print(f"[pattern] {name}: search vs forced decoding max |dscore| {diff:.3e}, bit-equal: "
          f"{bool(torch.equal(got['scores'][fin].view(torch.int32), fs[fin].view(torch.int32)))}")
    assert diff < TOL
    assert (fs[~fin] == 0).all() and (forced.lengths.cpu()[~fin] == 0).all()


# ------------------------------------------------------------------ 4. property
@pytest.mark.parametrize("regex", PC.PROPERTY_REGEXES)
def test_every_hypothesis_matches_its_regex(regex):
    """seeded random inputs on the shipped character set: every finite hypothesis satisfies re.fullmatch and fits the steps;
    hypothesis 0 is absent only where the language is empty at that L"""
    from glass_amd.evaluation.pattern import DecodePattern
    chars = LC.shipped_characters()
    B, k, T, L, C, eos = 6, 5, 16, 26, 97, 1
    dec = G._decoder(BC.decoder_sd(C, fc_scale=1.0, eos=eos), C, L)
    x = PC.rng_x(B, T, 4242).to(G._dev())
    pat = DecodePattern(regex, chars, L, eos, device=G._dev())
    got = dec.beam_decode(x, k, eos, pattern=pat)
    sc, ln, sym, tags = got.scores.cpu(), got.lengths.cpu(), got.symbols.cpu(), got.words.cpu()
    fin = torch.isfinite(sc)
    assert (torch.isneginf(sc) == ~fin).all() and ((ln > 0) == fin).all() and torch.equal(tags.long(), torch.where(fin, 0, -1))
    rx = re.compile(regex)
    seen = set()
    for b in range(B):
        assert torch.equal(sc[b], sc[b].sort(descending=True).values), "best first"
        for i in range(k):
            if fin[b, i]:
                text = PC.text_of(sym[b, i], ln[b, i], chars)
                assert 1 <= len(text) == int(ln[b, i]) - 1 <= L - 1 and rx.fullmatch(text), (regex, b, i, text)
                assert int(sym[b, i, int(ln[b, i]) - 1]) == eos
                seen.add(text)
    empty = regex == r"x{30}"
    assert pat.start.tolist() == ([-1] if empty else [0])
    assert (~fin[:, 0]).all() if empty else fin[:, 0].all()
    print(f"[pattern] {regex}: {int(fin.sum())} finite hypotheses, e.g. {sorted(seen)[:6]}")


# ------------------------------------------------------------------ 5. equivalent automata, repeated runs
@pytest.mark.parametrize("name", ["star_k4", "plates_c97_l26_t32_k3", "rows512_b32_k16"])
def test_equivalent_automata_and_two_runs_are_bit_identical(name):
    r = _run(name)
    d = r["d"]
    raw = _pattern(d, minimize=False)
    assert raw.num_states >= r["pat"].num_states
    other = r["dec"].beam_decode(r["x"], d["k"], d["eos"], path_probs=True, pattern=raw, segments=r["seg"])
    again = r["dec"].beam_decode(r["x"], d["k"], d["eos"], path_probs=True, pattern=r["pat"], segments=r["seg"])
    for n in FIELDS:
        assert torch.equal(_bits(getattr(other, n)), _bits(r["cpu"][n])), (name, n, "minimize=False")
        assert torch.equal(_bits(getattr(again, n)), _bits(r["cpu"][n])), (name, n, "second run")
    print(f"[pattern] {name}: {raw.num_states} states unminimised, {r['pat'].num_states} minimised")


def test_distributions_and_empty_batch():
    r = _run("two_segments")
    d, dec = r["d"], r["dec"]
    out = dec.beam_decode(r["x"], d["k"], d["eos"], path_probs=True, distributions="all", pattern=r["pat"], segments=r["seg"])
    assert torch.equal(out.words, r["got"].words) and out.distributions.shape == (d["B"], d["k"], d["L"], d["C"])
    want = dec.score(r["x"], out.symbols, out.lengths, eos=d["eos"], probs=True).probs
    assert torch.equal(out.distributions, want) and not out.distributions[2:4].any()
    e = dec.beam_decode(torch.zeros((0, 7, 256), device=r["x"].device), 3, d["eos"], path_probs=True, pattern=r["pat"],
                        segments=torch.zeros((0,), dtype=torch.int32, device=r["x"].device))
    assert e.symbols.shape == (0, 3, d["L"]) and e.words.shape == (0, 3) and e.path_probs.shape == (0, d["L"], d["C"])


# ------------------------------------------------------------------ 6. the recognizer head and the driver
REGEX = r"[A-Z]{2}\d{1,3}"


def _features():
    g = torch.Generator(device="cpu")
    g.manual_seed(77)
    x = torch.randn((5, 8, 32, 256), generator=g).to(G._dev())
    return x, torch.tensor([0, 0, 0, 1, 1], dtype=torch.int32, device=G._dev())


def test_head_set_pattern_and_config_key():
    from glass_amd.evaluation.lexicon import LexiconTrie
    from glass_amd.evaluation.pattern import DecodePattern
    x, roi_image = _features()
    h = GL._head(["MODEL.ROI_RECOGNIZER_HEAD.BEAM_WIDTH", 3])
    assert h.pattern is None
    free = h.forward_nhwc(x, roi_image, 2)
    pat = DecodePattern(REGEX, h.text_encoder, h.decoder.max_word_len, h.beam_eos, device=G._dev())
    h.set_pattern(pat)
    p = h.forward_nhwc(x, roi_image, 2)
    enc = h.encoder.forward_nhwc(h.backbone.forward_nhwc(x), rnn="steps")
    r = h.decoder.beam_decode(enc, 3, h.beam_eos, path_probs=True, pattern=pat)
    assert torch.equal(p, r.path_probs) and not torch.equal(p, free)
    texts, scores = G._decode_rows(h, p)                                             # glass_text_argmax + the word post-processor
    best = r.scores[:, 0].cpu().double().numpy()
    print(f"[pattern] head: {texts} {scores.tolist()} scores {best.tolist()}")
    assert all(re.fullmatch(REGEX, t) for t in texts), texts
    assert (np.abs(scores - np.exp(best)) <= 1e-4 * np.exp(best)).all()
    # ---- the two constraints exclude each other
    trie = LexiconTrie(["car"], h.text_encoder, h.decoder.max_word_len, h.beam_eos, device=G._dev())
    with pytest.raises(ValueError, match="pattern is set"):
        h.set_lexicon(trie)
    h.set_pattern(None)
    assert torch.equal(h.forward_nhwc(x, roi_image, 2), free)                        # switched off: bit for bit
    h.set_lexicon(trie)
    with pytest.raises(ValueError, match="lexicon is set"):
        h.set_pattern(pat)
    # ---- DECODE_PATTERN builds the same pattern at construction
    hc = GL._head(["MODEL.ROI_RECOGNIZER_HEAD.BEAM_WIDTH", 3, "MODEL.ROI_RECOGNIZER_HEAD.DECODE_PATTERN", REGEX])
    assert hc.pattern is not None and np.array_equal(hc.pattern.next, pat.next)
    assert torch.equal(hc.forward_nhwc(x, roi_image, 2), p)
    # ---- with BEAM_DISTRIBUTIONS: the full rows are a forced replay of the best hypothesis
    hd = GL._head(["MODEL.ROI_RECOGNIZER_HEAD.BEAM_WIDTH", 3, "MODEL.ROI_RECOGNIZER_HEAD.BEAM_DISTRIBUTIONS", True])
    hd.set_pattern(pat)
    rows, dist = hd.forward_nhwc(x, roi_image, 2)
    assert torch.equal(rows, p)
    want = hd.decoder.score(enc, r.symbols[:, 0].contiguous(), r.lengths[:, 0].contiguous(), eos=h.beam_eos, probs=True).probs
    assert torch.equal(dist, want) and dist.any()
    # ---- per-image segments, one of them with no string at this max_len: all-zero rows
    two = DecodePattern({"none": r"x{40}", "p": REGEX}, h.text_encoder, h.decoder.max_word_len, h.beam_eos, device=G._dev())
    h.set_lexicon(None)
    h.set_pattern(two, torch.tensor([0, 1], dtype=torch.int32).to(G._dev()))
    z = h.forward_nhwc(x, roi_image, 2)
    assert not z[:3].any() and torch.equal(z[3:], p[3:])


def _model(opts=()):
    import glass_amd
    from glass_amd.config import get_glass_cfg
    from glass_amd.utils.synth import make_state_dict
    cfg = get_glass_cfg(os.path.join(ROOT, "configs", "glass_icdar15_mi355x.yaml"),
                        ["MODEL.DEVICE", "cuda:0", "INPUT.MIN_SIZE_TEST", 128, "INPUT.MAX_SIZE_TEST", 1000,
                         "POST_PROCESSING.TEXT_THRESHOLD", 0.0, "POST_PROCESSING.DETECT_THRESHOLD", 0.0,
                         "POST_PROCESSING.LOW_CONFIDENCE", 0.0, "POST_PROCESSING.VALID_CONFIDENCE", 0.0,
                         "MODEL.ROI_RECOGNIZER_HEAD.BEAM_WIDTH", 3] + list(opts))
    model = glass_amd.build_model(cfg)
    model.load_state_dict(make_state_dict(1234))
    return cfg, model


def test_driver_and_runner_with_a_pattern():
    """inference_on_dataset(pattern=...) switches the head and hands it back; every surviving word matches its own image's
    regex; DECODE_PATTERN through GlassRunner's opts gives the rows of set_pattern; with the key empty and no pattern set the
    outputs are the plain search's, bit for bit"""
    from glass_amd.data import DatasetMapper
    from glass_amd.evaluation import inference_on_dataset
    from glass_amd.evaluation.pattern import DecodePattern
    from glass_amd.inference.glass_runner import GlassRunner
    from glass_amd.config import get_glass_cfg
    from glass_amd.utils.synth import make_image, make_state_dict
    cfg, model = _model()
    head = model.roi_heads.recognizer_head
    rx = {"img_0.jpg": r"\d{2,4}", "img_1.jpg": REGEX}
    pat = DecodePattern(rx, head.text_encoder, head.decoder.max_word_len, head.beam_eos, device=G._dev())
    dds = [{"file_name": f"img_{i}.jpg", "image": make_image(i, 96, 128).numpy(), "annotations": []} for i in range(2)]
    mapper = DatasetMapper(cfg, device="cuda:0", fused=True)
    plain = inference_on_dataset(model, dds, mapper, batch_size=8)
    outs = inference_on_dataset(model, dds, mapper, batch_size=8, pattern=pat, pattern_key=lambda inp: inp["file_name"])
    assert head.pattern is None and head.lexicon is None and head.image_segments is None      # handed back as it was
    survived = 0
    for dd, o in zip(dds, outs):
        inst = o["instances"]
        if len(inst):
            texts, _ = G._decode_rows(head, inst.pred_text_prob)
            print(f"[pattern] driver: {dd['file_name']}: {texts}")
            assert all(re.fullmatch(rx[dd["file_name"]], t) for t in texts), (dd["file_name"], texts)
            survived += len(texts)
    assert survived > 0, "no word survived: the case checks nothing"
    after = inference_on_dataset(model, dds, mapper, batch_size=8)
    for a, b in zip(plain, after):                                                   # no pattern: what it was before, bit for bit
        assert torch.equal(a["instances"].pred_text_prob, b["instances"].pred_text_prob)
        assert torch.equal(a["instances"].pred_boxes.tensor, b["instances"].pred_boxes.tensor)
    # ---- the config key through the runner against set_pattern on the model
    img = make_image(3, 160, 224).numpy()
    base = ["MODEL.DEVICE", "cuda:0", "INPUT.MIN_SIZE_TEST", 160, "INPUT.MAX_SIZE_TEST", 200, "POST_PROCESSING.TEXT_THRESHOLD", 0.0,
            "MODEL.ROI_RECOGNIZER_HEAD.BEAM_WIDTH", 3]
    path = os.path.join(ROOT, "configs", "glass_icdar15_mi355x.yaml")
    sd = make_state_dict(1234)
    with_key, by_hand, empty_key = (GlassRunner(None, None, cfg=get_glass_cfg(path, base + extra), state_dict=sd, post_process=True)
                                    for extra in (["MODEL.ROI_RECOGNIZER_HEAD.DECODE_PATTERN", REGEX], [],
                                                  ["MODEL.ROI_RECOGNIZER_HEAD.DECODE_PATTERN", ""]))
    assert empty_key.model.roi_heads.recognizer_head.pattern is None
    free = by_hand(img)
    assert len(free) > 0
    _same_instances(empty_key(img), free, "DECODE_PATTERN empty")
    h = by_hand.model.roi_heads.recognizer_head
    h.set_pattern(DecodePattern(REGEX, h.text_encoder, h.decoder.max_word_len, h.beam_eos, device=G._dev()))
    keyed = with_key(img)
    _same_instances(keyed, by_hand(img), "DECODE_PATTERN against set_pattern")
    assert not torch.equal(keyed.pred_text_prob, free.pred_text_prob)
    assert all(re.fullmatch(REGEX, t) for t in G._decode_rows(h, keyed.pred_text_prob)[0])
    assert keyed.has("pred_texts") and all(re.fullmatch(REGEX, t) for t in keyed.pred_texts), keyed.pred_texts    # the word post-processor
    assert len(by_hand.run_tiled(img, tile=128, overlap=64, border=8)) > 0          # one segment: accepted
    h.image_segments = torch.zeros((1,), dtype=torch.int32, device=G._dev())
    with pytest.raises(NotImplementedError, match="image_segments"):
        by_hand.run_tiled(img, tile=128, overlap=64, border=8)


def _same_instances(a, b, what):
    assert len(a) == len(b), (what, len(a), len(b))
    assert torch.equal(a.pred_boxes.tensor, b.pred_boxes.tensor) and torch.equal(a.scores, b.scores), what
    assert torch.equal(a.pred_text_prob, b.pred_text_prob), what
    if a.has("pred_polygons") or b.has("pred_polygons"):
        assert torch.equal(a.pred_polygons, b.pred_polygons) and a.pred_texts == b.pred_texts, what
        assert torch.equal(a.pred_text_scores, b.pred_text_scores), what
