"""GPU: the lexicon-constrained device beam search (glass_beam_search_lexicon, ASTER_V2.beam_decode(lexicon=...),
RecognizerRCNNHeadV3.set_lexicon, inference_on_dataset(lexicon=...)) against the float64 replay of tests/lexicon_beam_cases.py,
the same replay driven through the existing decoder-step kernel, forced decoding, and through the head and the driver."""
import math
import os

import numpy as np
import pytest
import torch

import beam_cases as BC
import lexicon_beam_cases as LC
import test_gpu_beam_search as G

pytestmark = pytest.mark.gpu

ROOT = LC.ROOT
# symbols, lengths and words are compared exactly, scores and path rows within TOL: the constants of the unconstrained
# search's test, measured there for the same step arithmetic (tests/test_gpu_beam_search.py); every item's gaps in the float64
# replay must exceed MARGIN (asserted on the CPU too: tests/test_lexicon_beam.py)
MARGIN, TOL = G.MARGIN, G.TOL
assert (MARGIN, TOL) == (LC.MARGIN, LC.TOL)


def _trie(d):
    from glass_amd.evaluation.lexicon import LexiconTrie
    return LexiconTrie(d["lexicon"], d["characters"], d["L"], d["eos"], case_insensitive=d["case_insensitive"], device=G._dev())


_RUNS = {}


def _run(name):
    """everything the tests of one case share, computed once: decoder, trie, the kernel-driven replay, the device search"""
    if name not in _RUNS:
        from glass_amd.ops import native as K
        d = LC.case_data(name)
        B, k, T, L, C, eos = (d[n] for n in ("B", "k", "T", "L", "C", "eos"))
        dec = G._decoder(d["sd"], C, L)
        x = d["x"].to(G._dev())
        trie = _trie(d)
        seg = torch.tensor(LC.item_segments(d), dtype=torch.int32).to(G._dev())      # a device tensor: passed through unchecked
        xproj = K.linear(x.view(B * T, 256), dec.w["xW"], dec.w["xB"]).view(B, T, 256)
        xi = x.unsqueeze(1).expand(B, k, T, 256).reshape(B * k, T, 256).contiguous()
        xpi = xproj.unsqueeze(1).expand(B, k, T, 256).reshape(B * k, T, 256).contiguous()

        def step(state, y_prev):
            logits, _, state = K.attention_decode_step(xi, xpi, dec.w, state, y_prev.to(torch.int32).to(x.device), C)
            return logits, state
        drv = LC.replay_with(step, torch.zeros((B * k, 256), dtype=torch.float32, device=x.device), B, k, C, L, eos, d["keys"],
                             d["item_roots"])
        got = dec.beam_decode(x, k, eos, path_probs=True, lexicon=trie, segments=seg)
        _RUNS[name] = dict(d=d, dec=dec, x=x, trie=trie, seg=seg, drv=drv, got=got,
                           cpu={n: getattr(got, n).cpu() for n in ("symbols", "scores", "lengths", "path_probs", "words")})
    return _RUNS[name]


@pytest.mark.parametrize("name", list(LC.CASES))
def test_all_hypotheses_against_the_replays(name):
    """symbols, lengths, words and the zero pattern of the path rows = the replay's (all-float64, and with every step's logits
    from `K.attention_decode_step` on inflated inputs); scores and path rows within TOL of both.  No item is excluded.
    Measured on an MI355X, per case: smallest selection gap | smallest completion gap (float64 replay) || largest |dscore| of
    the device search vs the kernel-driven replay | vs the float64 replay
      k1_c5_l1             -      | -      || 0      | 0         (no word fits one step: no hypothesis at all)
      k2_c13_l4            3.2e-1 | 3.8e+0 || 1.0e-6 | 3.2e-6
      k3_c97_l26_shipped   3.9e-2 | 8.9e-2 || 1.5e-5 | 1.3e-5
      k5_c256_l6_mw8       5.2e-1 | 2.6e+0 || 4.6e-6 | 1.8e-5
      k16_b32_l6_rows512   5.9e-4 | 5.6e-3 || 4.8e-6 | 1.2e-5
      k4_many_completions  1.7e-1 | 5.6e-2 || 2.3e-6 | 2.8e-6
      k5_dead_slots        -      | 2.8e+0 || 4.1e-7 | 1.5e-6
      k16_exhaustive       -      | 3.0e-2 || 3.1e-6 | 6.2e-6"""
    r = _run(name)
    d, drv, got = r["d"], r["drv"], r["cpu"]
    f64, B, k, L, C = d["f64"], d["B"], d["k"], d["L"], d["C"]
    gap = min(float(f64["sel_gap"].min()), float(f64["done_gap"].min()))
    print(f"[lexbeam] {name}: smallest selection gap {float(f64['sel_gap'].min()):.3e}, smallest completion gap "
          f"{float(f64['done_gap'].min()):.3e}; device vs kernel-driven replay {G._absdiff(got['scores'], drv['scores']):.3e}, "
          f"vs float64 replay {G._absdiff(got['scores'], f64['scores']):.3e}; trie {r['trie'].num_nodes} nodes, F {r['trie'].num_fold}, "
          f"MW {r['trie'].mask_words}, completed {f64['completed'].tolist()}")
    assert gap > MARGIN, "a near-tie: choose another seed for this case, do not relax the margin"
    assert got["symbols"].shape == (B, k, L) and got["scores"].shape == got["lengths"].shape == got["words"].shape == (B, k)
    assert got["path_probs"].shape == (B, L, C) and got["words"].dtype == torch.int32
    for ref in (f64, drv):
        assert torch.equal(got["symbols"].long(), ref["symbols"]), name
        assert torch.equal(got["lengths"].long(), ref["lengths"]), name
        assert torch.equal(got["words"].long(), ref["words"]), name
        assert (torch.isneginf(got["scores"]) == torch.isneginf(ref["scores"])).all()
        assert G._absdiff(got["scores"], ref["scores"]) < TOL
        for b in range(B):
            want = BC.path_rows(ref["symbols"][b, 0], ref["step_scores"][b, 0], ref["lengths"][b, 0], ref["scores"][b, 0], C)
            rows = got["path_probs"][b].double().numpy()
            assert ((rows != 0) == (want != 0)).all(), (name, b)
            assert float(np.abs(rows - want).max()) < TOL, (name, b)
    assert not torch.isnan(got["scores"]).any() and not (got["scores"] == math.inf).any()
    if name == "k5_c256_l6_mw8":
        assert r["trie"].mask_words == 8
    if name == "k3_c97_l26_shipped":
        assert r["trie"].num_fold < 95 and not torch.isfinite(got["scores"][2:4]).any()


@pytest.mark.parametrize("name", LC.EXHAUSTIVE)
def test_exhaustive_against_forced_decoding(name):
    """identity fold, at most k words, every word shorter than max_len - 1: the finite hypotheses are exactly the segment's
    words, and their scores those of `ASTER_V2.score` on word + eos"""
    r = _run(name)
    d, got = r["d"], r["cpu"]
    all_words = [w for key in d["lexicon"] for w in d["lexicon"][key]]
    fin = torch.isfinite(got["scores"])
    for b, key in enumerate(d["item_keys"]):
        n = int(fin[b].sum())
        assert fin[b, :n].all() and sorted(all_words[int(i)] for i in got["words"][b, :n]) == sorted(d["lexicon"][key])
        for i in range(n):
            w = all_words[int(got["words"][b, i])]
            assert got["symbols"][b, i].tolist() == [d["characters"].index(c) for c in w] + [d["eos"]] * (d["L"] - len(w))
    forced = r["dec"].score(r["x"], r["got"].symbols, r["got"].lengths, eos=d["eos"])
    fs = forced.scores.cpu()
    diff = G._absdiff(got["scores"][fin], fs[fin])
    print(f"[lexbeam] {name}: search vs forced decoding max |dscore| {diff:.3e}, bit-equal: "
          f"{bool(torch.equal(got['scores'][fin].view(torch.int32), fs[fin].view(torch.int32)))}")
    assert diff < TOL
    assert (fs[~fin] == 0).all() and (forced.lengths.cpu()[~fin] == 0).all()          # a missing hypothesis has length 0


def test_two_runs_are_bit_identical():
    r = _run("k16_b32_l6_rows512")
    d = r["d"]
    again = r["dec"].beam_decode(r["x"], d["k"], d["eos"], path_probs=True, lexicon=r["trie"], segments=r["seg"])
    for n, t in r["cpu"].items():
        assert torch.equal(getattr(again, n).cpu().view(torch.int32), t.view(torch.int32)), n


def test_distributions_are_a_forced_replay():
    r = _run("k3_c97_l26_shipped")
    d, dec = r["d"], r["dec"]
    out = dec.beam_decode(r["x"], d["k"], d["eos"], path_probs=True, distributions="all", lexicon=r["trie"], segments=r["seg"])
    assert torch.equal(out.words, r["got"].words) and out.distributions.shape == (d["B"], d["k"], d["L"], d["C"])
    want = dec.score(r["x"], out.symbols, out.lengths, eos=d["eos"], probs=True).probs
    assert torch.equal(out.distributions, want)
    assert not out.distributions[2:4].any()                                            # the items without a hypothesis


def test_limits_raise_before_any_launch_and_empty_batch():
    from glass_amd._lib import GlassLibraryError
    from glass_amd.ops import native as K
    r = _run("k2_c13_l4")
    d, dec, trie = r["d"], r["dec"], r["trie"]
    C, L, eos = d["C"], d["L"], d["eos"]
    x = r["x"][:2].contiguous()
    xp = torch.zeros_like(x)
    seg = torch.zeros((2,), dtype=torch.int32, device=x.device)
    t = trie.tensors
    with pytest.raises(GlassLibraryError, match="k=17"):
        K.beam_search_lexicon(x, xp, dec.w, 17, C, L, eos, t, seg)
    with pytest.raises(GlassLibraryError, match="k=14 .* C=13"):
        K.beam_search_lexicon(x, xp, dec.w, 14, C, L, eos, t, seg)
    with pytest.raises(GlassLibraryError, match="max_len=65"):
        K.beam_search_lexicon(x, xp, dec.w, 2, C, 65, eos, t, seg)
    x65 = torch.zeros((2, 65, 256), device=x.device)
    with pytest.raises(GlassLibraryError, match="T=65"):
        K.beam_search_lexicon(x65, x65, dec.w, 2, C, L, eos, t, seg)
    for name in ("child_mask", "child_base", "node_word", "seg_root", "fold"):
        with pytest.raises(GlassLibraryError, match="null|N=0|S=0"):
            K.beam_search_lexicon(x, xp, dec.w, 2, C, L, eos, {**t, name: None}, seg)
    for F in (0, 257):
        with pytest.raises(GlassLibraryError, match=f"F={F}"):
            K.beam_search_lexicon(x, xp, dec.w, 2, C, L, eos, {**t, "F": F}, seg)
    with pytest.raises(GlassLibraryError):
        K.beam_search_lexicon(x, xp, dec.w, 2, C, L, eos, t, seg[:1])
    with pytest.raises(ValueError, match="segments"):
        dec.beam_decode(x, 2, eos, lexicon=trie, segments=[0, 5])                    # host segments are checked before upload
    torch.cuda.synchronize()                                                           # nothing was launched
    e = dec.beam_decode(torch.zeros((0, 8, 256), device=x.device), 3, eos, path_probs=True, lexicon=trie,
                        segments=torch.zeros((0,), dtype=torch.int32, device=x.device))
    assert e.symbols.shape == (0, 3, L) and e.scores.shape == e.lengths.shape == e.words.shape == (0, 3)
    assert e.path_probs.shape == (0, L, C) and e.words.is_cuda and e.words.dtype == torch.int32


# ------------------------------------------------------------------ the recognizer head and the driver
def _head(opts=()):
    """the shipped recognizer head with synthetic weights (the output layer as generated: a constrained search is forced along
    words the model finds unlikely, and a sharpened layer would push their probabilities below float32's normal range)"""
    from glass_amd.config import get_glass_cfg
    from glass_amd.modeling.recognition.recognizer_head_v2 import RecognizerRCNNHeadV3
    from glass_amd.structures.core import ShapeSpec
    from glass_amd.utils.synth import make_state_dict
    cfg = get_glass_cfg(os.path.join(ROOT, "configs", "glass_icdar15_mi355x.yaml"), ["MODEL.DEVICE", "cuda:0"] + list(opts))
    head = RecognizerRCNNHeadV3(cfg, ShapeSpec(channels=256))
    head.import_weights(dict(make_state_dict(1234, parts=("recog",))), G._dev(), "roi_heads.recognizer_head.")
    return head


LEX = {"left": ["car", "Card", "go", "X1", "stop"], "right": ["Hello", "he", "42", "zebra"]}


def test_head_set_lexicon():
    """random fused features [5,8,32,256] over two images with different segments"""
    from glass_amd.evaluation.lexicon import LexiconMatcher, LexiconTrie
    g = torch.Generator(device="cpu")
    g.manual_seed(77)
    x = torch.randn((5, 8, 32, 256), generator=g).to(G._dev())
    roi_image = torch.tensor([0, 0, 0, 1, 1], dtype=torch.int32, device=G._dev())
    keys = ["right", "right", "right", "left", "left"]                              # image 0 -> segment 1, image 1 -> segment 0
    h = _head(["MODEL.ROI_RECOGNIZER_HEAD.BEAM_WIDTH", 3])
    trie = LexiconTrie(LEX, h.text_encoder, h.decoder.max_word_len, h.beam_eos, device=G._dev())
    image_segments = torch.tensor([1, 0], dtype=torch.int32).to(G._dev())
    free = h.forward_nhwc(x, roi_image, 2)
    h.set_lexicon(trie, image_segments)
    p = h.forward_nhwc(x, roi_image, 2)
    enc = h.encoder.forward_nhwc(h.backbone.forward_nhwc(x), rnn="steps")
    r = h.decoder.beam_decode(enc, 3, h.beam_eos, path_probs=True, lexicon=trie,
                              segments=torch.tensor([1, 1, 1, 0, 0], dtype=torch.int32).to(G._dev()))
    assert torch.equal(p, r.path_probs)
    texts, scores = G._decode_rows(h, p)
    words = r.words[:, 0].cpu().tolist()
    best = r.scores[:, 0].cpu().double().numpy()
    print(f"[lexbeam] head: {texts} {scores.tolist()} words {words} scores {best.tolist()}")
    for i, (text, key) in enumerate(zip(texts, keys)):
        assert words[i] >= 0 and text.upper() == trie.upper[words[i]]
        assert text.upper() in [w.upper() for w in LEX[key]], (i, text)
    assert (np.abs(scores - np.exp(best)) <= 1e-4 * np.exp(best)).all()
    pairs = {k: {w.upper(): w for w in v} for k, v in LEX.items()}
    assert [dist for _, dist in LexiconMatcher(LEX, pairs, device=G._dev()).match(texts, keys)] == [0] * 5
    assert not torch.equal(p, free)
    h.set_lexicon(None)
    assert torch.equal(h.forward_nhwc(x, roi_image, 2), free)                        # switched off: bit for bit
    # ---- with BEAM_DISTRIBUTIONS: the full rows are a forced replay of the best hypothesis
    hd = _head(["MODEL.ROI_RECOGNIZER_HEAD.BEAM_WIDTH", 3, "MODEL.ROI_RECOGNIZER_HEAD.BEAM_DISTRIBUTIONS", True])
    hd.set_lexicon(trie, image_segments)
    rows, dist = hd.forward_nhwc(x, roi_image, 2)
    assert torch.equal(rows, p)
    want = hd.decoder.score(enc, r.symbols[:, 0].contiguous(), r.lengths[:, 0].contiguous(), eos=h.beam_eos, probs=True).probs
    assert torch.equal(dist, want)
    # ---- an image whose segment is empty: all-zero rows
    none = LexiconTrie({"a": [], "b": LEX["left"]}, h.text_encoder, h.decoder.max_word_len, h.beam_eos, device=G._dev())
    h.set_lexicon(none, torch.tensor([0, 1], dtype=torch.int32).to(G._dev()))
    z = h.forward_nhwc(x, roi_image, 2)
    assert not z[:3].any() and z[3:].any()


def test_driver_with_per_image_lexicons():
    """inference_on_dataset(lexicon=trie, lexicon_key=...) on two small synthetic images with per-image word lists: every
    surviving word's text is a word of its own image's list"""
    import glass_amd
    from glass_amd.config import get_glass_cfg
    from glass_amd.data import DatasetMapper
    from glass_amd.evaluation import inference_on_dataset
    from glass_amd.evaluation.lexicon import LexiconTrie
    from glass_amd.utils.synth import make_image, make_state_dict
    cfg = get_glass_cfg(os.path.join(ROOT, "configs", "glass_icdar15_mi355x.yaml"),
                        ["MODEL.DEVICE", "cuda:0", "INPUT.MIN_SIZE_TEST", 128, "INPUT.MAX_SIZE_TEST", 1000,
                         "POST_PROCESSING.TEXT_THRESHOLD", 0.0, "POST_PROCESSING.DETECT_THRESHOLD", 0.0,
                         "POST_PROCESSING.LOW_CONFIDENCE", 0.0, "POST_PROCESSING.VALID_CONFIDENCE", 0.0,
                         "MODEL.ROI_RECOGNIZER_HEAD.BEAM_WIDTH", 3])
    model = glass_amd.build_model(cfg)
    model.load_state_dict(make_state_dict(1234))
    head = model.roi_heads.recognizer_head
    lex = {"img_0.jpg": LEX["left"], "img_1.jpg": LEX["right"]}
    trie = LexiconTrie(lex, head.text_encoder, head.decoder.max_word_len, head.beam_eos, device=G._dev())
    dds = [{"file_name": f"img_{i}.jpg", "image": make_image(i, 96, 128).numpy(), "annotations": []} for i in range(2)]
    mapper = DatasetMapper(cfg, device="cuda:0", fused=True)
    outs = inference_on_dataset(model, dds, mapper, batch_size=8, lexicon=trie, lexicon_key=lambda inp: inp["file_name"])
    assert head.lexicon is None and head.image_segments is None                      # the head is handed back as it was
    survived = 0
    for dd, o in zip(dds, outs):
        inst = o["instances"]
        if len(inst) == 0:
            continue
        texts, _ = G._decode_rows(head, inst.pred_text_prob)
        print(f"[lexbeam] driver: {dd['file_name']}: {texts}")
        allowed = [w.upper() for w in lex[dd["file_name"]]]
        assert all(t.upper() in allowed for t in texts), (dd["file_name"], texts)
        survived += len(texts)
    assert survived > 0, "no word survived: the case checks nothing"
