"""GPU: forced decoding on the device (glass_forced_decode, ASTER_V2.score / forward(labels) / beam_decode(distributions=),
MODEL.ROI_RECOGNIZER_HEAD.BEAM_DISTRIBUTIONS) against the float64 forced replay of tests/forced_cases.py, the device beam
search, a forced replay driven through the existing step kernel, the reference's golden, and through the recognizer head and
the whole model.  No test feeds an out-of-range symbol to the GPU: the in-kernel guard is read, not provoked."""
import math
import os

import numpy as np
import pytest
import torch

import beam_cases as BC
import forced_cases as FC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-4                      # tests/test_gpu_beam_search.py's TOL, for the same arithmetic


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _decoder(sd, C, L):
    from glass_amd.modeling.recognition.recognizer_decoder import ASTER_V2
    from glass_amd.structures.core import ShapeSpec
    dec = ASTER_V2(BC.decoder_cfg(C, L), ShapeSpec(channels=256))
    dec.import_weights(sd, _dev(), BC.PRE)
    return dec


def _kernel_driven_forced(dec, x, targets, lengths):
    """the forced replay with every decoder step computed by the existing kernel (`K.attention_decode_step`, three launches
    per step) on inflated inputs: targets [B,n,L] long (CPU), lengths [B,n] -> logits [B,n,L,C] float32 (CPU), zero from the
    length on"""
    from glass_amd.ops import native as K
    B, T, D = x.shape
    _, n, L = targets.shape
    C = dec.num_classes
    xproj = K.linear(x.view(B * T, D), dec.w["xW"], dec.w["xB"]).view(B, T, D)
    xi = x.unsqueeze(1).expand(B, n, T, D).reshape(B * n, T, D).contiguous()
    xpi = xproj.unsqueeze(1).expand(B, n, T, D).reshape(B * n, T, D).contiguous()
    state = torch.zeros((B * n, D), dtype=torch.float32, device=x.device)
    y_prev = torch.zeros((B * n,), dtype=torch.int32, device=x.device)
    tg = targets.reshape(B * n, L).to(torch.int32).to(x.device)
    rows = []
    for t in range(L):
        logits, _, state = K.attention_decode_step(xi, xpi, dec.w, state, y_prev, C)
        rows.append(logits)
        y_prev = tg[:, t].contiguous()
    out = torch.stack(rows, 1).view(B, n, L, C).cpu()
    dead = torch.arange(L).view(1, 1, L) >= lengths.unsqueeze(2)
    out[dead] = 0.0
    return out


_RUNS = {}


def _run(case):
    """everything the tests of one generated case share, computed once: the decoder, the inputs on the device, per target set
    the device result (host targets: validated, uploaded) and the kernel-driven replay's logits"""
    if case[0] not in _RUNS:
        name, B, k, T, L, C, seed = case
        d = FC.case_data(case)
        dec = _decoder(d["sd"], C, L)
        x = d["x"].to(_dev())
        got, drv = {}, {}
        for s in FC.SETS:
            tg, ln = d["sets"][s]
            r = dec.score(x, tg, ln, eos=0, probs=True, logits=True)
            got[s] = type(r)(*[t.cpu() for t in r])
            drv[s] = _kernel_driven_forced(dec, x, tg, d["f64"][s]["lengths"])
        _RUNS[case[0]] = dict(dec=dec, x=x, got=got, drv=drv, data=d)
    return _RUNS[case[0]]


def _maxabs(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max()) if a.size else 0.0


@pytest.mark.parametrize("case", BC.CASES, ids=[c[0] for c in BC.CASES])
def test_records_against_the_float64_replay(case):
    """per target set: lengths exact; step_logp and probs within TOL of the float64 replay; every entry at and beyond the
    length exactly zero; out_scores bit for bit the sequential float32 sum of the call's own step_logp[:length] (numpy, on
    the host) - the contract, so unlikely targets need no score tolerance"""
    name, B, k, T, L, C, seed = case
    r = _run(case)
    for s in FC.SETS:
        got, f = r["got"][s], r["data"]["f64"][s]
        assert got.step_logp.shape == (B, k, L) and got.scores.shape == (B, k) and got.lengths.shape == (B, k)
        assert got.probs.shape == (B, k, L, C) and got.logits.shape == (B, k, L, C) and got.lengths.dtype == torch.int32
        assert torch.equal(got.lengths.long(), f["lengths"]), (name, s)
        d_lp, d_p = _maxabs(got.step_logp, f["step_logp"]), _maxabs(got.probs, f["probs"])
        want = FC.f32_sequential_sum(got.step_logp.numpy(), got.lengths.numpy())
        same = np.array_equal(got.scores.numpy().view(np.int32), want.view(np.int32))
        print(f"[forced] {name}/{s}: max |dstep_logp| {d_lp:.3e}, max |dprobs| {d_p:.3e} vs float64; lowest step_logp "
              f"{float(got.step_logp.min()):.2f}; scores == sequential float32 sum: {same}")
        assert d_lp < TOL and d_p < TOL, (name, s)
        dead = torch.arange(L).view(1, 1, L) >= got.lengths.long().unsqueeze(2)
        for t in (got.step_logp, got.probs, got.logits):
            assert not t[dead].any(), (name, s)
        assert same, (name, s)


@pytest.mark.parametrize("case", BC.CASES, ids=[c[0] for c in BC.CASES])
def test_against_the_beam_search_on_the_device(case):
    """set (a) from the device's own search: forced scores of all k hypotheses within TOL of `beam_decode`'s; the "best"
    distributions at symbols[t] within TOL of the path rows, rows summing to 1 up to the length and zero after it; "all" holds
    "best" as its hypothesis 0, bit for bit"""
    name, B, k, T, L, C, seed = case
    r = _run(case)
    dec, x = r["dec"], r["x"]
    bs = dec.beam_decode(x, k, 0, path_probs=True, distributions="best")
    ba = dec.beam_decode(x, k, 0, distributions="all")
    assert bs.distributions.shape == (B, L, C) and ba.distributions.shape == (B, k, L, C) and ba.path_probs is None
    assert torch.equal(ba.distributions[:, 0], bs.distributions)
    assert torch.equal(ba.symbols, bs.symbols) and torch.equal(ba.scores, bs.scores)
    f = dec.score(x, bs.symbols, bs.lengths)                                  # device tensors: passed through
    finite = ~torch.isneginf(bs.scores)
    assert finite.all(), "k <= C: every hypothesis of these cases exists"
    assert torch.equal(f.lengths, bs.lengths)
    d = _maxabs(f.scores.cpu(), bs.scores.cpu())
    print(f"[forced] {name}: forced scores vs beam_decode's, all {B * k} hypotheses: max |dscore| {d:.3e} (zero: {d == 0.0})")
    assert d < TOL
    dist, path, sym, ln = bs.distributions.cpu(), bs.path_probs.cpu(), bs.symbols[:, 0].cpu().long(), bs.lengths[:, 0].cpu().long()
    at = dist.gather(2, sym.unsqueeze(2)).squeeze(2)
    live = torch.arange(L).view(1, L) < ln.unsqueeze(1)
    d_path = _maxabs(at[live], path.max(2).values[live])
    print(f"[forced] {name}: distributions[t, symbols[t]] vs path rows: max |d| {d_path:.3e}")
    assert d_path < TOL
    assert _maxabs(dist.sum(2)[live], 1.0) < TOL and not dist[~live].any()


def test_minus_inf_hypotheses_get_length_zero_and_all_zero_rows(monkeypatch):
    """a search that returns fewer than k hypotheses marks the rest with score -inf; the replay gives them length 0 (torch ops
    on the device) and therefore all-zero rows.  With k <= C the search itself always fills its k slots, so the -inf scores
    are put into the search's result here, between the two calls of `beam_decode`."""
    from glass_amd.ops import native as K
    case = BC.CASES[1]
    name, B, k, T, L, C, seed = case
    r = _run(case)
    inner = K.beam_search

    def with_missing(*a, **kw):
        out = inner(*a, **kw)
        out[1][:, -1] = -math.inf
        out[1][0, 0] = -math.inf
        return out
    monkeypatch.setattr(K, "beam_search", with_missing)
    ba = r["dec"].beam_decode(r["x"], k, 0, distributions="all")
    bb = r["dec"].beam_decode(r["x"], k, 0, distributions="best")
    monkeypatch.undo()
    ref = r["dec"].beam_decode(r["x"], k, 0, distributions="all")
    assert not ba.distributions[:, -1].any() and not ba.distributions[0, 0].any() and not bb.distributions[0].any()
    assert torch.equal(ba.distributions[1:, 0], ref.distributions[1:, 0]) and ref.distributions[0, 0].any()
    assert torch.equal(bb.distributions[1:], ref.distributions[1:, 0])


@pytest.mark.parametrize("case", BC.CASES, ids=[c[0] for c in BC.CASES])
def test_logits_against_the_kernel_driven_replay_and_float64(case):
    """Logits, per target set: within TOL of a forced replay driven through the parent's kernel (`K.attention_decode_step` per
    step on inflated inputs); against float64 the bound is TWICE the difference that kernel-driven replay itself shows to
    float64 on the same case, measured here.  Measured on an MI355X (max over the three target sets; |logit| up to ~1e2), per
    case: forced vs kernel-driven replay | forced vs float64 | kernel-driven replay vs float64 (the bound is twice this)
      b1_k1_t7_l1           0 (bit-equal) | 1.5e-5 | 1.5e-5
      b3_k2_t32_l26         0 (bit-equal) | 3.6e-5 | 3.6e-5
      b17_k5_t64_l64        0 (bit-equal) | 5.7e-5 | 5.7e-5
      b3_k5_t7_l26_c5       0 (bit-equal) | 4.2e-5 | 4.2e-5
      b3_k16_t32_l26_c256   0 (bit-equal) | 5.0e-5 | 5.0e-5
      b32_k16_t7_l6_rows512 0 (bit-equal) | 8.1e-5 | 8.1e-5
    (the reference golden, test_forward_with_labels_against_the_reference_golden: 3.8e-5 for both, forced = kernel-driven)"""
    name, B, k, T, L, C, seed = case
    r = _run(case)
    for s in FC.SETS:
        got, drv, f = r["got"][s].logits, r["drv"][s], r["data"]["f64"][s]["logits"]
        d_drv, d_f64, ref_f64 = _maxabs(got, drv), _maxabs(got, f), _maxabs(drv, f)
        print(f"[forced] {name}/{s}: logits vs kernel-driven replay max |d| {d_drv:.3e} (bit-equal: {torch.equal(got, drv)}); "
              f"vs float64 {d_f64:.3e}; kernel-driven replay vs float64 {ref_f64:.3e} (bound {2 * ref_f64:.3e})")
        assert d_drv < TOL, (name, s)
        assert d_f64 <= 2 * ref_f64, (name, s)


def test_forward_with_labels_against_the_reference_golden(golden_dir):
    """`ASTER_V2.forward(features, labels)` = the reference's AttentionRecognitionHead.forward (tests/golden/forced_decode.npz:
    x [3,32,256], 26 steps, 97 classes, no stop): logits [3,26,97]; the bound is twice the difference the kernel-driven replay
    shows to the golden, measured here; the `labels is None` path still returns the greedy decoder's probabilities"""
    g = np.load(os.path.join(golden_dir, "forced_decode.npz"), allow_pickle=False)
    dec = _decoder(BC.decoder_sd(97, int(g["seed"]), float(g["fc_scale"]), float(g["bias0"])), 97, 26)
    x, labels = torch.from_numpy(g["x"]).to(_dev()), torch.from_numpy(g["labels"])
    got = dec.forward(x, labels)
    assert got.shape == (3, 26, 97) and got.is_cuda
    assert torch.equal(dec.forward(x, labels.to(_dev())), got)                # device labels: passed through, same rows
    drv = _kernel_driven_forced(dec, x, labels[:, 1:].unsqueeze(1), torch.full((3, 1), 26))[:, 0]
    want = torch.from_numpy(g["logits"])
    d, ref = _maxabs(got.cpu(), want), _maxabs(drv, want)
    print(f"[forced] golden: forward(features, labels) vs reference max |dlogit| {d:.3e}; kernel-driven replay vs reference "
          f"{ref:.3e} (bound {2 * ref:.3e}); vs kernel-driven replay {_maxabs(got.cpu(), drv):.3e}")
    assert d <= 2 * ref and _maxabs(got.cpu(), drv) < TOL
    p = dec.forward(x)
    assert p.shape == (3, 26, 97) and float(p.min()) >= 0.0 and float(p.sum(2).max()) < 1.0 + TOL


def test_two_runs_are_bit_identical():
    case = BC.CASES[2]
    r = _run(case)
    tg, ln = r["data"]["sets"]["perturb"]
    again = r["dec"].score(r["x"], tg, ln, eos=0, probs=True, logits=True)
    for a, b in zip(again, r["got"]["perturb"]):
        assert torch.equal(a.cpu().view(torch.int32), b.view(torch.int32))


def test_targets_without_the_sequence_axis_and_optional_rows():
    case = BC.CASES[1]
    r = _run(case)
    tg, _ = r["data"]["sets"]["perturb"]
    one = r["dec"].score(r["x"], tg[:, 0])
    assert one.probs is None and one.logits is None and one.step_logp.shape == tg[:, 0].shape and one.scores.shape == (tg.shape[0],)
    assert torch.equal(one.step_logp.cpu(), r["got"]["perturb"].step_logp[:, 0])
    assert torch.equal(one.scores.cpu(), r["got"]["perturb"].scores[:, 0])


def test_limits_raise_before_any_launch_and_empty_batch():
    from glass_amd import _lib
    from glass_amd._lib import GlassLibraryError
    from glass_amd.ops import native as K
    dec = _decoder(BC.decoder_sd(97), 97, 26)
    x = BC.rand_x(2, 8, 5).to(_dev())
    xp = torch.zeros_like(x)
    tg = lambda n, L: torch.zeros((2, n, L), dtype=torch.int32, device=_dev())
    with pytest.raises(GlassLibraryError, match="n=17"):
        K.forced_decode(x, xp, dec.w, tg(17, 26), None, 97, 26, 0)
    with pytest.raises(GlassLibraryError, match="max_len=65"):
        K.forced_decode(x, xp, dec.w, tg(2, 65), None, 97, 65, 0)
    x65 = torch.zeros((2, 65, 256), device=_dev())
    with pytest.raises(GlassLibraryError, match="T=65"):
        K.forced_decode(x65, x65, dec.w, tg(2, 26), None, 97, 26, 0)
    with pytest.raises(GlassLibraryError):
        K.forced_decode(x, xp[:, :4], dec.w, tg(2, 26), None, 97, 26, 0)
    L = _lib.lib()
    real = L.glass_forced_decode_workspace_bytes
    try:
        L.glass_forced_decode_workspace_bytes = lambda *a: 64
        with pytest.raises(GlassLibraryError, match="workspace too small"):
            K.forced_decode(x, xp, dec.w, tg(2, 26), None, 97, 26, 0)
    finally:
        L.glass_forced_decode_workspace_bytes = real
    torch.cuda.synchronize()                                   # nothing was launched: no error surfaces here either
    e = dec.score(torch.zeros((0, 8, 256), device=_dev()), torch.zeros((0, 3, 26), dtype=torch.long), probs=True, logits=True)
    assert e.step_logp.shape == (0, 3, 26) and e.scores.shape == (0, 3) and e.lengths.shape == (0, 3)
    assert e.probs.shape == (0, 3, 26, 97) and e.logits.shape == (0, 3, 26, 97) and e.step_logp.is_cuda


# ------------------------------------------------------------------ the recognizer head and the whole model
def _head(opts=()):
    """the head of tests/test_gpu_beam_search.py: sharper output layer, a stop symbol that ends words at different steps"""
    from glass_amd.config import get_glass_cfg
    from glass_amd.modeling.recognition.recognizer_head_v2 import RecognizerRCNNHeadV3
    from glass_amd.structures.core import ShapeSpec
    from glass_amd.utils.synth import make_state_dict
    cfg = get_glass_cfg(os.path.join(ROOT, "configs", "glass_icdar15_mi355x.yaml"), ["MODEL.DEVICE", "cuda:0"] + list(opts))
    head = RecognizerRCNNHeadV3(cfg, ShapeSpec(channels=256))
    stop, seven = head.text_encoder.character.index("[s]"), head.text_encoder.character.index("7")
    sd = dict(make_state_dict(1234, parts=("recog",)))
    sd[BC.Q + "fc.weight"] = sd[BC.Q + "fc.weight"] * 6.0
    sd[BC.Q + "fc.bias"] = sd[BC.Q + "fc.bias"].clone()
    sd[BC.Q + "fc.weight"][stop] = sd[BC.Q + "fc.weight"][seven]
    sd[BC.Q + "fc.bias"][stop] = sd[BC.Q + "fc.bias"][seven] + 0.5
    head.import_weights(sd, _dev(), "roi_heads.recognizer_head.")
    return head


W5 = ["MODEL.ROI_RECOGNIZER_HEAD.BEAM_WIDTH", 5]
DIST = ["MODEL.ROI_RECOGNIZER_HEAD.BEAM_DISTRIBUTIONS", True]


def test_head_beam_distributions():
    """random fused features [5,8,32,256] over two images, BEAM_WIDTH 5: with BEAM_DISTRIBUTIONS the path rows are
    `torch.equal` to the run without it; the distribution rows sum to 1 within TOL up to the length, are zero after it, and
    their arg-max row entry at the emitted symbol is the path row's entry within TOL"""
    g = torch.Generator(device="cpu")
    g.manual_seed(77)
    x = torch.randn((5, 8, 32, 256), generator=g).to(_dev())
    roi_image = torch.tensor([0, 0, 0, 1, 1], dtype=torch.int32, device=_dev())
    off = _head(W5).forward_nhwc(x, roi_image, 2)
    h = _head(W5 + DIST)
    on = h.forward_nhwc(x, roi_image, 2)
    assert torch.is_tensor(off) and isinstance(on, tuple) and len(on) == 2
    rows, dist = on
    assert torch.equal(rows, off) and dist.shape == rows.shape
    enc = h.encoder.forward_nhwc(h.backbone.forward_nhwc(x), rnn="steps")
    r = h.decoder.beam_decode(enc, 5, h.beam_eos, path_probs=True)
    assert torch.equal(r.path_probs, rows)
    ln = r.lengths[:, 0].cpu().long()
    live = torch.arange(26).view(1, 26) < ln.unsqueeze(1)
    dist, rows = dist.cpu(), rows.cpu()
    print(f"[forced] head: lengths {ln.tolist()}, max |row sum - 1| {_maxabs(dist.sum(2)[live], 1.0):.3e}")
    assert (ln < 26).any() and (ln > 1).any(), "the words do not exercise the stop"
    assert _maxabs(dist.sum(2)[live], 1.0) < TOL and not dist[~live].any()
    sym = r.symbols[:, 0].cpu().long()
    assert _maxabs(dist.gather(2, sym.unsqueeze(2)).squeeze(2)[live], rows.max(2).values[live]) < TOL
    # the reference call surface attaches both fields per image
    from glass_amd.structures.core import Instances, RotatedBoxes
    inst = []
    for c in (3, 2):
        i = Instances((64, 64))
        i.pred_boxes = RotatedBoxes(torch.zeros((c, 5), device=_dev()))
        inst.append(i)
    out = h(x.permute(0, 3, 1, 2).contiguous(), inst)
    assert torch.equal(torch.cat([i.pred_text_prob for i in out]), on[0]) and torch.equal(torch.cat([i.pred_text_dist for i in out]), on[1])


def _runner(extra):
    from glass_amd.config import get_glass_cfg
    from glass_amd.inference.glass_runner import GlassRunner
    from glass_amd.utils.synth import make_state_dict
    cfg = get_glass_cfg(os.path.join(ROOT, "configs", "glass_icdar15_mi355x.yaml"),
                        ["INPUT.MIN_SIZE_TEST", 160, "INPUT.MAX_SIZE_TEST", 200, "MODEL.DEVICE", "cuda:0",
                         "POST_PROCESSING.TEXT_THRESHOLD", 0.0, "POST_PROCESSING.DETECT_THRESHOLD", 0.0,
                         "POST_PROCESSING.LOW_CONFIDENCE", 0.0, "POST_PROCESSING.VALID_CONFIDENCE", 0.0] + W5 + list(extra))
    return GlassRunner(None, None, cfg=cfg, state_dict=make_state_dict(1234), post_process=True)


def test_runner_end_to_end_with_beam_distributions():
    """GlassRunner with BEAM_WIDTH 5 on a small synthetic image, with and without BEAM_DISTRIBUTIONS: pred_text_prob, the
    texts, the text scores and the boxes are `torch.equal` / equal; pred_text_dist rows sum to 1 within TOL up to the stop
    and are zero after it; the records' `character_probs` are those rows; WeightedLexiconMatcher.match on the records equals
    `find_match_word_weighted` word for word and bit for bit on a small synthetic lexicon"""
    from glass_amd.evaluation import WeightedLexiconMatcher, find_match_word_weighted
    from glass_amd.evaluation.text_evaluator import instances_to_coco_json
    from glass_amd.utils.synth import make_image
    img = make_image(0, 120, 150).numpy()
    off = _runner([])(img)
    run = _runner(DIST)
    on = run(img)
    assert len(off) > 0 and len(on) == len(off), "no word survived: the case checks nothing"
    assert not off.has("pred_text_dist") and on.has("pred_text_dist")
    assert torch.equal(on.pred_text_prob, off.pred_text_prob) and torch.equal(on.pred_boxes.tensor, off.pred_boxes.tensor)
    assert on.pred_texts == off.pred_texts and torch.equal(torch.as_tensor(on.pred_text_scores), torch.as_tensor(off.pred_text_scores))
    rows, dist = on.pred_text_prob.cpu(), on.pred_text_dist.cpu()
    assert dist.shape == rows.shape
    live = rows.sum(2) > 0                                   # a path row below the length holds exp(.) > 0, zero after it
    assert _maxabs(dist.sum(2)[live], 1.0) < TOL and not dist[~live].any() and live.any()
    enc = run.text_encoder
    recs = instances_to_coco_json(on, "img", enc)
    kept = [i for i, t in enumerate(get_texts(on, enc)) if len(t) > 0]
    assert recs and len(recs) == len(kept)
    for rec, i in zip(recs, kept):
        assert np.array_equal(np.asarray(rec["character_probs"]), dist[i].double().numpy())
    words = [r["rec"] for r in recs if all(ord(c) < 128 for c in r["rec"])]
    scores = [r["character_probs"] for r in recs if all(ord(c) < 128 for c in r["rec"])]
    # near misses of the words, not the words themselves: the winners are decided by the weighted costs, i.e. by the rows
    lexicon = sorted(({w[:-1] + "x" for w in words if len(w) > 1} | {w[1:] for w in words if len(w) > 2}
                      | {w[:len(w) // 2] + "Q" + w[len(w) // 2 + 1:] for w in words} | {"apple", "Orange", "street", "EXIT", "a"})
                     - set(words))
    pairs = {w.upper(): w for w in lexicon}
    lexicon = list(pairs.values())
    m = WeightedLexiconMatcher(lexicon, pairs, enc, device=_dev())
    got = m.match(words, scores=scores)
    want = [find_match_word_weighted(w, lexicon, pairs, s, enc) for w, s in zip(words, scores)]
    print(f"[forced] runner: {len(on)} words {on.pred_texts}; lexicon of {len(lexicon)}; matches {got}")
    assert words and got == want and any(d > 0 for _, d in got)


def get_texts(instances, enc):
    from glass_amd.postprocess.post_processor_academic import get_instances_text
    return get_instances_text(instances.pred_text_prob, enc, True)[0]
