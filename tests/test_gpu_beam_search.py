"""GPU: the device beam search (glass_beam_search, ASTER_V2.beam_decode, MODEL.ROI_RECOGNIZER_HEAD.BEAM_WIDTH) against the
reference's golden, the host path `ASTER_V2.beam_search`, the float64 replay of tests/beam_cases.py, the greedy decoder, and
through the recognizer head and the whole model."""
import math
import os

import numpy as np
import pytest
import torch

import beam_cases as BC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Symbols are compared exactly, so no selection may be a near-tie: every item's smallest selection gap and smallest gap
# between neighbouring final scores (float64 replay) must exceed MARGIN = ten times the largest score difference between the
# host path `ASTER_V2.beam_search` and the float64 replay on these same inputs (measured on an MI355X without the device
# search, figures in test_all_hypotheses_against_host_path_and_replay).  Ten times, because the device's log-softmax and
# torch's may differ by rounding in either direction at each of up to 64 steps.
MARGIN = 10 * 3.6e-5
TOL = 1e-4


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _decoder(sd, C, L):
    from glass_amd.modeling.recognition.recognizer_decoder import ASTER_V2
    from glass_amd.structures.core import ShapeSpec
    dec = ASTER_V2(BC.decoder_cfg(C, L), ShapeSpec(channels=256))
    dec.import_weights(sd, _dev(), BC.PRE)
    return dec


def _kernel_driven_replay(dec, x, k, C, L, eos):
    """the float64 search of beam_cases with every decoder step computed by the existing kernel on inflated inputs"""
    from glass_amd.ops import native as K
    B, T, D = x.shape
    xproj = K.linear(x.view(B * T, D), dec.w["xW"], dec.w["xB"]).view(B, T, D)
    xi = x.unsqueeze(1).expand(B, k, T, D).reshape(B * k, T, D).contiguous()
    xpi = xproj.unsqueeze(1).expand(B, k, T, D).reshape(B * k, T, D).contiguous()

    def step(state, y_prev):
        logits, _, state = K.attention_decode_step(xi, xpi, dec.w, state, y_prev.to(torch.int32).to(x.device), C)
        return logits, state
    return BC.replay_with(step, torch.zeros((B * k, D), dtype=torch.float32, device=x.device), B, k, C, L, eos)


_RUNS = {}


def _run(case):
    """everything the tests of one generated case share, computed once: inputs, the host path, both replays, the device search"""
    if case[0] not in _RUNS:
        name, B, k, T, L, C, seed = case
        sd = BC.decoder_sd(C)
        dec = _decoder(sd, C, L)
        xc = BC.rand_x(B, T, seed)
        x = xc.to(_dev())
        host_p, host_s = dec.beam_search(x, k, 0)
        f64 = BC.replay(sd, xc, k, C, L, 0)
        drv = _kernel_driven_replay(dec, x, k, C, L, 0)
        got = dec.beam_decode(x, k, 0, path_probs=True)
        _RUNS[case[0]] = dict(dec=dec, x=x, host_p=host_p.cpu(), host_s=host_s.cpu().double(), f64=f64, drv=drv,
                              got=type(got)(*[t.cpu() for t in got]))
    return _RUNS[case[0]]


def _absdiff(a, b):
    """largest |a - b| over entries where either is finite; entries that are -inf on both sides agree"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    both_ninf = np.isneginf(a) & np.isneginf(b)
    d = np.where(both_ninf, 0.0, np.abs(np.where(both_ninf, 0.0, a) - np.where(both_ninf, 0.0, b)))
    return float(d.max()) if d.size else 0.0


def test_golden(golden_dir):
    """the reference's own function (tests/golden/beam_search.npz): best symbols identical, scores within 1e-4"""
    g = np.load(os.path.join(golden_dir, "beam_search.npz"), allow_pickle=False)
    dec = _decoder(BC.decoder_sd(97, 1234, float(g["fc_scale"]), float(g["bias0"])), 97, 26)
    for name in ("a", "b", "c"):
        x, width = torch.from_numpy(g[f"{name}:x"]).to(_dev()), int(g[f"{name}:width"])
        r = dec.beam_decode(x, width, 0)
        assert r.symbols.shape == (x.shape[0], width, 26) and r.symbols.dtype == torch.int32 and r.path_probs is None
        assert r.symbols[:, 0].cpu().tolist() == g[f"{name}:p"].tolist(), name
        d = _absdiff(r.scores[:, 0].cpu(), g[f"{name}:s"])
        print(f"[beam] golden {name}: width {width}, max |dscore| {d:.3e}")
        assert d < TOL, name


@pytest.mark.parametrize("case", BC.CASES, ids=[c[0] for c in BC.CASES])
def test_all_hypotheses_against_host_path_and_replay(case):
    """Seeded inputs, synthetic decoder weights for the case's C with the golden's sharper output layer and boosted <eos>.
      * best beam = `ASTER_V2.beam_search`'s up to its length (positions from the length on hold, by the reference's design,
        what the result slot held before; there the host path depends on how torch.topk orders -inf ties), score within 1e-4;
      * all k hypotheses (every position), lengths and the best hypothesis's path rows = the replay's, where the replay takes
        each step's logits from the existing kernel `K.attention_decode_step` and searches in float64 by the stated rule;
        scores within 1e-4 of that replay and of the all-float64 one.
    No item is excluded: every item's gaps (all-float64 replay) must exceed MARGIN.  Measured on an MI355X, per case: largest
    |dscore| host path vs float64 replay (its largest value, 3.6e-5, sets MARGIN = 3.6e-4) | smallest selection gap |
    smallest final-score gap || device search vs host path | vs kernel-driven replay | vs float64 replay
      b1_k1_t7_l1           3.2e-8 | 1.1e+1 | -      || 0      | 3.2e-8 | 3.2e-8
      b3_k2_t32_l26         2.9e-6 | 5.7e-2 | 7.8e-2 || 7.2e-7 | 6.0e-7 | 1.8e-5
      b17_k5_t64_l64        3.6e-5 | 2.4e-3 | 2.2e-3 || 1.4e-6 | 2.7e-6 | 4.7e-5
      b3_k5_t7_l26_c5       6.8e-7 | 2.0e-1 | 1.5e+0 || 0      | 1.9e-6 | 1.4e-5
      b3_k16_t32_l26_c256   7.8e-6 | 8.6e-3 | 1.1e-2 || 4.8e-7 | 3.0e-6 | 6.0e-5
      b32_k16_t7_l6_rows512 9.0e-6 | 3.8e-3 | 1.2e-3 || 3.6e-7 | 1.7e-6 | 5.8e-5
      b2_k3_t7_l6_c13       2.9e-6 | 3.9e-1 | 1.7e+0 || 3.7e-9 | 2.4e-7 | 1.6e-5
      b2_k4_t7_l6_c13       1.0e-5 | 1.1e+0 | 1.4e+0 || 1.2e-7 | 5.7e-7 | 2.5e-5
    (the float64 column covers all k hypotheses, the host columns the best one; the golden's three cases: 6.9e-6, 6.0e-6,
    1.0e-5 against the reference's scores)"""
    name, B, k, T, L, C, seed = case
    r = _run(case)
    f64, drv, got = r["f64"], r["drv"], r["got"]
    ref_pair = _absdiff(r["host_s"], f64["scores"][:, 0])
    gap = min(float(f64["sel_gap"].min()), float(f64["score_gap"].min()))
    print(f"[beam] {name}: host beam_search vs float64 replay max |dscore| {ref_pair:.3e}; smallest selection gap "
          f"{float(f64['sel_gap'].min()):.3e}, smallest final-score gap {float(f64['score_gap'].min()):.3e}; device vs host "
          f"{_absdiff(got.scores[:, 0], r['host_s']):.3e}, vs kernel-driven replay {_absdiff(got.scores, drv['scores']):.3e}, "
          f"vs float64 replay {_absdiff(got.scores, f64['scores']):.3e}")
    assert 10 * ref_pair <= MARGIN, "MARGIN no longer covers the reference pair's own difference"
    assert gap > MARGIN, "a near-tie: choose another seed for this case, do not relax the margin"
    assert got.symbols.shape == (B, k, L) and got.scores.shape == (B, k) and got.lengths.shape == (B, k)
    assert got.path_probs.shape == (B, L, C)
    # ---- the host path
    for b in range(B):
        n = int(got.lengths[b, 0])
        assert got.symbols[b, 0, :n].tolist() == r["host_p"][b, :n].tolist(), (name, b)
    assert _absdiff(got.scores[:, 0], r["host_s"]) < TOL
    # ---- the replay
    assert torch.equal(drv["symbols"], f64["symbols"]) and torch.equal(drv["lengths"], f64["lengths"])
    assert torch.equal(got.symbols.long(), drv["symbols"]), name
    assert torch.equal(got.lengths.long(), drv["lengths"]), name
    assert _absdiff(got.scores, drv["scores"]) < TOL and _absdiff(got.scores, f64["scores"]) < TOL
    assert (torch.isneginf(got.scores) == torch.isneginf(drv["scores"])).all()
    for b in range(B):
        want = BC.path_rows(drv["symbols"][b, 0], drv["step_scores"][b, 0], drv["lengths"][b, 0], drv["scores"][b, 0], C)
        rows = got.path_probs[b].double().numpy()
        assert ((rows != 0) == (want != 0)).all(), (name, b)
        assert float(np.abs(rows - want).max()) < TOL, (name, b)


def test_width_one_is_greedy_decoding():
    """symbols = arg-max of the greedy decoder's rows up to and including each row's first <eos> (rows after the greedy
    decoder's batch-global break are zero and not compared, as in test_gpu_a_stages.py); path probabilities = its maxima"""
    sd = BC.decoder_sd(97)
    dec = _decoder(sd, 97, 26)
    x = BC.rand_x(5, 32, 220).to(_dev())        # float64 replay: lengths 13, 26, 3, 26, 1
    r = dec.beam_decode(x, 1, 0, path_probs=True)
    probs, sym, rows = dec(x).cpu().numpy(), r.symbols[:, 0].cpu().numpy(), r.path_probs.cpu().numpy()
    ended = 0
    for b in range(sym.shape[0]):
        n = int(r.lengths[b, 0])
        assert n == (int(np.argmax(sym[b] == 0)) + 1 if (sym[b] == 0).any() else sym.shape[1])
        live = probs[b, :n].sum(-1) > 0
        assert live.any()
        assert (probs[b, :n].argmax(-1)[live] == sym[b, :n][live]).all(), b
        assert (rows[b, :n].argmax(-1) == sym[b, :n]).all() and not rows[b, n:].any()
        assert float(np.abs(rows[b, :n].max(-1)[live] - probs[b, :n].max(-1)[live]).max()) < TOL
        ended += n < sym.shape[1]
    assert ended, "no row ended: the case does not exercise the stop"


def test_two_runs_are_bit_identical():
    r = _run(BC.CASES[2])
    again = r["dec"].beam_decode(r["x"], BC.CASES[2][2], 0, path_probs=True)
    for a, b in zip(again, r["got"]):
        assert torch.equal(a.cpu().view(torch.int32), b.view(torch.int32))


def test_limits_raise_before_any_launch_and_empty_batch():
    from glass_amd._lib import GlassLibraryError
    from glass_amd.ops import native as K
    dec = _decoder(BC.decoder_sd(97), 97, 26)
    x = BC.rand_x(2, 8, 5).to(_dev())
    with pytest.raises(GlassLibraryError, match="k=17"):
        dec.beam_decode(x, 17)
    with pytest.raises(GlassLibraryError, match="k=0"):
        dec.beam_decode(x, 0)
    xp = torch.zeros_like(x)
    with pytest.raises(GlassLibraryError, match="max_len=65"):
        K.beam_search(x, xp, dec.w, 2, 97, 65, 0)
    with pytest.raises(GlassLibraryError, match="k=6 .* C=5"):
        K.beam_search(x, xp, dec.w, 6, 5, 26, 0)
    x65 = torch.zeros((1, 65, 256), device=_dev())
    with pytest.raises(GlassLibraryError, match="T=65"):
        K.beam_search(x65, x65, dec.w, 2, 97, 26, 0)
    with pytest.raises(GlassLibraryError):
        K.beam_search(x, xp[:, :4], dec.w, 2, 97, 26, 0)
    torch.cuda.synchronize()                                   # nothing was launched: no error surfaces here either
    e = dec.beam_decode(torch.zeros((0, 8, 256), device=_dev()), 3, 0, path_probs=True)
    assert e.symbols.shape == (0, 3, 26) and e.scores.shape == (0, 3) and e.lengths.shape == (0, 3)
    assert e.path_probs.shape == (0, 26, 97) and e.symbols.is_cuda


# ------------------------------------------------------------------ the recognizer head and the whole model
def _head(opts=(), drop_key=False):
    from glass_amd.config import get_glass_cfg
    from glass_amd.modeling.recognition.recognizer_head_v2 import RecognizerRCNNHeadV3
    from glass_amd.structures.core import ShapeSpec
    cfg = get_glass_cfg(os.path.join(ROOT, "configs", "glass_icdar15_mi355x.yaml"), ["MODEL.DEVICE", "cuda:0"] + list(opts))
    if drop_key:
        cfg.MODEL.ROI_RECOGNIZER_HEAD.pop("BEAM_WIDTH")
    head = RecognizerRCNNHeadV3(cfg, ShapeSpec(channels=256))
    stop = head.text_encoder.character.index("[s]")
    from glass_amd.utils.synth import make_state_dict
    sd = dict(make_state_dict(1234, parts=("recog",)))
    sd[BC.Q + "fc.weight"] = sd[BC.Q + "fc.weight"] * 6.0               # as in the golden: separated beams
    sd[BC.Q + "fc.bias"] = sd[BC.Q + "fc.bias"].clone()
    # words that end, at different steps: the stop symbol takes over the output row of '7', a character these weights emit
    # often, with a bias 0.5 higher - where '7' would have been emitted the word stops
    seven = head.text_encoder.character.index("7")
    sd[BC.Q + "fc.weight"][stop] = sd[BC.Q + "fc.weight"][seven]
    sd[BC.Q + "fc.bias"][stop] = sd[BC.Q + "fc.bias"][seven] + 0.5
    head.import_weights(sd, _dev(), "roi_heads.recognizer_head.")
    return head


def _decode_rows(head, rows):
    rows = rows.cpu().numpy()
    out = head.text_encoder.decode_attention(rows.argmax(-1), rows.max(-1).copy())
    return [o["text"] for o in out], np.array([float(o["score"]) for o in out])


def test_head_beam_width():
    """random fused features [5,8,32,256] over two images: BEAM_WIDTH 0 is bit-identical to a head built without the key,
    1 decodes to the default head's texts (word scores within 1e-4), 3 to beam_decode's best hypotheses"""
    g = torch.Generator(device="cpu")
    g.manual_seed(77)
    x = torch.randn((5, 8, 32, 256), generator=g).to(_dev())
    roi_image = torch.tensor([0, 0, 0, 1, 1], dtype=torch.int32, device=_dev())
    base = _head(drop_key=True)
    assert base.beam_width == 0
    p_base = base.forward_nhwc(x, roi_image, 2)
    p0 = _head(["MODEL.ROI_RECOGNIZER_HEAD.BEAM_WIDTH", 0]).forward_nhwc(x, roi_image, 2)
    assert torch.equal(p_base, p0)
    texts, scores = _decode_rows(base, p_base)
    p1 = _head(["MODEL.ROI_RECOGNIZER_HEAD.BEAM_WIDTH", 1]).forward_nhwc(x, roi_image, 2)
    assert p1.shape == p_base.shape
    t1, s1 = _decode_rows(base, p1)
    print(f"[beam] head: greedy {texts} {scores.tolist()}; width 1 {t1} {s1.tolist()}")
    assert t1 == texts and float(np.abs(s1 - scores).max()) < TOL
    assert any(len(t) < 25 for t in texts) and any(len(t) > 0 for t in texts), "the words do not exercise the stop"
    h3 = _head(["MODEL.ROI_RECOGNIZER_HEAD.BEAM_WIDTH", 3])
    p3 = h3.forward_nhwc(x, roi_image, 2)
    enc = h3.encoder.forward_nhwc(h3.backbone.forward_nhwc(x), rnn="steps")
    r = h3.decoder.beam_decode(enc, 3, h3.beam_eos, path_probs=True)
    assert torch.equal(p3, r.path_probs)
    t3, s3 = _decode_rows(h3, p3)
    want = [o["text"] for o in h3.text_encoder.decode_attention(r.symbols[:, 0].cpu().numpy().astype(np.int64))]
    assert t3 == want
    assert float(np.abs(s3 - np.exp(r.scores[:, 0].cpu().double().numpy())).max()) < TOL


def test_runner_end_to_end_with_beam_width():
    """GlassRunner with BEAM_WIDTH 3 on a small synthetic image, through detections_finalize and the word post-processor:
    every surviving word's text and text score are what the beam result of its source RoI decodes to.  The word score is a
    float32 product of at most 26 factors exp(score_t - score_{t-1}) against exp of the float32 sum: relative 1e-4 covers
    26 roundings of 2^-23 each by two orders of magnitude."""
    from glass_amd.inference.glass_runner import GlassRunner
    from glass_amd.config import get_glass_cfg
    from glass_amd.postprocess.post_processor_academic import strip_special
    from glass_amd.utils.synth import make_image, make_state_dict
    cfg = get_glass_cfg(os.path.join(ROOT, "configs", "glass_icdar15_mi355x.yaml"),
                        ["INPUT.MIN_SIZE_TEST", 160, "INPUT.MAX_SIZE_TEST", 200, "MODEL.DEVICE", "cuda:0",
                         "POST_PROCESSING.TEXT_THRESHOLD", 0.0, "POST_PROCESSING.DETECT_THRESHOLD", 0.0,
                         "POST_PROCESSING.LOW_CONFIDENCE", 0.0, "POST_PROCESSING.VALID_CONFIDENCE", 0.0,
                         "MODEL.ROI_RECOGNIZER_HEAD.BEAM_WIDTH", 3])
    runner = GlassRunner(None, None, cfg=cfg, state_dict=make_state_dict(1234), post_process=True)
    dec = runner.model.roi_heads.recognizer_head.decoder
    seen = []
    inner = dec.beam_decode

    def recording(*a, **kw):
        seen.append(inner(*a, **kw))
        return seen[-1]
    dec.beam_decode = recording
    out = runner(make_image(0, 120, 150).numpy())
    print(f"[beam] runner: {sum(s.symbols.shape[0] for s in seen)} RoIs decoded, {len(out)} words survive: {out.pred_texts}")
    assert len(seen) >= 1 and len(out) > 0, "no word survived: the case checks nothing"
    rows = torch.cat([s.path_probs for s in seen]).cpu()
    sym = torch.cat([s.symbols[:, 0] for s in seen]).cpu().numpy().astype(np.int64)
    score = torch.cat([s.scores[:, 0] for s in seen]).cpu().double().numpy()
    word_rows = out.pred_text_prob.cpu()
    text_scores = np.asarray(out.pred_text_scores.cpu() if torch.is_tensor(out.pred_text_scores) else out.pred_text_scores, dtype=np.float64)
    for i in range(len(out)):
        src = [j for j in range(rows.shape[0]) if torch.equal(rows[j], word_rows[i])]
        assert src, f"word {i}: its pred_text_prob rows are no RoI's path rows"
        j = src[0]
        # (the word post-processing strips one leading and one trailing special character from a word's text)
        assert out.pred_texts[i] == strip_special(runner.text_encoder.decode_attention(sym[j][None])[0]["text"])
        assert abs(text_scores[i] - math.exp(score[j])) <= 1e-4 * math.exp(score[j])
