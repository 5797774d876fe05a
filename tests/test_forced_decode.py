"""CPU: the float64 forced replay (tests/forced_cases.py) against the float64 beam search it must agree with and against the
reference's own teacher-forced forward (tests/golden/forced_decode.npz), the declared entries, the cfg key and the host-side
validation of targets."""
import math
import os

import numpy as np
import pytest
import torch

import beam_cases as BC
import forced_cases as FC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cfg(opts=()):
    from glass_amd.config import get_glass_cfg
    return get_glass_cfg(os.path.join(ROOT, "configs", "glass_icdar15_mi355x.yaml"), ["MODEL.DEVICE", "cpu"] + list(opts))


@pytest.mark.parametrize("case", BC.CASES, ids=[c[0] for c in BC.CASES])
def test_forced_replay_of_the_hypotheses_reproduces_the_search(case):
    """set (a): replaying a hypothesis of the float64 beam search gives the search's own scores after every step (the
    hypothesis's ancestor chain IS its symbol sequence) - to 1e-12, both being float64 sums of the same terms in another
    order - for every hypothesis that exists (finite score)"""
    name, B, k, T, L, C, seed = case
    d = FC.case_data(case)
    rep, f = d["replay"], d["f64"]["hyp"]
    assert torch.equal(f["lengths"], rep["lengths"])
    run = f["step_logp"].cumsum(2)
    worst, checked = 0.0, 0
    for b in range(B):
        for j in range(k):
            if float(rep["scores"][b, j]) > -math.inf:
                n = int(rep["lengths"][b, j])
                worst = max(worst, float((run[b, j, :n] - rep["step_scores"][b, j, :n]).abs().max()))
                assert abs(float(f["scores"][b, j] - rep["scores"][b, j])) <= 1e-12
                checked += 1
    print(f"[forced] {name}: {checked} hypotheses, max |dscore_t| forced replay vs search {worst:.3e}")
    assert checked >= B and worst <= 1e-12


@pytest.mark.parametrize("case", BC.CASES, ids=[c[0] for c in BC.CASES])
def test_target_sets_cover_what_they_claim(case):
    """zeros from the length on; the perturbed set changes lengths in both directions (where L allows); the explicit lengths
    include 0 and L"""
    name, B, k, T, L, C, seed = case
    d = FC.case_data(case)
    for s in FC.SETS:
        f = d["f64"][s]
        tg, _ = d["sets"][s]
        assert tg.min() >= 0 and tg.max() < C
        dead = torch.arange(L).view(1, 1, L) >= f["lengths"].unsqueeze(2)
        assert not f["step_logp"][dead].any() and not f["probs"][dead].any() and not f["logits"][dead].any()
        live = ~dead
        assert torch.allclose(f["probs"].sum(3)[live], torch.ones((), dtype=torch.float64), atol=1e-12)
    ln = d["f64"]["lengths"]["lengths"]
    assert int(ln.max()) == L and (B * k == 1 or int(ln.min()) == 0)
    if B * k >= 4 and L > 1:
        a, p = d["f64"]["hyp"]["lengths"], d["f64"]["perturb"]["lengths"]
        assert (p.view(-1)[2::4] == 1).all(), "a stop at step 0 gives length 1"
        assert (p.view(-1)[1::4] == L).all(), "a sequence without its stop runs all steps"
        assert not torch.equal(a, p)


def test_effective_lengths():
    tg = torch.tensor([[[3, 0, 2, 0], [1, 2, 3, 4], [0, 0, 0, 0]]])
    assert FC.effective_lengths(tg, None, 0).tolist() == [[2, 4, 1]]
    assert FC.effective_lengths(tg, torch.tensor([[0, 9, 3]]), 0).tolist() == [[0, 4, 3]]
    lp = np.array([[0.1, 0.2, 0.4]], dtype=np.float32)
    want = np.float32(np.float32(np.float32(0.1) + np.float32(0.2)) + np.float32(0.4))
    assert FC.f32_sequential_sum(lp, np.array([3]))[0] == want and FC.f32_sequential_sum(lp, np.array([0]))[0] == 0


def test_float64_replay_reproduces_the_reference_forward(golden_dir):
    """the reference's AttentionRecognitionHead.forward on x [3,32,256], 26 steps, 97 classes (scripts/make_forced_golden.py):
    step i reads y_prev = labels[:, i], i.e. the symbol emitted at step t is labels[:, t + 1]; logits within 1e-4, the bound
    tests/test_beam_search.py uses for its replay of the beam golden"""
    g = np.load(os.path.join(golden_dir, "forced_decode.npz"), allow_pickle=False)
    sd = BC.decoder_sd(97, int(g["seed"]), float(g["fc_scale"]), float(g["bias0"]))
    x, labels = torch.from_numpy(g["x"]), torch.from_numpy(g["labels"])
    assert labels.shape == (3, 27) and g["logits"].shape == (3, 26, 97)
    f = FC.forced_f64(sd, x, labels[:, 1:].unsqueeze(1), torch.full((3, 1), 26))
    d = float(np.abs(f["logits"][:, 0].numpy() - g["logits"].astype(np.float64)).max())
    print(f"[forced] golden: max |dlogit| float64 replay vs reference {d:.3e} (max |logit| {float(np.abs(g['logits']).max()):.1f})")
    assert d < 1e-4
    # the rows depend on the labels: with the word shifted by one slot the replay is far from the golden
    f_bad = FC.forced_f64(sd, x, labels[:, :26].unsqueeze(1), torch.full((3, 1), 26))
    assert float(np.abs(f_bad["logits"][:, 0].numpy() - g["logits"]).max()) > 1.0


def test_forced_decode_entries_are_declared_and_have_no_cpu_fallback():
    from glass_amd import _lib
    from glass_amd.ops import native as K
    hdr = open(os.path.join(ROOT, "include", "glass_hip.h")).read()
    for name in ("glass_forced_decode_workspace_bytes", "glass_forced_decode"):
        assert name in _lib.EXPORTS and name + "(" in hdr, name
    assert _lib.ABI_VERSION == 8                                          # additive change
    _lib.build_library()
    L = _lib.lib()
    assert L.glass_forced_decode_workspace_bytes(3, 5, 32, 256, 97, 26) == 3 * 5 * (256 * 4 * 4 + 2 * 4)
    assert L.glass_forced_decode_workspace_bytes(0, 5, 32, 256, 97, 26) == 0
    x = torch.zeros((1, 4, 256))
    with pytest.raises(_lib.GlassLibraryError):
        K.forced_decode(x, x, {}, torch.zeros((1, 1, 26), dtype=torch.int32), None, 97, 26, 0)


def test_beam_distributions_key_defaults_off_and_needs_a_beam_width():
    from glass_amd.config import get_glass_cfg
    from glass_amd.modeling.recognition.recognizer_head_v2 import RecognizerRCNNHeadV3
    from glass_amd.structures.core import ShapeSpec
    key = "MODEL.ROI_RECOGNIZER_HEAD.BEAM_DISTRIBUTIONS"
    assert get_glass_cfg().MODEL.ROI_RECOGNIZER_HEAD.BEAM_DISTRIBUTIONS is False
    assert _cfg().MODEL.ROI_RECOGNIZER_HEAD.BEAM_DISTRIBUTIONS is False
    assert RecognizerRCNNHeadV3(_cfg(), ShapeSpec(channels=256)).beam_distributions is False
    head = RecognizerRCNNHeadV3(_cfg(["MODEL.ROI_RECOGNIZER_HEAD.BEAM_WIDTH", 3, key, True]), ShapeSpec(channels=256))
    assert head.beam_distributions is True and head.beam_width == 3
    with pytest.raises(ValueError, match="BEAM_WIDTH"):
        RecognizerRCNNHeadV3(_cfg([key, True]), ShapeSpec(channels=256))


def _decoder(C=97, L=26):
    from glass_amd.modeling.recognition.recognizer_decoder import ASTER_V2
    from glass_amd.structures.core import ShapeSpec
    return ASTER_V2(BC.decoder_cfg(C, L), ShapeSpec(channels=256))       # no weights imported: nothing may get that far


def test_host_targets_are_validated_before_anything_is_uploaded():
    """lists and CPU tensors: shape, dtype and range [0, C) raise ValueError - on a machine without a device, where an upload
    or a kernel call would raise something else"""
    dec = _decoder()
    x = torch.zeros((2, 8, 256))
    ok = torch.zeros((2, 26), dtype=torch.long)
    for bad, what in ((ok[:, :25], "shape"), (ok[:1], "shape"), (torch.zeros((2, 17, 26), dtype=torch.long), "n="),
                      (ok.float(), "integers"), (ok.clone().fill_(97), "outside"), (ok.clone().fill_(-1), "outside"),
                      ([[0] * 26, [0] * 25 + [200]], "outside"), (torch.zeros((2, 3, 4, 26), dtype=torch.long), "shape")):
        with pytest.raises(ValueError, match=what if what != "shape" else "must be"):
            dec.score(x, bad)
    for bad_len, what in ((torch.tensor([27, 0]), "outside"), (torch.tensor([-1, 0]), "outside"), (torch.tensor([1, 2, 3]), "match"),
                          (torch.tensor([1.0, 2.0]), "integers")):
        with pytest.raises(ValueError, match=what):
            dec.score(x, ok, bad_len)
    with pytest.raises(ValueError, match="distributions"):
        dec.beam_decode(x, 3, distributions="every")
    with pytest.raises(ValueError, match="labels"):
        dec.forward(x, labels=torch.zeros((2, 26), dtype=torch.long))         # [R, max_word_len + 1] is 27 wide


def test_forced_result_and_beam_result_fields():
    from glass_amd.modeling.recognition.recognizer_decoder import BeamResult, ForcedResult
    assert ForcedResult._fields == ("step_logp", "scores", "lengths", "probs", "logits")
    # the tuple keeps its four fields (callers rebuild a result from them); `distributions` rides as an attribute
    assert BeamResult._fields == ("symbols", "scores", "lengths", "path_probs")
    r = BeamResult(1, 2, 3, 4)
    assert r.distributions is None and tuple(r) == (1, 2, 3, 4) and type(r)(*r).path_probs == 4
    assert BeamResult(1, 2, 3, None, 5).distributions == 5 and BeamResult(1, 2, 3, distributions=5).path_probs is None


def test_coco_records_take_character_probs_from_the_distribution_rows():
    """text and score_text from pred_text_prob (path rows), character_probs from pred_text_dist when the instances have it"""
    from glass_amd.evaluation.text_evaluator import instances_to_coco_json
    from glass_amd.modeling.recognition.text_encoder import TextEncoder
    from glass_amd.structures.core import Instances, RotatedBoxes
    enc = TextEncoder(_cfg())
    stop = enc.character.index("[s]")
    a, b = enc.character.index("a"), enc.character.index("b")
    C = len(enc.character)
    path = torch.zeros((1, 26, C))
    path[0, 0, a], path[0, 1, b], path[0, 2, stop] = 0.9, 0.8, 0.7
    g = torch.Generator().manual_seed(3)
    dist = torch.softmax(torch.randn((1, 26, C), generator=g), 2)
    inst = Instances((50, 60))
    inst.pred_boxes = RotatedBoxes(torch.tensor([[20.0, 20.0, 10.0, 5.0, 0.0]]))
    inst.scores = torch.tensor([0.5])
    inst.pred_text_prob = path
    plain = instances_to_coco_json(inst, "f", enc)
    inst.pred_text_dist = dist
    both = instances_to_coco_json(inst, "f", enc)
    assert len(plain) == 1 and len(both) == 1 and both[0]["rec"] == plain[0]["rec"] == "ab"
    assert both[0]["score_text"] == plain[0]["score_text"]
    assert np.array_equal(np.asarray(plain[0]["character_probs"]), path[0].double().numpy())
    assert np.array_equal(np.asarray(both[0]["character_probs"]), dist[0].double().numpy())
