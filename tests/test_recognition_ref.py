"""CPU: the float64 references of tests/recognition_ref.py against the fp32 oracle (oracle/glass_cpu.py, itself pinned to the
reference project's modules by the goldens) at the shipped shape - T = 32, C = 97, max_len = 26, the synthetic checkpoint.  The
GPU edge tests (tests/test_gpu_recognition_edges.py) hold the kernels to these functions at shapes the oracle never runs, so
the functions themselves are pinned here, where no GPU is needed.  Bounds: the oracle is fp32, so 1e-5 on O(1) outputs after a
32-step recurrence and 1e-4 (relative to the output range) behind the 4608-term out-conv."""
import torch

import recognition_ref as RR
from glass_amd.utils.synth import make_state_dict
from oracle import glass_cpu as O

DEC = "roi_heads.recognizer_head.decoder.recognizer.decoder."


def _sd():
    return make_state_dict(1234)


def test_fusion_attention_reference_matches_the_oracle():
    sd = _sd()
    p = "roi_heads.fusion_net."
    R, C, H, W = 2, 512, 8, 32
    x = torch.randn((R, C, H, W), generator=torch.Generator().manual_seed(1))
    want = O.gc_attention_fusion(sd, x)
    order = torch.zeros(C, dtype=torch.long)
    order[0::2] = torch.arange(C)[: C // 2]
    order[1::2] = torch.arange(C)[C // 2:]
    slab = x[:, order].permute(0, 2, 3, 1).reshape(R, H * W, C).contiguous()
    got, mid = RR.gc_attention(slab, sd[p + "conv_mask.weight"].reshape(-1), sd[p + "conv_mask.bias"],
                               sd[p + "channel_add_conv.0.weight"].reshape(256, 512), sd[p + "channel_add_conv.0.bias"],
                               sd[p + "channel_add_conv.1.weight"].reshape(-1), sd[p + "channel_add_conv.1.bias"].reshape(-1),
                               sd[p + "channel_add_conv.3.weight"].reshape(512, 256), sd[p + "channel_add_conv.3.bias"])
    assert got.dtype == torch.float64 and mid["logit"].shape == (R, H * W, 8)
    assert float((got - slab.double()).abs().max()) > 0.05, "the channel_add term must be visible"
    fused = got.float().reshape(R, H, W, C).permute(0, 3, 1, 2).contiguous()
    got_out = O.conv_bn(fused, sd, p + "out.weight", p + "out.bias", padding=1)       # the oracle's own out-conv on top
    err = float((got_out - want).abs().max()) / float(want.abs().max())
    print(f"[parity] float64 fusion attention + oracle out-conv vs oracle: max err / range {err:.2e}")
    assert err < 1e-4


def test_bilstm_reference_matches_the_oracle():
    sd = _sd()
    q = "roi_heads.recognizer_head.encoder.bilsm_stack.0.rnn."
    x = torch.randn((5, 32, 256), generator=torch.Generator().manual_seed(2))
    sfx = ("", "_reverse")
    want = torch.cat([O._lstm_dir(x, sd[q + "weight_ih_l0" + s], sd[q + "weight_hh_l0" + s], sd[q + "bias_ih_l0" + s],
                                  sd[q + "bias_hh_l0" + s], bool(d)) for d, s in enumerate(sfx)], dim=2)
    xg = torch.stack([(x.double() @ sd[q + "weight_ih_l0" + s].double().t() + sd[q + "bias_ih_l0" + s].double()
                       + sd[q + "bias_hh_l0" + s].double()).float() for s in sfx], dim=2)            # [R, T, 2, 1024]
    whh = torch.stack([sd[q + "weight_hh_l0" + s].float() for s in sfx])
    got = RR.bilstm(xg, whh)
    assert got.dtype == torch.float64 and got.shape == (5, 32, 512)
    err = float((got - want).abs().max())
    one, _ = RR.lstm_direction(xg[:, :, 1], whh[1], True)
    print(f"[parity] float64 BiLSTM recurrence vs oracle: max |dh| {err:.2e}")
    assert err < 1e-5 and torch.equal(one, got[:, :, 256:])
    # the fp32 evaluation of the same formulas is the oracle's arithmetic up to the order of two additions
    assert float((RR.bilstm(xg, whh, dtype=torch.float32) - want).abs().max()) < 1e-5


def test_decoder_references_match_the_oracle():
    """seed 3: the float64 reference's top-2 gap is above 1e-4 at every live step of the 9 RoIs (asserted), so the oracle's fp32
    greedy path cannot leave the reference's"""
    sd = _sd()
    W = RR.plain_from_state_dict(sd, DEC)
    x = torch.randn((9, 32, 256), generator=torch.Generator().manual_seed(3))
    xp = RR.xproj_of(x, W)
    want = O.attention_decoder(sd, x, rois_per_image=[4, 5])
    ref = RR.greedy_decode(x, xp, W, [0] * 4 + [1] * 5, 26, 0)
    assert float(ref["gap"][ref["live"]].min()) > 1e-4
    err = float((ref["probs"] - want).abs().max())
    print(f"[parity] float64 greedy decode vs oracle: max |dp| {err:.2e}, live steps {int(ref['live'].sum())} of {9 * 26}")
    assert err < 1e-5
    assert torch.equal(ref["live"], want.sum(-1) > 0), "early-break rows differ"
    assert torch.equal(ref["pred"][ref["live"]], want.argmax(-1)[ref["live"]])
    # the early break, against the oracle's: eos = what RoI 0 emits at step 2, RoI 0 alone in its image
    e = int(ref["pred"][0, 2])
    want_b = O.attention_decoder(sd, x, eos=e, rois_per_image=[1, 3, 5])
    ref_b = RR.greedy_decode(x, xp, W, [0] + [1] * 3 + [2] * 5, 26, e)
    assert not bool(ref_b["live"][0, 3:].any()) and bool(ref_b["live"][0, :3].all()) and bool(ref_b["live"][8].any())
    assert torch.equal(ref_b["live"], want_b.sum(-1) > 0) and float((ref_b["probs"] - want_b).abs().max()) < 1e-5
    # one step, teacher-forced from the zero state: step 0 of the oracle's loop
    logits, probs, h1 = RR.decoder_step(x, xp, torch.zeros((9, 256)), torch.zeros((9,), dtype=torch.int32), W)
    assert float((probs - want[:, 0]).abs().max()) < 1e-5 and torch.equal(probs, ref["probs"][:, 0])
    assert torch.allclose(torch.softmax(logits, 1), probs) and h1.shape == (9, 256)
    # a symbol outside [0, C) is clamped, as the C ABI says
    lo = RR.decoder_step(x, xp, h1, torch.full((9,), -1), W)[0]
    hi = RR.decoder_step(x, xp, h1, torch.full((9,), 97), W)[0]
    assert torch.equal(lo, RR.decoder_step(x, xp, h1, torch.zeros((9,), dtype=torch.long), W)[0])
    assert torch.equal(hi, RR.decoder_step(x, xp, h1, torch.full((9,), 96), W)[0])


def test_weight_builder_makes_the_layouts_the_decoder_module_imports():
    from glass_amd.ops import native as K
    plain = RR.make_decoder_plain(40, 11)
    w = RR.pack_decoder(plain, "cpu")
    assert torch.equal(w["fcW"], K.pack_kblocked(plain["fcW"])) and w["fcW"].shape == (64, 40, 4)
    assert torch.equal(w["sW"], K.pack_kblocked(plain["sW"])) and torch.equal(w["sW_rm"], plain["sW"])
    assert w["emb_gi"].shape == (40, 768) and w["emb"].shape == (40, 256) and w["w_ih"].shape == (768, 512)
    # against ASTER_V2.import_weights itself, on the synthetic checkpoint
    from glass_amd.modeling.recognition.recognizer_decoder import ASTER_V2
    sd = _sd()
    dec = ASTER_V2.__new__(ASTER_V2)
    dec.w = {}
    ASTER_V2.import_weights(dec, sd, "cpu", "roi_heads.recognizer_head.decoder.")
    mine = RR.pack_decoder(RR.plain_from_state_dict(sd, DEC), "cpu")
    for k, v in mine.items():
        assert (dec.w[k] == v) if k == "temperature" else torch.equal(dec.w[k], v), k


def test_greedy_reference_ties_and_break():
    """constructed exact ties: identical fc rows give one tie group, the first index wins and the gap looks past the group; an
    image stops after the step at which its last RoI has emitted eos"""
    plain = RR.make_decoder_plain(8, 5)
    plain["fcW"][:] = 0
    plain["fcB"][:] = 0.25
    x = torch.randn((3, 4, 256), generator=torch.Generator().manual_seed(6))
    r = RR.greedy_decode(x, RR.xproj_of(x, plain), plain, [0, 0, 1], 3, eos=1)
    assert bool(r["live"].all()) and bool((r["pred"] == 0).all()) and bool((r["ties"] == 8).all())
    assert bool(torch.isinf(r["gap"]).all()) and float((r["probs"] - 0.125).abs().max()) < 1e-15
    r = RR.greedy_decode(x, RR.xproj_of(x, plain), plain, [0, 0, 1], 3, eos=0)
    assert r["live"].tolist() == [[True, False, False]] * 3 and float(r["probs"][:, 1:].abs().max()) == 0.0
