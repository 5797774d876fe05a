"""GPU: the character boxes (include/glass_hip_feature_chars.h).  glass_forced_attention against glass_forced_decode (every shared
output `torch.equal`) and against the float64 replay of char_box_cases.py; the properties of the attention rows; glass_char_spans
against its host statement; glass_char_quads tied to the recogniser's pooler; MODEL.ROI_RECOGNIZER_HEAD.CHAR_BOXES through the
recogniser head and GlassRunner.run_batch.  The one symbol outside [0, C) that a case holds is met by the step -1 launch's
range check (read in csrc/decoder_search.hip: it ends the sequence there and is never used as an index)."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import beam_cases as BC
import char_box_cases as C
import forced_cases as FC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-4                      # tests/test_gpu_forced_decode.py's and test_gpu_beam_search.py's TOL, for the same arithmetic
KEY = ["MODEL.ROI_RECOGNIZER_HEAD.CHAR_BOXES", True]
W5 = ["MODEL.ROI_RECOGNIZER_HEAD.BEAM_WIDTH", 5]
DIST = ["MODEL.ROI_RECOGNIZER_HEAD.BEAM_DISTRIBUTIONS", True]
PATTERN = ["MODEL.ROI_RECOGNIZER_HEAD.DECODE_PATTERN", "[0-9a-z]{3,9}"]      # (with "+" every best word is one letter)


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


_DECODERS = {}


def _weights(C_):
    """the decoder weights for C_ classes on the device (the entry points take max_len per call)"""
    if C_ not in _DECODERS:
        from glass_amd.modeling.recognition.recognizer_decoder import ASTER_V2
        from glass_amd.structures.core import ShapeSpec
        sd = BC.decoder_sd(C_)
        dec = ASTER_V2(BC.decoder_cfg(C_, 26), ShapeSpec(channels=256))
        dec.import_weights(sd, _dev(), BC.PRE)
        _DECODERS[C_] = (dec, sd)
    return _DECODERS[C_]


# (name, B, n, T, L, C, seed): B 0 / 1 / 3 / 17, all five row blocks (n 1, 2, 3 -> 4, 5 -> 8, 16), T 1 / 2 / 31 / 32 / 64, L 1 / 2 / 26 /
# 64, C 2 / 97 / 256
SHAPES = [
    ("b0", 0, 1, 32, 26, 97, 1),
    ("b1_n1_t1_l1_c2", 1, 1, 1, 1, 2, 2),
    ("b3_n2_t2_l2_c97", 3, 2, 2, 2, 97, 3),
    ("b17_n3_t31_l26_c97", 17, 3, 31, 26, 97, 4),
    ("b3_n5_t32_l26_c256", 3, 5, 32, 26, 256, 5),
    ("b3_n16_t64_l64_c97", 3, 16, 64, 64, 97, 6),
]


def _targets(B, n, L, C_, seed, given):
    """targets int32 [B,n,L] and lengths [B,n] | None.  `given`: seeded lengths that hold 0 and L.  Else the lengths come from the
    stop symbol 0: sequence 0 of item 0 runs to L without a stop, the last item's n sequences all stop at step 0 (they have
    ended while the other items go on), and (B >= 2, L >= 2) item 1's sequence 0 stops at a symbol outside [0, C) at step 1"""
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    tg = torch.randint(0, C_, (B, n, L), generator=g, dtype=torch.int32) if B else torch.zeros((0, n, L), dtype=torch.int32)
    if given or B == 0:
        return tg, (FC.seeded_lengths(B, n, L, seed + 7).to(torch.int32) if B else torch.zeros((0, n), dtype=torch.int32))
    tg[0, 0] = torch.randint(1, C_, (L,), generator=g, dtype=torch.int32)
    if B >= 2:
        tg[B - 1, :, 0] = 0
        if L >= 2:
            tg[1, 0, 0], tg[1, 0, 1] = 1, C_ + 5
    return tg, None


def _effective(tg, ln, C_):
    """the effective lengths glass_forced_decode computes, on the host"""
    B, n, L = tg.shape
    out = torch.zeros((B, n), dtype=torch.long)
    for b in range(B):
        for j in range(n):
            lim = L if ln is None else min(max(int(ln[b, j]), 0), L)
            e = lim
            for t in range(lim):
                s = int(tg[b, j, t])
                if s < 0 or s >= C_:
                    e = t
                    break
                if ln is None and s == 0:
                    e = t + 1
                    break
            out[b, j] = e
    return out


_REPLAYS = {}


def _replay(shape, given):
    """one shape, computed once: the inputs on the device, glass_forced_decode's and glass_forced_attention's outputs"""
    key = (shape[0], given)
    if key not in _REPLAYS:
        from glass_amd.ops import native as K
        name, B, n, T, L, C_, seed = shape
        dec, sd = _weights(C_)
        x = BC.rand_x(B, T, seed).to(_dev())
        xproj = K.linear(x.view(B * T, 256), dec.w["xW"], dec.w["xB"]).view(B, T, 256) if B else x
        tg, ln = _targets(B, n, L, C_, seed, given)
        tgd, lnd = tg.to(_dev()), (ln.to(_dev()) if ln is not None else None)
        plain = K.forced_decode(x, xproj, dec.w, tgd, lnd, C_, L, 0, probs=True, logits=True)
        att = K.forced_decode(x, xproj, dec.w, tgd, lnd, C_, L, 0, probs=True, logits=True, attention=True)
        _REPLAYS[key] = dict(x=x, xproj=xproj, tg=tg, ln=ln, tgd=tgd, lnd=lnd, plain=plain, att=att, w=dec.w, sd=sd)
    return _REPLAYS[key]


@pytest.mark.parametrize("given", [True, False], ids=["lengths", "stop"])
@pytest.mark.parametrize("shape", SHAPES, ids=[s[0] for s in SHAPES])
def test_replay_outputs_equal_forced_decode(shape, given):
    name, B, n, T, L, C_, seed = shape
    r = _replay(shape, given)
    assert len(r["plain"]) == 5 and len(r["att"]) == 6                 # the rows come as one more trailing element, when asked
    for a, b, what in zip(r["att"][:5], r["plain"], ("step_logp", "scores", "lengths", "probs", "logits")):
        assert a.shape == b.shape and torch.equal(a, b), (name, what)
    assert r["att"][5].shape == (B, n, L, T) and r["att"][5].dtype == torch.float32
    eff = _effective(r["tg"], r["ln"], C_)
    assert torch.equal(r["att"][2].cpu().long(), eff), name
    if B:
        assert int(eff.max()) == L and (not given or B * n == 1 or int(eff.min()) == 0), name
    if not given and B >= 2:
        assert int(eff[B - 1].max()) == 1                              # an item whose n sequences have all ended
        if L >= 2:
            assert int(eff[1, 0]) == 1 and math.isinf(float(r["att"][1][1, 0]))    # stopped by the symbol outside [0, C)


@pytest.mark.parametrize("given", [True, False], ids=["lengths", "stop"])
@pytest.mark.parametrize("shape", SHAPES, ids=[s[0] for s in SHAPES])
def test_attention_rows(shape, given):
    from glass_amd import _lib
    from glass_amd.ops import native as K
    name, B, n, T, L, C_, seed = shape
    r = _replay(shape, given)
    rows = r["att"][5].cpu()
    ln = r["att"][2].cpu().long()
    live = torch.arange(L).view(1, 1, L) < ln.unsqueeze(2)
    assert not rows[~live].any(), name                                 # rows from the length on are exactly zero
    if B:
        assert float(rows.min()) >= 0.0 and torch.isfinite(rows).all()
        dev = float((rows.sum(3)[live] - 1.0).abs().max()) if live.any() else 0.0
        print(f"[chars] {name}/{'lengths' if given else 'stop'}: {int(live.sum())} live rows, max |row sum - 1| {dev:.3e}")
        assert dev < TOL, name
        for b in range(B):                                             # row 0 (h = 0) is the same for the item's sequences
            first = [j for j in range(n) if ln[b, j] > 0]
            for j in first[1:]:
                assert torch.equal(rows[b, j, 0], rows[b, first[0], 0]), (name, b, j)
    # two runs are bit-identical, and a NaN-poisoned buffer comes back fully written
    again = K.forced_decode(r["x"], r["xproj"], r["w"], r["tgd"], r["lnd"], C_, L, 0, attention=True)[5]
    assert torch.equal(again, r["att"][5]), name
    if B:
        buf = torch.full((B, n, L, T), float("nan"), dtype=torch.float32, device=_dev())
        outs = [torch.empty((B, n, L), device=_dev()), torch.empty((B, n), device=_dev()), torch.empty((B, n), dtype=torch.int32, device=_dev())]
        nbytes = int(_lib.lib().glass_forced_attention_workspace_bytes(B, n, T, 256, C_, L))
        ws = torch.empty((max(nbytes, 16),), dtype=torch.uint8, device=_dev())
        w = K._decoder_weights(r["w"])
        _lib.check(_lib.lib().glass_forced_attention(r["x"].data_ptr(), r["xproj"].data_ptr(), ctypes.byref(w), B, n, T, 256, C_, L, 0,
                                                     r["tgd"].data_ptr(), r["lnd"].data_ptr() if r["lnd"] is not None else None,
                                                     outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), None, None,
                                                     buf.data_ptr(), ws.data_ptr(), nbytes, K.stream_handle()), "glass_forced_attention")
        assert torch.equal(buf, r["att"][5]), name


F64_CASES = [c for c in BC.CASES if c[0] in ("b3_k2_t32_l26", "b17_k5_t64_l64", "b3_k5_t7_l26_c5", "b3_k16_t32_l26_c256")]


@pytest.mark.parametrize("case", F64_CASES, ids=[c[0] for c in F64_CASES])
def test_rows_against_the_float64_replay(case):
    """the hypotheses of the float64 beam replay and seeded lengths (the sets of tests/forced_cases.py): every attention row within
    TOL of the float64 replay's.  Measured on one MI355X: the largest difference over the four cases is 6.9e-07 - far below
    the bound, which is the one the forced decoding and the beam search hold for this arithmetic, not one fitted to this code."""
    from glass_amd.ops import native as K
    name, B, k, T, L, C_, seed = case
    d = FC.case_data(case)
    from glass_amd.modeling.recognition.recognizer_decoder import ASTER_V2
    from glass_amd.structures.core import ShapeSpec
    dec = ASTER_V2(BC.decoder_cfg(C_, L), ShapeSpec(channels=256))
    dec.import_weights(d["sd"], _dev(), BC.PRE)
    x = d["x"].to(_dev())
    for s in ("hyp", "lengths"):
        tg, ln = d["sets"][s]
        want = C.forced_attention_f64(d["sd"], d["x"], tg, ln)
        got = dec.score(x, tg, ln, eos=0, attention=True)
        assert torch.equal(got.lengths.cpu().long(), d["f64"][s]["lengths"]) and len(got) == 5
        diff = float((got.attention.cpu().double() - want).abs().max())
        print(f"[chars] {name}/{s}: max |attention - float64 replay| {diff:.3e} over {tuple(want.shape)}")
        assert got.attention.shape == (B, k, L, T) and diff < TOL, (name, s)


# ---------------------------------------------------------------------- spans
def _spans_on_device(att, tg, ln, eos):
    from glass_amd.ops import native as K
    out = K.char_spans(torch.from_numpy(np.ascontiguousarray(att)).to(_dev()), torch.from_numpy(np.ascontiguousarray(tg)).to(_dev()),
                       torch.from_numpy(np.ascontiguousarray(ln)).to(_dev()), eos)
    return {k: v.cpu().numpy() for k, v in out.items()}


def test_spans_equal_the_host_statement_on_every_cpu_case():
    from glass_amd.postprocess.char_boxes import char_spans_host
    sizes = set()
    for name, att, tg, ln, ref in C.all_cases():
        got = _spans_on_device(att, tg, ln, C.EOS)
        worst = C.assert_same(got, char_spans_host(att, tg, ln, C.EOS), name)
        C.assert_matches_reference(got, ref, name, att.shape[1])       # and the exact checker, as the host statement does
        sizes.add(att.shape[0])
        print(f"[chars] device spans, {name}: {att.shape[0]} words, worst float32 ulp vs the host statement {worst}")
    assert {1, 63, 64, 65} <= sizes


@pytest.mark.parametrize("R", [0, 1, 63, 64, 65, 1024])
def test_spans_on_the_device_rows(R):
    """the device's own attention rows (softmax rows, the stop found by the replay), tiled to R words"""
    from glass_amd.ops import native as K
    from glass_amd.postprocess.char_boxes import char_spans_host
    r = _replay(SHAPES[3], False)                                      # 17 x 3 sequences, T 31, L 26
    att = r["att"][5].reshape(-1, 26, 31)
    tg, ln = r["tgd"].reshape(-1, 26), r["att"][2].reshape(-1)
    idx = torch.arange(R, device=_dev()) % att.shape[0]
    att, tg, ln = att[idx].contiguous(), tg[idx].contiguous(), ln[idx].contiguous()
    out = K.char_spans(att, tg, ln, 0)
    assert out["spans"].shape == (R, 26, 2) and out["count"].shape == (R,) and out["count"].dtype == torch.int32
    got = {k: v.cpu().numpy() for k, v in out.items()}
    want = char_spans_host(att.cpu().numpy(), tg.cpu().numpy(), ln.cpu().numpy(), 0)
    worst = C.assert_same(got, want, f"R={R}")
    if R:
        assert got["valid"].all() and got["count"].max() > 2
        again = K.char_spans(att, tg, ln, 0)
        assert all(torch.equal(again[k], out[k]) for k in out)
        print(f"[chars] device rows, R={R}: counts up to {int(got['count'].max())}, non-monotone {int((got['monotone'] == 0).sum())} "
              f"of {R}, worst float32 ulp {worst}")


# ---------------------------------------------------------------------- quads, tied to the pooler
def test_quads_sit_where_the_pooler_samples():
    """A one-level map whose channels are the image coordinates x + 0.5 and y + 0.5 of its pixels: linear ramps, so a bilinear
    sample returns the sampled position and the pooled value of column j of a (1, T) pooling is the image position of that
    column's centre.  The centre of the quad of the span (j / T, (j + 1) / T) must be that point."""
    from glass_amd.ops import native as K
    from glass_amd.postprocess.post_processor_rotated_boxes import PostProcessorRotatedBoxes
    H, W, T, ratio = 96, 128, 8, 2
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    feat = torch.stack([xs + 0.5, ys + 0.5, torch.zeros_like(xs), torch.zeros_like(xs)], -1).unsqueeze(0).contiguous().to(_dev())
    boxes = torch.tensor([[64.0, 48.0, 40.0, 10.0, a] for a in (0.0, 30.0, 90.0, -170.0, 180.0)] + [[40.25, 50.5, 33.0, 7.0, 12.5]])
    R = boxes.shape[0]
    pooled = K.roi_align_rotated([feat], [1.0], boxes.to(_dev()), torch.zeros((R,), dtype=torch.int32, device=_dev()), (1, T), ratio)
    pooled = pooled.cpu().double()[:, 0, :, :2]                         # [R, T, (x, y)]
    # the same pooled value in float64: the mean over the kernel's sample grid of the sampled positions (no sample is clamped)
    want = np.zeros((R, T, 2))
    for r in range(R):
        cx, cy, w, h, a = (float(v) for v in boxes[r])
        th = a * math.pi / 180.0
        for j in range(T):
            acc = np.zeros(2)
            for iy in range(ratio):
                yy = -h / 2 + (iy + 0.5) * h / ratio
                for ix in range(ratio):
                    xx = -w / 2 + j * w / T + (ix + 0.5) * (w / T) / ratio
                    x, y = yy * math.sin(th) + xx * math.cos(th) + cx - 0.5, yy * math.cos(th) - xx * math.sin(th) + cy - 0.5
                    assert 0.0 <= x <= W - 1 and 0.0 <= y <= H - 1
                    acc += [x + 0.5, y + 0.5]
            want[r, j] = acc / (ratio * ratio)
    pool_err = float(np.abs(pooled.numpy() - want).max())
    tol = max(4.0 * pool_err, 1e-4)
    spans = torch.tensor([[[j / T, (j + 1) / T] for j in range(T)]] * R, dtype=torch.float32).to(_dev())
    count = torch.full((R,), T, dtype=torch.int32, device=_dev())
    quads = K.char_quads(spans, count, boxes.to(_dev()))
    assert quads.shape == (R, T, 4, 2)
    centre = quads.cpu().double().mean(2)
    err = float((centre - pooled).abs().max())
    print(f"[chars] quads: pooled ramp fp32 - float64 {pool_err:.3e} px, tolerance {tol:.3e} px, max |quad centre - pooled position| "
          f"{err:.3e} px")
    assert err <= tol
    # a span (0, 1) is the word's own polygon, corner for corner (float32 torch against float64 rounded once: a few ulps of the
    # coordinates' magnitude, 128 * 2^-23 = 1.5e-5 each)
    whole = torch.tensor([[[0.0, 1.0]]] * R).to(_dev())
    q = K.char_quads(whole, torch.ones((R,), dtype=torch.int32, device=_dev()), boxes.to(_dev())).cpu()
    poly = PostProcessorRotatedBoxes.boxes_to_polygons(boxes)
    assert float((q[:, 0] - poly).abs().max()) < 1e-4
    poly64 = PostProcessorRotatedBoxes.boxes_to_polygons(boxes.double())
    assert float((q[:, 0].double() - poly64).abs().max()) < 2e-5
    # rows from the count on are zero; bad frames give zero rows; two runs agree
    part = K.char_quads(spans, torch.tensor([0, 1, 3, 8, 99, -4], dtype=torch.int32, device=_dev()), boxes.to(_dev())).cpu()
    for r, m in enumerate((0, 1, 3, 8, 8, 0)):
        assert torch.equal(part[r, :m], quads.cpu()[r, :m]) and not part[r, m:].any()
    bad = boxes.clone()
    bad[0, 0], bad[1, 2], bad[2, 3], bad[3, 4], bad[4, 1] = float("nan"), 0.0, -1.0, float("inf"), float("-inf")
    qb = K.char_quads(spans, count, bad.to(_dev())).cpu()
    assert not qb[:5].any() and torch.equal(qb[5], quads.cpu()[5])
    assert K.char_quads(spans[:0], count[:0], boxes[:0].to(_dev())).shape == (0, T, 4, 2)
    from glass_amd.postprocess.char_boxes import char_quads_host
    host = char_quads_host(spans.cpu().numpy(), count.cpu().numpy(), boxes.numpy())
    assert int(C.ulps32(quads.cpu().numpy(), host).max()) <= 1


# ---------------------------------------------------------------------- the recogniser head
def _head(opts=()):
    """the head of tests/test_gpu_forced_decode.py: sharper output layer, a stop symbol that ends words at different steps"""
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


HEAD_CASES = [("greedy", [], False), ("beam5", W5, False), ("beam5_dist", W5 + DIST, False), ("beam5_pattern", W5 + PATTERN, False),
              ("greedy_steps", [], True)]


@pytest.mark.parametrize("R", [5, 70])
@pytest.mark.parametrize("case", HEAD_CASES, ids=[c[0] for c in HEAD_CASES])
def test_head_with_the_key_on(case, R):
    from glass_amd.modeling.recognition.recognizer_head_v2 import split_text_rows
    from glass_amd.ops import native as K
    from glass_amd.postprocess.char_boxes import unpack_chars
    name, opts, steps = case
    g = torch.Generator(device="cpu")
    g.manual_seed(77 + R)
    x = torch.randn((R, 8, 32, 256), generator=g).to(_dev())
    roi_image = (torch.arange(R, dtype=torch.int32) * 2 // R).to(_dev())
    h_off, h = _head(opts), _head(opts + KEY)
    if steps:
        h_off.rnn_override = h.rnn_override = "steps"
    off = h_off.forward_nhwc(x, roi_image, 2)
    on = h.forward_nhwc(x, roi_image, 2)
    assert isinstance(on, tuple) and len(on) == 3
    rows, dist, packed = split_text_rows(on, chars=True)
    rows_off, dist_off = split_text_rows(off)
    assert torch.equal(rows, rows_off), name                           # the text rows do not change with the key
    assert (dist is None) == (dist_off is None) and (dist is None or torch.equal(dist, dist_off)), name
    L, Cn, eos = h.decoder.max_word_len, h.decoder.num_classes, h.beam_eos
    assert packed.shape == (R, L + 1, 3)
    # by hand on the encoder output
    enc = h.encoder.forward_nhwc(h.backbone.forward_nhwc(x), rnn="steps")
    T = enc.shape[1]
    xproj = K.linear(enc.reshape(R * T, 256), h.decoder.w["xW"], h.decoder.w["xB"]).view(R, T, 256)
    if h.beam_width:
        lex = {}
        if h.pattern is not None:
            lex = {"pattern": h.pattern, "segments": torch.zeros((R,), dtype=torch.int32, device=_dev()), "weight_scale": h.weight_scale}
        b = h.decoder.beam_decode(enc, h.beam_width, eos, path_probs=True, **lex)
        assert torch.equal(b.path_probs, rows)
        sym = b.symbols[:, 0].contiguous()
        ln = torch.where(torch.isneginf(b.scores[:, 0]), torch.zeros_like(b.lengths[:, 0]), b.lengths[:, 0]).contiguous()
        live = torch.arange(L, device=_dev()).view(1, L) < ln.unsqueeze(1)
        assert torch.equal(rows.argmax(-1)[live].int(), sym[live])       # the symbols are the arg-max of the path rows
        f = K.forced_decode(enc.contiguous(), xproj, h.decoder.w, sym.unsqueeze(1), ln.unsqueeze(1).contiguous(), Cn, L, eos, attention=True)
    else:
        sym = rows.argmax(-1).to(torch.int32)
        f = K.forced_decode(enc.contiguous(), xproj, h.decoder.w, sym.unsqueeze(1), None, Cn, L, eos, attention=True)
    want = K.char_spans(f[5][:, 0].contiguous(), sym, f[2][:, 0].contiguous(), eos)
    got = unpack_chars(packed)
    assert torch.equal(got["pred_char_spans"], want["spans"]) and torch.equal(got["pred_char_centres"], want["centres"]), name
    assert torch.equal(got["pred_char_count"], want["count"].long()) and torch.equal(got["pred_char_monotone"], want["monotone"] > 0), name
    assert torch.equal(packed[:, L, 2], want["valid"].float())
    # the count is the number of steps before the stop
    s = rows.argmax(-1).cpu()
    stops = [int((s[i] == eos).nonzero()[0]) if (s[i] == eos).any() else L for i in range(R)]
    cnt = got["pred_char_count"].cpu().tolist()
    if not h.beam_width:
        assert cnt == stops, name
    assert max(cnt) > 1 and min(cnt) < L, "the words do not exercise the stop"
    print(f"[chars] head {name}, R={R}: counts {sorted(set(cnt))}, non-monotone {int((~got['pred_char_monotone']).sum())} of {R}")


# ---------------------------------------------------------------------- the runner
def _runner(extra):
    from glass_amd.config import get_glass_cfg
    from glass_amd.inference.glass_runner import GlassRunner
    from glass_amd.utils.synth import make_state_dict
    cfg = get_glass_cfg(os.path.join(ROOT, "configs", "glass_icdar15_mi355x.yaml"),
                        ["INPUT.MIN_SIZE_TEST", 160, "INPUT.MAX_SIZE_TEST", 200, "MODEL.DEVICE", "cuda:0",
                         "POST_PROCESSING.TEXT_THRESHOLD", 0.0, "POST_PROCESSING.DETECT_THRESHOLD", 0.0,
                         "POST_PROCESSING.LOW_CONFIDENCE", 0.0, "POST_PROCESSING.VALID_CONFIDENCE", 0.0] + list(extra))
    return GlassRunner(None, None, cfg=cfg, state_dict=make_state_dict(1234), post_process=True)


def test_run_batch_carries_the_character_fields():
    from glass_amd.inference.glass_runner import GlassRunner
    from glass_amd.postprocess import char_quads, chars_of
    from glass_amd.postprocess.char_boxes import CHAR_FIELDS
    from glass_amd.structures.core import RotatedBoxes
    from glass_amd.utils.synth import make_image
    imgs = [make_image(0, 120, 150).numpy(), make_image(1, 120, 150).numpy()]
    off = _runner([]).run_batch(imgs)
    run = _runner(KEY)
    on = run.run_batch(imgs)
    batch = run.model.last_batch                                       # the padded batch of the one model call (equal sizes: one group)
    ratio = run.get_inference_scale_ratio(imgs[0].shape)
    sc = torch.tensor([[1.0 / ratio, 1.0 / ratio]] * 2, dtype=torch.float32).to(_dev())
    pooled = GlassRunner._scaled_boxes(batch.boxes, sc).cpu()
    stop = run.text_encoder.character.index("[s]")
    total = same = 0
    for n, (a, b) in enumerate(zip(off, on)):
        assert len(a) > 0 and len(a) == len(b), "no word survived: the case checks nothing"
        for k, v in a.get_fields().items():                            # every field that existed before is what it was
            w = b.get(k)
            if isinstance(v, RotatedBoxes):
                assert torch.equal(v.tensor, w.tensor), k
            elif torch.is_tensor(v):
                assert torch.equal(v, w), k
            else:
                assert v == w, k
            assert not k.startswith("pred_char_")
        assert set(b.get_fields()) - set(a.get_fields()) == set(CHAR_FIELDS)
        R, L = len(b), b.pred_text_prob.shape[1]
        assert b.pred_char_spans.shape == (R, L, 2) and b.pred_char_centres.shape == (R, L) and b.pred_char_frames.shape == (R, 5)
        assert b.pred_char_count.dtype == torch.int64 and b.pred_char_monotone.dtype == torch.bool
        s = b.pred_text_prob.argmax(-1).cpu()
        stops = [int((s[i] == stop).nonzero()[0]) if (s[i] == stop).any() else L for i in range(R)]
        assert b.pred_char_count.cpu().tolist() == stops               # the steps before the stop in pred_text_prob
        frames, boxes = b.pred_char_frames.cpu(), b.pred_boxes.tensor.cpu()
        for i in range(R):                                             # each frame is a pooled box, in output pixels
            assert (pooled[n] == frames[i]).all(1).any(), (n, i)
            same += int(torch.equal(frames[i], boxes[i]))
        total += R
        words = chars_of(b, run.text_encoder)
        assert [len(w) for w in words] == stops
        quads = char_quads(b)
        assert quads.shape == (R, L, 4, 2)
        for i, word in enumerate(words):
            for t, ch in enumerate(word):
                assert ch["quad"] == quads[i, t].cpu().tolist() and ch["char"] == run.text_encoder.character[int(s[i, t])]
                assert ch["prob"] == float(b.pred_text_prob[i, t].max())
                mid = quads[i, t].cpu().double().mean(0)
                lo, hi = (float(v) for v in b.pred_char_spans[i, t])
                c = float(b.pred_char_centres[i, t])
                assert lo <= c <= hi or not bool(b.pred_char_monotone[i])
                # the centre lies on the box's axis: as far from the quad's middle as (c - (lo + hi) / 2) * w
                d = math.hypot(ch["centre"][0] - float(mid[0]), ch["centre"][1] - float(mid[1]))
                assert abs(d - abs(c - (lo + hi) / 2) * float(frames[i, 2])) < 1e-3
        keep = torch.arange(R, device=_dev()) % 2 == 0                 # the fields survive filtering
        sub = b[keep]
        assert torch.equal(sub.pred_char_spans, b.pred_char_spans[keep]) and torch.equal(sub.pred_char_frames, b.pred_char_frames[keep])
    assert same > 0, "no word kept its pooled box: the frame is checked against nothing"
    print(f"[chars] run_batch: {total} words, {same} with pred_boxes == pred_char_frames (the others were merged)")
    with pytest.raises(NotImplementedError, match="CHAR_BOXES"):
        run.run_tiled(imgs[0])
