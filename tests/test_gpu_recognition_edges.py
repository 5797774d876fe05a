"""GPU: the recognition head kernel by kernel - fusion attention (csrc/fusion_attention.hip), the BiLSTM recurrence in its step
and persistent forms (csrc/bilstm.hip, csrc/recurrent_persistent.hip), one teacher-forced decoder step and the greedy decoder in
its step and persistent forms (csrc/decoder.hip, csrc/recurrent_persistent.hip) - against the float64 references of
tests/recognition_ref.py, at the class counts, sequence lengths, RoI counts and value ranges the stage tests never run.
Inputs, references and the fp32-vs-float64 error each bound is derived from come from tests/recognition_edge_cases.py:

    bound = min(max(4 x [error of the fp32 evaluation of the reference formulas on the test's own inputs], 1e-6), project bound)

with the project bound 1e-4 for BiLSTM / decoder outputs and 1e-3 for the fusion attention.  Logits and states that are not O(1)
(the +-80 logits, the scaled state) are compared relative to the largest magnitude of the reference.  Every test prints its
measured (kernel error, fp32 error, bound) as a [parity] line.

Measured on an MI355X (kernel vs float64 | fp32 formulas vs float64 on the same inputs | bound), largest of each group:
  fusion attention   randn 1.4e-6 | 1.5e-6 | 6.0e-6;  peaked 2.9e-6 | 5.0e-6 | 2.0e-5;  flat hid 2.4e-5 | 2.2e-5 | 8.8e-5;
                     uniform head: 6.3e-6 | 1.1e-6 | 4.3e-6 with the context summed over the 256 positions one by one (found by
                     this test); gc_attention_kernel now sums each trip of 16 as a tree: 9.5e-7 | 1.6e-6 | 4.3e-6 .. 6.3e-6
  BiLSTM             T <= 3: 3.7e-7 | 3.1e-7 | 1.0e-6 .. 1.2e-6;  T = 32: 5.8e-7 | 6.9e-7 | 1.0e-6 .. 2.7e-6 (|c| up to 31.9)
  decoder step       logits (relative) 6.1e-7 | 5.1e-7 | 1.0e-6 .. 2.0e-6;  probabilities 7.0e-6 | 1.1e-5 | 1.0e-6 .. 4.4e-5;
                     h_out (relative) 2.3e-6 | 3.3e-6 | 1.6e-6 .. 1.3e-5;  R = 513 / 1027: 1.9e-6 | 2.0e-6 | 6.1e-6 .. 7.8e-6
  greedy decode      steps 2.4e-6, persistent 1.2e-6 | 1.9e-6 | 1.9e-6 .. 7.5e-6;  uniform rows 3.7e-10 | 3.7e-10 | 1.0e-6
The non-finite cases run the kernels on NaN / inf inputs; they rely on the bound arg-max of csrc/decoder.hip (every index the
decoder derives stays in [0, C)), which the C ABI header states as the contract."""
import pytest
import torch

import recognition_edge_cases as E
import recognition_ref as RR

pytestmark = pytest.mark.gpu

PERSISTENT_MODES = ((2, 1), (2, 2), (1, 1))


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _say(capsys, msg):
    with capsys.disabled():
        print("\n" + msg, end="")


def _hold(capsys, what, got, want, err32, project, relative=False):
    """max |got - want| (over max(1, max |want|) if `relative`) against the derived bound; a NaN in `got` fails"""
    scale = max(1.0, float(want.abs().max())) if relative else 1.0
    err = float((got.detach().cpu().double() - want).abs().max()) / scale
    b = E.bound(err32 / scale, project)
    _say(capsys, f"[parity] {what}: kernel vs float64 {err:.2e}, fp32 formulas vs float64 {err32 / scale:.2e}, bound {b:.2e}"
                 + (f" (relative to {scale:.1f})" if relative else ""))
    assert err <= b, (what, err, b)


def _first_argmax(p):
    C = p.shape[-1]
    top = p.max(-1, keepdim=True).values
    return torch.where(p == top, torch.arange(C), torch.full((1,), C)).min(-1).values


# ================================================================================================ fusion attention
def _fusion_run(x, w):
    from glass_amd.ops import native as K
    d = _dev()
    xd = x.reshape(x.shape[0], 8, 32, 512).clone().to(d)
    wd = {k: v.contiguous().to(d) for k, v in w.items()}
    K.gc_attention_inplace(xd, 8, wd["w_mask"], wd["b_mask"], wd["w1"], wd["b1"], wd["ln_g"], wd["ln_b"], wd["w2"], wd["b2"])
    torch.cuda.synchronize()
    return xd.reshape(x.shape)


@pytest.mark.parametrize("R", [1, 3])
@pytest.mark.parametrize("kind", E.FUSION_KINDS)
def test_fusion_attention_against_float64(kind, R, capsys):
    """glass_gc_attention_inplace called directly: randn; mask logits up to +-60 (near one-hot softmax); two heads with equal
    logits at all positions (softmax 1/256); hid nearly constant (LayerNorm variance ~ its epsilon).
    uniform_head is the case that found the drift of a 256-term running sum of like terms (R = 1: 6.3e-6 against a bound of
    4.3e-6); with the 16-term trees in phase 3 of the kernel it measures 6.3e-7"""
    c = E.fusion_case(kind, R)
    logit, hid = c["mid"]["logit"], c["mid"]["hid"]
    if kind == "peaked":
        assert 55 < float(logit.abs().max()) < 65 and float(torch.softmax(logit, 1).max()) > 0.999
    if kind == "uniform_head":
        assert float((logit[:, :, [2, 5]].max(1).values - logit[:, :, [2, 5]].min(1).values).abs().max()) == 0.0
    if kind == "flat_hid":
        assert 0.5e-5 < float(hid.var(1, unbiased=False).min()) and float(hid.var(1, unbiased=False).max()) < 2e-5
    got = _fusion_run(c["x"], c["w"])
    _hold(capsys, f"fusion attention {kind} R={R}", got, c["want"], c["err32"], E.FUSION_PROJECT_BOUND)


def test_fusion_attention_with_no_rois_touches_nothing():
    from glass_amd._lib import lib
    from glass_amd.ops import native as K
    d = _dev()
    w = {k: v.contiguous().to(d) for k, v in E.fusion_weights(3).items()}
    args = (w["w_mask"], w["b_mask"], w["w1"], w["b1"], w["ln_g"], w["ln_b"], w["w2"], w["b2"])
    empty = torch.empty((0, 8, 32, 512), device=d)
    assert K.gc_attention_inplace(empty, 8, *args).shape == (0, 8, 32, 512)
    x = torch.randn((1, 8, 32, 512), generator=torch.Generator().manual_seed(1)).to(d)
    keep = x.clone()
    # the library itself with R = 0 and a live buffer: it must return OK before it reads or launches anything
    rc = lib().glass_gc_attention_inplace(K._dev(x), 0, 256, 512, 8, 256, *[K._dev(t) for t in args], K.stream_handle())
    torch.cuda.synchronize()
    assert rc == 0 and torch.equal(x, keep)


# ================================================================================================ BiLSTM recurrence
@pytest.mark.parametrize("kind", E.LSTM_KINDS)
@pytest.mark.parametrize("R,T", E.LSTM_SHAPES)
def test_bilstm_against_float64_and_persistent_bit_identical(R, T, kind, capsys):
    """the step kernels against float64 at one and two time steps, a ragged RoI group, saturated gates and a cell state that
    grows to ~T; the three persistent forms bit-identical to the step kernels on every one of these inputs"""
    from glass_amd.ops import native as K
    c = E.lstm_case(R, T, kind)
    if kind == "grow":
        assert c["cmax"] > 0.95 * T, "the cell state must grow by about one per step"
    xg, whh = c["xg"].to(_dev()), c["whh"].to(_dev())
    K.recurrence_status(reset=True)
    steps = K.bilstm_recurrence(xg, whh, 256, mode="steps")
    _hold(capsys, f"BiLSTM steps R={R} T={T} {kind} (|c| up to {c['cmax']:.1f})", steps, c["want"], c["err32"], E.LSTM_PROJECT_BOUND)
    for mode in PERSISTENT_MODES:
        got = K.bilstm_recurrence(xg, whh, 256, mode=mode)
        assert torch.equal(got, steps), (mode, float((got - steps).abs().max()))
    assert K.recurrence_status() == 0


# ================================================================================================ decoder step, teacher-forced
def _step_run(c):
    from glass_amd.ops import native as K
    d = _dev()
    C = c["plain"]["fcW"].shape[0]
    w = RR.pack_decoder(c["plain"], d)
    out = K.attention_decode_step(c["x"].to(d), c["xproj"].to(d), w, c["h"].to(d), c["y"].to(d), C)
    torch.cuda.synchronize()
    return out


def _step_hold(capsys, what, c):
    logits, probs, h_out = _step_run(c)
    wl, wp, wh = c["want"]
    assert logits.shape == wl.shape and probs.shape == wp.shape and h_out.shape == wh.shape
    _hold(capsys, what + " logits", logits, wl, c["err32"][0], E.DEC_PROJECT_BOUND, relative=True)
    _hold(capsys, what + " probabilities", probs, wp, c["err32"][1], E.DEC_PROJECT_BOUND)
    _hold(capsys, what + " h_out", h_out, wh, c["err32"][2], E.DEC_PROJECT_BOUND, relative=True)


@pytest.mark.parametrize("T,C,R", E.STEP_SHAPES)
def test_decoder_step_shapes_against_float64(T, C, R, capsys):
    """dec_fc_att_kernel + dec_gru_kernel with h and y_prev given (no arg-max in the loop): T up to DEC_TMAX = 64 around the 16-row
    unroll of the context sum, C up to DEC_CMAX = 256 around the 64-lane slots of the soft-max"""
    _step_hold(capsys, f"decoder step T={T} C={C} R={R}", E.step_case(T, C, R))


@pytest.mark.parametrize("kind", E.STEP_KINDS[1:])
@pytest.mark.parametrize("T,C,R", E.STEP_VARIANT_SHAPES)
def test_decoder_step_value_edges_against_float64(T, C, R, kind, capsys):
    c = E.step_case(T, C, R, kind)
    if kind == "y_edges":
        assert {-1, 0, C - 1, C} <= set(c["y"].tolist()) or R < 4
    if kind == "h_saturating":
        assert c["sat"] > 0.4
    if kind == "logits80":
        assert abs(float(c["want"][0].abs().max()) - 80.0) < 1e-3
    _step_hold(capsys, f"decoder step T={T} C={C} R={R} {kind}", c)


@pytest.mark.parametrize("T,C,R", E.STEP_TAIL_SHAPES)
def test_decoder_step_partial_tail_workgroups_against_float64(T, C, R, capsys):
    """R = 513 selects dec_fc_att_kernel<2> and leaves one RoI to its last workgroup, R = 1027 selects <4> and leaves three"""
    assert (R >= 1024 and R % 4 == 3) or (512 <= R < 1024 and R % 2 == 1)
    _step_hold(capsys, f"decoder step T={T} C={C} R={R}", E.step_case(T, C, R))


# ================================================================================================ greedy decode, end to end
def _greedy_hold(capsys, case, mode):
    from glass_amd._lib import lib
    from glass_amd.ops import native as K
    T, C, L, tie = case
    c = E.greedy_case(*case)
    want = c["want"]
    live, img = want["live"], c["roi_image"]
    # ---- what the comparison rests on, from the float64 reference alone
    assert len(img) <= 40 and float(want["gap"][live].min()) > E.GREEDY_GAP and c["same_path32"]
    if tie == "uniform":
        assert bool(live.all()) and bool((want["pred"] == 0).all()) and bool((want["ties"] == C).all())
    else:
        assert c["n_early"] > 0 and c["n_never"] > 0
        assert int(live[img == 0].sum(1).max()) <= min(2, L), "image 0 must break within its first two steps"
        assert bool(live[img == 2].all()), "image 2 must never break"
        if L > 2:
            assert not bool(live[img == 0][:, 2:].any())
    if tie not in (None, "uniform"):
        assert int(((want["ties"] == 2) & live).sum()) > 0, "the constructed tie must win some step"
    # ---- the kernel
    supported = lib().glass_decode_persistent_supported(T, 256, C, L)
    assert supported == (1 if case in E.GREEDY_BOTH else 0)
    d = _dev()
    w = RR.pack_decoder(c["plain"], d)
    K.recurrence_status(reset=True)
    got = K.attention_decode(c["x"].to(d), c["xproj"].to(d), w, img.to(d), 3, C, L, c["eos"], mode=mode).cpu()
    assert K.recurrence_status() == 0
    assert torch.equal(got.sum(-1) != 0, live), "zero rows after the per-image break differ"
    assert float(got[~live].abs().max() if bool((~live).any()) else 0.0) == 0.0
    _hold(capsys, f"greedy decode {mode} T={T} C={C} L={L} tie={tie} ({int(live.sum())} live rows)", got, want["probs"], c["err32"],
          E.DEC_PROJECT_BOUND)
    assert torch.equal(_first_argmax(got)[live], want["pred"][live])
    if tie == "uniform":
        assert bool((got == got[..., :1]).all()), "equal logits must give bit-equal probabilities"
    elif tie is not None:
        a, b = tie
        assert torch.equal(got[..., a], got[..., b]), "identical fc rows must give bit-equal probabilities"


@pytest.mark.parametrize("mode", ["steps", (1, 1)], ids=["steps", "persistent"])
@pytest.mark.parametrize("case", E.GREEDY_BOTH, ids=lambda c: "T%d-C%d-L%d-%s" % (c[0], c[1], c[2], c[3]))
def test_greedy_decode_against_float64(case, mode, capsys):
    """both decoders, three images (one breaks early, one never), exact ties across and inside the 64-lane slots, no RoI excluded:
    the float64 reference's top-2 gap exceeds 1e-4 at every live step (asserted), the bound is far below it"""
    _greedy_hold(capsys, case, mode)


@pytest.mark.parametrize("case", E.GREEDY_STEP_ONLY, ids=lambda c: "T%d-C%d-L%d-%s" % (c[0], c[1], c[2], c[3]))
def test_greedy_decode_outside_the_persistent_envelope_against_float64(case, capsys):
    """T > 32 or C > 128: glass_decode_persistent_supported says 0 and the step kernels are held to float64 (not to themselves)"""
    _greedy_hold(capsys, case, "steps")


# ================================================================================================ independence, non-finite inputs
def _others(t):
    keep = torch.tensor([i for i in range(E.POISON_R) if i != E.POISON_ROI], device=t.device)
    return t.index_select(0, keep).cpu()        # the poisoned RoI's rows are never read back


@pytest.mark.parametrize("poison", list(E.POISONS))
def test_fusion_attention_rois_are_independent(poison):
    x = torch.randn((E.POISON_R, 256, 512), generator=torch.Generator().manual_seed(61))
    w = E.fusion_weights(62)
    clean = _others(_fusion_run(x, w))
    bad = x.clone()
    bad[E.POISON_ROI, 100, 300] = E.POISONS[poison]
    assert torch.equal(_others(_fusion_run(bad, w)), clean)
    assert torch.equal(_others(_fusion_run(x, w)), clean), "a following ordinary call"


@pytest.mark.parametrize("poison", list(E.POISONS))
def test_bilstm_rois_are_independent(poison):
    from glass_amd.ops import native as K
    d = _dev()
    xg = (torch.randn((E.POISON_R, 32, 2, 1024), generator=torch.Generator().manual_seed(63)) * 1.5)
    whh = E.lstm_whh().to(d)
    bad = xg.clone()
    bad[E.POISON_ROI, 3, 1, 700] = E.POISONS[poison]
    bad[E.POISON_ROI, 9, 0, 5] = E.POISONS[poison]
    K.recurrence_status(reset=True)
    for mode in ("steps",) + PERSISTENT_MODES:
        clean = _others(K.bilstm_recurrence(xg.to(d), whh, 256, mode=mode))
        assert torch.equal(_others(K.bilstm_recurrence(bad.to(d), whh, 256, mode=mode)), clean), mode
        assert K.recurrence_status() == 0
        assert torch.equal(_others(K.bilstm_recurrence(xg.to(d), whh, 256, mode=mode)), clean), "a following ordinary call"
        assert bool(torch.isfinite(clean).all())


@pytest.mark.parametrize("mode", ["steps", (1, 1)], ids=["steps", "persistent"])
@pytest.mark.parametrize("poison", list(E.POISONS))
def test_decoder_rois_are_independent(poison, mode):
    """a NaN / +inf / 1e30 feature in RoI 5, alone in its image: the call completes, nothing is read back from RoI 5, every other
    RoI is bit-identical to the call without it (the greedy arg-max of a non-finite row is bound to [0, C) in the kernel)"""
    from glass_amd.ops import native as K
    d = _dev()
    T, C, L = 32, 97, 26
    plain = RR.make_decoder_plain(C, 64)
    w = RR.pack_decoder(plain, d)
    x = torch.randn((E.POISON_R, T, 256), generator=torch.Generator().manual_seed(65))
    bad = x.clone()
    bad[E.POISON_ROI, 7, 11] = E.POISONS[poison]
    img = torch.tensor(E.POISON_IMAGES, dtype=torch.int32, device=d)

    def run(v):
        out = K.attention_decode(v.to(d), RR.xproj_of(v, plain).to(d), w, img, 3, C, L, 0, mode=mode)
        torch.cuda.synchronize()
        return _others(out)
    K.recurrence_status(reset=True)
    clean = run(x)
    assert torch.equal(run(bad), clean)
    assert K.recurrence_status() == 0
    assert torch.equal(run(x), clean), "a following ordinary call"
    assert bool(torch.isfinite(clean).all()) and float(clean.sum()) > 0
