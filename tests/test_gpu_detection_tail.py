"""GPU: box_decode_kernel, nms_select_kernel (csrc/proposals.hip) and detections_finalize_kernel (csrc/detections.hip)
through their ops.native wrappers, against the float64 references of tests/detection_tail_cases.py.  Every case is
generated there with margins around each discontinuity (tests/test_detection_tail.py asserts them and holds the
references to the oracle), so kept sets and orders are compared exactly and no row is masked.  Each test prints its
worst measured error per field."""
import types

import numpy as np
import pytest
import torch

import detection_tail_cases as C

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _up(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).contiguous().to(_dev())


def _box_err(got, want, rtol, atol, what):
    """asserts |got - want| <= atol + rtol |want| per field (angle: circular difference); -> worst (xywh, angle) error"""
    got, want = np.asarray(got, dtype=np.float64).reshape(-1, 5), np.asarray(want, dtype=np.float64).reshape(-1, 5)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not len(got):
        return 0.0, 0.0
    d = np.abs(got[:, :4] - want[:, :4])
    da = np.abs(C.angle_diff(got[:, 4], want[:, 4]))
    assert np.all(d <= atol + rtol * np.abs(want[:, :4])), (what, float(d.max()))
    assert np.all(da <= atol + rtol * np.abs(want[:, 4])), (what, float(da.max()))
    return float(d.max()), float(da.max())


def _say(capsys, line):
    with capsys.disabled():
        print("\n" + line, end="")


# ------------------------------------------------------------------------------------------------ box decode
@pytest.mark.parametrize("wset", [0, 1])
@pytest.mark.parametrize("R", [1, 129, 300])
def test_box_decode_equals_float64_reference(R, wset, capsys):
    """clamp edge, angle wraps, saturated logits, orientation ties and non-finite deltas at fixed rows (decode_case).
    boxes rtol 1e-4 / atol 2e-3 (angles circular), probabilities 1e-6, argmax exact; a non-finite delta gives a
    non-finite box exactly where the reference has one and leaves every other row alone."""
    from glass_amd.ops import native as K
    c = C.decode_case(R, wset)
    boxes, fg, o2 = C.decode_ref(c["cls"], c["deltas"], c["orient"], c["props"], c["weights"])
    ob, ofg, oo = K.box_decode(_up(c["cls"]), _up(c["deltas"]), _up(c["orient"]), _up(c["props"]), c["weights"])
    ob, ofg, oo = ob.cpu().numpy(), ofg.cpu().numpy(), oo.cpu().numpy()
    assert ob.shape == (R, 5) and ofg.shape == (R,) and oo.shape == (R, 2)
    assert np.array_equal(np.isfinite(ob), np.isfinite(boxes)), np.argwhere(np.isfinite(ob) != np.isfinite(boxes)).tolist()
    fin = np.isfinite(boxes).all(axis=1)
    e_box, e_ang = _box_err(ob[fin], boxes[fin], 1e-4, 2e-3, "decoded boxes")
    part = ~fin
    if part.any():                                                     # the finite fields of a row with a non-finite one
        m = np.isfinite(boxes[part])
        assert np.all(np.abs(ob[part][m] - boxes[part][m]) <= 2e-3 + 1e-4 * np.abs(boxes[part][m]))
    e_fg, e_or = float(np.abs(ofg - fg).max()), float(np.abs(oo[:, 1] - o2[:, 1]).max())
    assert np.isfinite(ofg).all() and np.isfinite(oo).all()
    assert e_fg <= 1e-6 and e_or <= 1e-6, (e_fg, e_or)
    assert np.array_equal(oo[:, 0], o2[:, 0])
    _say(capsys, f"box_decode R={R} weights={c['weights']}: box {e_box:.2e} angle {e_ang:.2e} fg {e_fg:.2e} orient prob {e_or:.2e}")


# ------------------------------------------------------------------------------------------------ NMS select
def _nms(case, nms_thresh, post_topk, score_thresh=None, cat="case"):
    from glass_amd.ops import native as K
    cat = case["cat"] if isinstance(cat, str) else cat
    st = case["score_thresh"] if score_thresh is None else score_thresh
    args = (_up(case["boxes"]), _up(case["scores"]), None if cat is None else _up(cat, torch.int32), _up(case["valid_count"], torch.int32),
            _up(case["image_hw"], torch.int32), st, nms_thresh, post_topk, case["flags"])
    out = K.rotated_nms_select(*args)
    again = K.rotated_nms_select(*args)
    assert all(torch.equal(a, b) for a, b in zip(out, again)), "two launches on the same inputs differ"
    ref = C.nms_select_ref(case["boxes"], case["scores"], cat, case["valid_count"], case["image_hw"], st, nms_thresh, post_topk, case["flags"])
    return [t.cpu().numpy() for t in out], ref


def _check_nms(case, out, ref, post_topk, what):
    ob, os_, oi, oc = out
    assert ob.shape == (2, post_topk, 5) and os_.shape == (2, post_topk) and oi.shape == (2, post_topk)
    worst = (0.0, 0.0)
    for n in range(2):
        k = len(ref[n])
        assert int(oc[n]) == k, (what, n, int(oc[n]), k)
        assert oi[n, :k].tolist() == ref[n], (what, n)
        assert np.array_equal(os_[n, :k].view(np.int32), case["scores"][n][ref[n]].view(np.int32)), (what, n)      # bit for bit
        e = _box_err(ob[n, :k], C.nms_clipped_boxes(case, n, ref[n]), 1e-5, 1e-4, what)
        worst = (max(worst[0], e[0]), max(worst[1], e[1]))
        assert not ob[n, k:].any() and not os_[n, k:].any() and not oi[n, k:].any(), (what, n, "rows behind the count")
    return worst


@pytest.mark.parametrize("post_topk", C.DENSE_TOPKS)
@pytest.mark.parametrize("nms_thresh", C.DENSE_THRESHS)
def test_nms_select_dense_case(nms_thresh, post_topk, capsys):
    """S = 320 over five chunks, valid_count [320, 200] with NaN / inf / huge rows behind it; the cap 64 ends with the
    last candidate of chunk 0, the cap 100 inside a chunk (asserted on the CPU)"""
    case = C.dense_case()
    out, ref = _nms(case, nms_thresh, post_topk)
    e = _check_nms(case, out, ref, post_topk, f"dense {nms_thresh} {post_topk}")
    _say(capsys, f"nms dense thr={nms_thresh} topk={post_topk}: kept {[len(r) for r in ref]}, box {e[0]:.2e} angle {e[1]:.2e}")


def test_nms_select_categories_clip_drop_empty(capsys):
    """S = 300, three categories holding the same 100 boxes, CLIP | DROP_EMPTY on 120 x 160, logits as scores.
    Also the dense boxes under random categories (no clipping)."""
    case = C.category_case()
    out, ref = _nms(case, case["nms_thresh"], 1024)
    e = _check_nms(case, out, ref, 1024, "categories")
    for n in range(2):                                       # no category offset leaks into the output boxes
        assert np.abs(out[0][n, :len(ref[n]), :2]).max() < 400
    dense = C.dense_case()
    cat = np.random.default_rng(3).integers(0, 3, (2, 320)).astype(np.int32)
    for thr in C.DENSE_THRESHS:
        out2, ref2 = _nms(dense, thr, 1024, cat=cat)
        _check_nms(dense, out2, ref2, 1024, f"dense with categories {thr}")
    _say(capsys, f"nms categories: kept {[len(r) for r in ref]} of 300, box {e[0]:.2e} angle {e[1]:.2e}")


def test_nms_select_score_ties_and_duplicate_boxes(capsys):
    """8 exact score values (-0.0 and +0.0 among them) over bit-equal duplicate boxes: the lower slot wins"""
    case = C.tie_case()
    out, ref = _nms(case, case["nms_thresh"], 1024)
    e = _check_nms(case, out, ref, 1024, "ties")
    _say(capsys, f"nms ties: kept {[len(r) for r in ref]} of 150, box {e[0]:.2e} angle {e[1]:.2e}")


@pytest.mark.parametrize("score_thresh", [C.FILTER_THRESH, float("-inf")])
def test_nms_select_filters(score_thresh):
    """a non-finite score and a non-finite value in each box field drop the row; score == score_thresh is dropped;
    score_thresh = -inf keeps zero and negative scores"""
    case = C.filter_case()
    out, ref = _nms(case, case["nms_thresh"], 1024, score_thresh=score_thresh)
    _check_nms(case, out, ref, 1024, f"filters {score_thresh}")
    assert (18 in ref[0]) == (score_thresh < 0) and 19 in ref[0] and not set(ref[0]) & set(range(12, 18))


@pytest.mark.parametrize("S", C.SIZE_EDGES)
def test_nms_select_size_edges(S, capsys):
    case = C.size_case(S)
    out, ref = _nms(case, case["nms_thresh"], 1024)
    e = _check_nms(case, out, ref, 1024, f"S={S}")
    _say(capsys, f"nms S={S}: kept {[len(r) for r in ref]}, box {e[0]:.2e} angle {e[1]:.2e}")


def test_nms_select_identical_boxes_and_nothing_valid():
    case = C.identical_case()
    out, ref = _nms(case, 0.5, 1024)
    assert [len(r) for r in ref] == [1, 1]
    _check_nms(case, out, ref, 1024, "identical")
    case = C.nothing_valid_case()
    out, ref = _nms(case, 0.5, 1024)
    assert ref == [[], []]
    _check_nms(case, out, ref, 1024, "nothing valid")


def test_nms_select_8192_candidates_fill_the_kept_list(capsys):
    """S = 8192 (the largest accepted), post_topk = 1024: both images end with a full kept list"""
    case = C.big_case()
    out, ref = _nms(case, case["nms_thresh"], 1024)
    assert [len(r) for r in ref] == [1024, 1024]
    e = _check_nms(case, out, ref, 1024, "S=8192")
    _say(capsys, f"nms S=8192: kept {[len(r) for r in ref]}, box {e[0]:.2e} angle {e[1]:.2e}")


# ------------------------------------------------------------------------------------------------ detections finalize
def _text(case, row_shape, gap, seed):
    """[rows, *row_shape] random rows and roi_start: the prefix sums of the clamped counts, plus `gap` unused rows
    between consecutive images"""
    roi = case["roi_start"].astype(np.int64) + gap * np.arange(case["N"])
    rows = int(sum(case["clamped"])) + gap * case["N"]
    text = torch.rand((rows,) + tuple(row_shape), generator=torch.Generator().manual_seed(seed), dtype=torch.float32)
    return text, roi.astype(np.int32)


def _check_finalize(case, row_shape, gap, with_orient, do_filter_small, what):
    from glass_amd.ops import native as K
    text, roi = (None, None) if row_shape is None else _text(case, row_shape, gap, 5)
    ref = C.finalize_ref(case["boxes"], case["scores"], case["orient"] if with_orient else None, None, case["counts"], roi,
                         case["scale_xy"], case["out_hw"], case["min_box_dim"], do_filter_small)
    out = K.detections_finalize(_up(case["boxes"]), _up(case["scores"]), _up(case["orient"]) if with_orient else None,
                                None if text is None else text.to(_dev()), _up(case["counts"], torch.int32),
                                None if roi is None else _up(roi, torch.int32), _up(case["scale_xy"]), _up(case["out_hw"], torch.int32),
                                case["min_box_dim"], do_filter_small)
    ob, os_, oo, ot, oc = [None if t is None else t.cpu() for t in out]
    N, Kk = case["N"], case["K"]
    assert (oo is None) == (not with_orient) and (ot is None) == (text is None)
    assert ob.shape == (N, Kk, 5) and os_.shape == (N, Kk) and (ot is None or ot.shape == (N, Kk) + tuple(row_shape))
    assert oc.tolist() == [len(k) for k, _ in ref], (what, oc.tolist(), [len(k) for k, _ in ref])
    worst = (0.0, 0.0)
    for n in range(N):
        kept, boxes = ref[n]
        k = len(kept)
        idx = torch.from_numpy(kept)
        e = _box_err(ob[n, :k].numpy(), boxes, 1e-5, 1e-4, what)
        worst = (max(worst[0], e[0]), max(worst[1], e[1]))
        assert torch.equal(os_[n, :k], torch.from_numpy(case["scores"][n])[idx]), (what, n, "scores")
        assert not ob[n, k:].any() and not os_[n, k:].any(), (what, n, "padded tail")
        if with_orient:
            assert torch.equal(oo[n, :k], torch.from_numpy(case["orient"][n])[idx]) and not oo[n, k:].any(), (what, n, "orientations")
        if text is not None:
            assert torch.equal(ot[n, :k], text[int(roi[n]) + idx]) and not ot[n, k:].any(), (what, n, "text rows")
    return worst, oc.tolist()


@pytest.mark.parametrize("row_shape,gap,with_orient,do_filter_small", [
    ((3, 97), 0, True, True),            # TC = 291: odd, more than one 256-thread pass
    ((3, 97), 5, False, True),           # roi_start with a gap between the images, no orientations
    (None, 0, True, False),              # no text (one workgroup per image), no small-box filter
    ((28, 28), 0, False, True),          # mask-shaped rows, TC = 784
])
def test_detections_finalize_beyond_one_wavefront(row_shape, gap, with_orient, do_filter_small, capsys):
    """N = 4, K = 600, counts [600, 0, 257, 1000 -> K]; every wavefront of two 256-slot chunks mixes kept and dropped
    slots, one keeps all 64 and one none (asserted on the CPU); scales 1.5 x 2.0 and 0.625"""
    case = C.finalize_case()
    e, counts = _check_finalize(case, row_shape, gap, with_orient, do_filter_small, f"finalize {row_shape} gap {gap}")
    _say(capsys, f"detections_finalize K=600 rows={row_shape} gap={gap} orient={with_orient} filter={do_filter_small}: kept {counts}, "
                 f"box {e[0]:.2e} angle {e[1]:.2e}")


def test_detections_finalize_k1024_everything_kept(capsys):
    case = C.finalize_full_case()
    e, counts = _check_finalize(case, (3, 97), 0, True, True, "finalize K=1024")
    assert counts == [1024, 1000]
    _say(capsys, f"detections_finalize K=1024: kept {counts}, box {e[0]:.2e} angle {e[1]:.2e}")


# ------------------------------------------------------------------------------------------------ decode -> NMS chain
def test_box_decode_then_nms_select_equals_box_inference_oracle(capsys):
    """the two launches of RotatedFastRCNNOutputLayers.inference_batched on 2 x 300 proposal slots, counts [300, 180],
    thresholds 0.05 / 0.35, top 100, against glass_cpu.box_inference: kept slots exact, values within the bars of
    test_box_branch_matches_oracle_teacher_forced; and against the float64 chain (probabilities 1e-6)"""
    from glass_amd.ops import native as K
    from oracle import glass_cpu as O
    case, ch = C.chain_case(), C.CHAIN
    N, P, cnt = ch["N"], ch["P"], case["counts"].tolist()
    cfg = types.SimpleNamespace(
        MODEL=types.SimpleNamespace(ROI_BOX_HEAD=types.SimpleNamespace(BBOX_REG_WEIGHTS=ch["weights"]),
                                    ROI_HEADS=types.SimpleNamespace(SCORE_THRESH_TEST=ch["score_thresh"], NMS_THRESH_TEST=ch["nms_thresh"])),
        TEST=types.SimpleNamespace(DETECTIONS_PER_IMAGE=ch["topk"]))
    cat = lambda a: torch.cat([torch.from_numpy(a[n, : cnt[n]]) for n in range(N)])
    dets = O.box_inference(cat(case["cls"]), cat(case["deltas"]), cat(case["orient"]),
                           [torch.from_numpy(case["props"][n, : cnt[n]]) for n in range(N)], [ch["hw"]] * N, cfg)
    keep, boxes, fg, o2 = C.chain_ref(case)
    db, dfg, do2 = K.box_decode(_up(case["cls"].reshape(-1, 2)), _up(case["deltas"].reshape(-1, 5)), _up(case["orient"].reshape(-1, 4)),
                                _up(case["props"].reshape(-1, 5)), ch["weights"])
    ob, os_, oi, oc = K.rotated_nms_select(db.view(N, P, 5), dfg.view(N, P), None, _up(case["counts"], torch.int32),
                                           _up(case["image_hw"], torch.int32), ch["score_thresh"], ch["nms_thresh"], ch["topk"], K.NMS_CLIP)
    ob, os_, oi, oc, do2 = ob.cpu().numpy(), os_.cpu().numpy(), oi.cpu().numpy(), oc.cpu().numpy(), do2.view(N, P, 2).cpu().numpy()
    worst = [0.0, 0.0, 0.0, 0.0]
    for n in range(N):
        k = len(keep[n])
        assert int(oc[n]) == k == len(dets[n]["kept"])
        assert oi[n, :k].tolist() == dets[n]["kept"].tolist() == keep[n]
        e = _box_err(ob[n, :k], dets[n]["pred_boxes"].numpy(), 1e-4, 2e-3, "chain boxes vs oracle")
        want = np.array([C.clip_ref(boxes[n, s], *ch["hw"]) for s in keep[n]])
        e64 = _box_err(ob[n, :k], want, 1e-4, 2e-3, "chain boxes vs float64")
        got_or = do2[n, keep[n]]
        e_s, e_o = float(np.abs(os_[n, :k] - dets[n]["scores"].numpy()).max()), float(np.abs(got_or - dets[n]["orientations"].numpy()).max())
        assert e_s <= 1e-3 and e_o <= 1e-3
        e_s64, e_o64 = float(np.abs(os_[n, :k] - fg[n, keep[n]]).max()), float(np.abs(got_or[:, 1] - o2[n, keep[n], 1]).max())
        assert e_s64 <= 1e-6 and e_o64 <= 1e-6 and np.array_equal(got_or[:, 0], o2[n, keep[n], 0])
        assert not ob[n, k:].any() and not os_[n, k:].any() and not oi[n, k:].any()
        worst = [max(a, b) for a, b in zip(worst, (max(e[0], e64[0]), max(e[1], e64[1]), max(e_s, e_s64), max(e_o, e_o64)))]
    _say(capsys, f"decode -> nms chain: kept {[len(k) for k in keep]}, box {worst[0]:.2e} angle {worst[1]:.2e} score {worst[2]:.2e} "
                 f"orientation {worst[3]:.2e}")
