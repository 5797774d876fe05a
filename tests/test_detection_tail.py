"""CPU: the float64 references of tests/detection_tail_cases.py against the oracle (oracle/d2ops.py, oracle/glass_cpu.py),
the margins of every generated case, and the structural properties that give the GPU tests of
tests/test_gpu_detection_tail.py their teeth (chunk boundaries of nms_select_kernel, wavefront boundaries of
detections_finalize_kernel)."""
import types

import numpy as np
import pytest
import torch

import detection_tail_cases as C
from oracle import d2ops
from oracle import glass_cpu as O


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _assert_boxes(got, want, rtol, atol, what):
    got, want = np.asarray(got, dtype=np.float64).reshape(-1, 5), np.asarray(want, dtype=np.float64).reshape(-1, 5)
    assert got.shape == want.shape, what
    np.testing.assert_allclose(got[:, :4], want[:, :4], rtol=rtol, atol=atol, err_msg=what)
    d = np.abs(C.angle_diff(got[:, 4], want[:, 4]))
    assert np.all(d <= atol + rtol * np.abs(want[:, 4])), (what, float(d.max()) if d.size else 0.0)


# ------------------------------------------------------------------------------------------------ box decode
@pytest.mark.parametrize("wset", [0, 1])
@pytest.mark.parametrize("R", [1, 129, 300])
def test_decode_ref_equals_oracle_apply_deltas_and_softmax(R, wset):
    c = C.decode_case(R, wset)
    boxes, fg, o2 = C.decode_ref(c["cls"], c["deltas"], c["orient"], c["props"], c["weights"])
    ob = d2ops.apply_deltas_rotated(_t(c["deltas"]), _t(c["props"]), c["weights"]).numpy()
    assert np.array_equal(np.isfinite(boxes), np.isfinite(ob))
    fin = np.isfinite(boxes).all(axis=1)
    _assert_boxes(boxes[fin], ob[fin], 1e-4, 2e-3, "decode_ref vs apply_deltas_rotated")
    probs = torch.softmax(_t(c["cls"]), dim=-1).numpy()
    assert np.abs(probs[:, 0] - fg).max() <= 1e-6
    om = torch.softmax(_t(c["orient"]), dim=-1).max(dim=1)
    assert np.array_equal(om[1].numpy(), o2[:, 0].astype(np.int64))
    assert np.abs(om[0].numpy() - o2[:, 1]).max() <= 1e-6
    # the case has what it claims
    assert C.orient_margin_ok(c["orient"])
    assert np.isfinite(fg).all() and np.isfinite(o2).all()
    if R > 1:
        assert len(c["special_slots"]) == 29 and c["special_slots"][-1] == R - 1
        assert len(c["nonfinite_rows"]) == 8 and not np.isfinite(boxes[c["nonfinite_rows"]]).all(axis=1).any()
        clamp = boxes[c["clamp_rows"], 2:4] / c["props"][c["clamp_rows"], 2:4].astype(np.float64)
        assert np.all(np.isclose(clamp.max(axis=1), 1000.0 / 16, rtol=1e-6))          # at or above the clamp: exp(SCALE_CLAMP)
        wraps = np.abs(c["deltas"][:, 4].astype(np.float64) / c["weights"][4]) * 180.0 / np.pi
        assert (wraps > 3 * 360).sum() >= 2 and ((wraps > 360) & (wraps < 2 * 360)).sum() >= 2
        ties = [r for r in range(R) if np.sum(c["orient"][r] == c["orient"][r].max()) > 1]
        assert len(ties) == 4 and {int(o2[r, 0]) for r in ties} == {0, 1, 2}           # first maximum
        assert fg.max() == 1.0 and fg.min() < 1e-40


# ------------------------------------------------------------------------------------------------ NMS select
def _oracle_plain(case, n, nms_thresh, cat=None):
    """d2ops.nms_rotated / batched_nms_rotated over the valid, above-threshold rows of image n (flags == 0 cases)"""
    cnt = int(case["valid_count"][n])
    b, s = case["boxes"][n][:cnt], case["scores"][n][:cnt]
    assert np.isfinite(b).all() and np.isfinite(s).all()
    idx = np.flatnonzero(s > np.float32(case["score_thresh"]))
    if cat is None:
        keep = d2ops.nms_rotated(b[idx], s[idx], nms_thresh)
    else:
        keep = d2ops.batched_nms_rotated(_t(b[idx]), _t(s[idx]), _t(cat[n][:cnt][idx].astype(np.int64)), nms_thresh)
    return [int(idx[k]) for k in keep.tolist()]


def _ref(case, nms_thresh=None, post_topk=None, cat="case", score_thresh=None):
    return C.nms_select_ref(case["boxes"], case["scores"], case["cat"] if isinstance(cat, str) else cat, case["valid_count"],
                            case["image_hw"], case["score_thresh"] if score_thresh is None else score_thresh,
                            case["nms_thresh"] if nms_thresh is None else nms_thresh,
                            case.get("post_topk", 1024) if post_topk is None else post_topk, case["flags"])


def _distinct(case):
    for n in range(2):
        s = case["scores"][n][: int(case["valid_count"][n])]
        s = s[np.isfinite(s)]
        if len(np.unique(s)) != len(s):
            return False
    return True


def _detail(case, n, nms_thresh, post_topk):
    return C.nms_image_detail(case["boxes"][n], case["scores"][n], None if case["cat"] is None else case["cat"][n],
                              case["valid_count"][n], case["image_hw"][n], case["score_thresh"], nms_thresh, post_topk, case["flags"])


def test_dense_case_margins_oracle_and_chunk_teeth():
    case = C.dense_case()
    assert case["boxes"].shape == (2, 320, 5) and case["valid_count"].tolist() == [320, 200]
    assert C.nms_margin_violations(case, C.DENSE_THRESHS) == [] and _distinct(case)
    assert not np.array_equal(case["boxes"][0, :200], case["boxes"][1, :200])
    for thr in C.DENSE_THRESHS:
        full = _ref(case, thr, 1024)
        assert [full[n] == _oracle_plain(case, n, thr) for n in range(2)] == [True, True]
        for topk in C.DENSE_TOPKS:
            assert _ref(case, thr, topk) == [k[:topk] for k in full]
        d = _detail(case, 0, thr, 1 << 30)
        nsurv, kept = len(d["order"]), d["kept_pos"]
        assert nsurv > 256 and len(kept) > 100 and len(d["sup_by"]) >= 30, (thr, nsurv, len(kept), len(d["sup_by"]))
        # a candidate of a later chunk suppressed only by boxes kept in earlier chunks; one suppressed only inside its own chunk
        assert any(p >= 64 and all(q // 64 < p // 64 for q in qs) for p, qs in d["sup_by"].items())
        assert any(all(q // 64 == p // 64 for q in qs) for p, qs in d["sup_by"].items())
        # post_topk = 64 is reached by the last candidate of a chunk, post_topk = 100 strictly inside one, with more to come
        assert kept[63] % 64 == 63
        assert kept[99] % 64 not in (0, 63) and kept[99] // 64 == kept[100] // 64
    d35, d70 = _detail(case, 0, 0.35, 1 << 30), _detail(case, 0, 0.7, 1 << 30)
    assert d35["keep"] != d70["keep"] and len(d70["sup_by"]) >= 30               # the jittered copies give 0.7 its teeth
    print(f"dense: kept {len(d35['kept_pos'])} at 0.35, {len(d70['kept_pos'])} at 0.7 of {len(d35['order'])} surviving rows")


def test_dense_case_with_categories_equals_batched_nms_rotated():
    case = C.dense_case()
    cat = np.random.default_rng(3).integers(0, 3, (2, 320)).astype(np.int32)
    for thr in C.DENSE_THRESHS:
        ref = _ref(case, thr, 1024, cat=cat)
        assert ref != _ref(case, thr, 1024)
        for n in range(2):
            assert ref[n] == _oracle_plain(case, n, thr, cat=cat)


def _oracle_rrpn(case, n):
    """the filter / clip / batched_nms body of d2ops.find_top_rrpn_proposals with one 'level' per category; its result
    carries no indices, so the kept rows are found again by their (distinct) scores"""
    cnt = int(case["valid_count"][n])
    b, s, c = case["boxes"][n][:cnt], case["scores"][n][:cnt], case["cat"][n][:cnt]
    levels = [np.flatnonzero(c == k) for k in range(3)]
    res = d2ops.find_top_rrpn_proposals([_t(b[ix])[None] for ix in levels], [_t(s[ix])[None] for ix in levels],
                                        [tuple(int(v) for v in case["image_hw"][n])], case["nms_thresh"], 1 << 20, case["post_topk"])
    slot = {float(v): i for i, v in enumerate(s)}
    return [slot[float(v)] for v in res[0][1].tolist()], res[0][0].numpy()


def test_category_case_margins_and_rrpn_oracle():
    case = C.category_case()
    assert case["boxes"].shape == (2, 300, 5) and case["flags"] == C.NMS_CLIP | C.NMS_DROP_EMPTY
    assert C.nms_margin_violations(case) == [] and _distinct(case)
    assert (case["scores"][0] < 0).sum() > 100 and (case["scores"][0] > 0).sum() > 20
    ref = _ref(case)
    for n in range(2):
        keep, boxes = _oracle_rrpn(case, n)
        assert ref[n] == keep
        _assert_boxes(C.nms_clipped_boxes(case, n, keep), boxes, 1e-5, 1e-4, "clipped boxes vs oracle")
    # every box once per category: a category decides alone (the result of each equals a run on its rows only), rows
    # are clipped, some become empty, and the categories do not all keep the same boxes
    d = _detail(case, 0, case["nms_thresh"], 1 << 30)
    raw = case["boxes"][0].astype(np.float64)
    assert len(d["order"]) < 300 and (300 - len(d["order"])) % 3 == 0                               # dropped as empty
    clipped = [s for s in d["order"] if not np.allclose(C.norm_angle(raw[s, 4]), raw[s, 4]) or not np.array_equal(raw[s, :4], C.clip_ref(raw[s], 120, 160)[:4])]
    assert len(clipped) >= 30
    kept_base = [sorted(int(case["base"][s]) for s in ref[0] if case["cat"][0][s] == k) for k in range(3)]
    assert kept_base[0] != kept_base[1] or kept_base[1] != kept_base[2]
    assert all(0 < len(k) < len(d["order"]) // 3 for k in kept_base)
    for k in range(3):
        only = case["scores"][0].copy()
        only[case["cat"][0] != k] = -np.inf
        alone = C.nms_image_detail(case["boxes"][0], only, None, 300, case["image_hw"][0], -1e30, case["nms_thresh"], 1024, case["flags"])
        assert alone["keep"] == [s for s in ref[0] if case["cat"][0][s] == k]


def test_tie_case_margins_and_oracle():
    case = C.tie_case()
    assert C.nms_margin_violations(case) == []
    s0 = case["scores"][0]
    assert set(np.unique(s0).tolist()) <= set(C.TIE_VALUES) and (np.signbit(s0) & (s0 == 0)).any() and (~np.signbit(s0) & (s0 == 0)).any()
    ref = _ref(case)
    for n in range(2):
        assert ref[n] == _oracle_plain(case, n, case["nms_thresh"])
    # a -0.0 row is kept ahead of a +0.0 row with a higher slot, and bit-equal boxes with equal scores leave the lower slot
    d = _detail(case, 0, case["nms_thresh"], 1 << 30)
    order = d["order"]
    z = [s for s in order if s0[s] == 0]
    assert z == sorted(z) and len({bool(np.signbit(s0[s])) for s in z}) == 2
    b0 = case["boxes"][0]
    won = [(order[qs[0]], order[p]) for p, qs in d["sup_by"].items() if np.array_equal(b0[order[qs[0]]], b0[order[p]]) and s0[order[qs[0]]] == s0[order[p]]]
    assert len(won) >= 3 and all(a < b for a, b in won)


def _oracle_fast_rcnn(boxes, scores, hw, score_thresh, nms_thresh, topk):
    """glass_cpu.fast_rcnn_inference_single_image_rotated on one image's valid rows -> kept source rows, boxes"""
    probs = np.stack([scores, np.zeros_like(scores)], axis=1)                     # (fg, bg): the last column is dropped
    ok = np.isfinite(boxes).all(axis=1) & np.isfinite(scores)
    out = O.fast_rcnn_inference_single_image_rotated(_t(boxes), _t(probs), None, tuple(int(v) for v in hw), score_thresh, nms_thresh, topk)
    return [int(np.flatnonzero(ok)[k]) for k in out["kept"].tolist()], out["pred_boxes"].numpy()


@pytest.mark.parametrize("score_thresh", [C.FILTER_THRESH, float("-inf")])
def test_filter_case_equals_fast_rcnn_inference_oracle(score_thresh):
    case = C.filter_case()
    assert C.nms_margin_violations(case) == []
    ref = _ref(case, score_thresh=score_thresh)
    for n in range(2):
        cnt = int(case["valid_count"][n])
        keep, boxes = _oracle_fast_rcnn(case["boxes"][n][:cnt], case["scores"][n][:cnt], case["image_hw"][n], score_thresh,
                                        case["nms_thresh"], 1024)
        assert ref[n] == keep
        _assert_boxes(C.nms_clipped_boxes(case, n, keep), boxes, 1e-5, 1e-4, "filter case boxes")
    k0 = set(ref[0])
    assert not k0 & set(range(12, 18)) and set(range(0, 6)) <= k0               # non-finite rows gone, their healthy twins stay
    assert 19 in k0
    assert (18 in k0) == (score_thresh < 0) and ({20, 21, 22, 23} <= k0) == (score_thresh < 0)
    assert np.isnan(case["scores"][0][12]) and all(not np.isfinite(case["boxes"][0][13 + k, k]) for k in range(5))


@pytest.mark.parametrize("S", C.SIZE_EDGES)
def test_size_cases_margins_and_oracle(S):
    case = C.size_case(S)
    assert case["boxes"].shape == (2, S, 5) and case["valid_count"].tolist() == [S, S * 5 // 8]
    assert C.nms_margin_violations(case) == [] and _distinct(case)
    ref = _ref(case)
    for n in range(2):
        assert ref[n] == _oracle_plain(case, n, case["nms_thresh"])
    if S == 1:
        assert ref == [[0], []]
    if S >= 64:
        d = _detail(case, 0, case["nms_thresh"], 1 << 30)
        assert len(d["sup_by"]) >= S // 8 and len(d["order"]) > (S * 9) // 10


def test_identical_and_nothing_valid_cases():
    case = C.identical_case()
    ref = _ref(case)
    assert ref == [[int(np.argmax(case["scores"][0]))], [int(np.argmax(case["scores"][1][:40]))]]
    assert [ref[n] == _oracle_plain(case, n, 0.5) for n in range(2)] == [True, True]
    assert _ref(C.nothing_valid_case()) == [[], []]


def test_big_case_margins_fills_the_kept_list_and_equals_oracle():
    case = C.big_case()
    assert case["boxes"].shape == (2, 8192, 5)
    assert C.nms_margin_violations(case) == [] and _distinct(case)
    ref = _ref(case)
    assert [len(k) for k in ref] == [1024, 1024]
    d = _detail(case, 0, case["nms_thresh"], 1024)
    assert len(d["order"]) > 7500 and len(d["sup_by"]) >= 50 and d["kept_pos"][-1] >= 1024 + 50
    # greedy NMS: the first kept rows depend on the better-scored rows only, so the oracle runs on the best 2048 of each image
    for n in range(2):
        cnt = int(case["valid_count"][n])
        best = np.sort(np.argsort(-case["scores"][n][:cnt], kind="stable")[:2048])
        keep = d2ops.nms_rotated(case["boxes"][n][best], case["scores"][n][best], case["nms_thresh"]).tolist()
        assert len(keep) > 1024 and ref[n] == [int(best[k]) for k in keep[:1024]]


# ------------------------------------------------------------------------------------------------ detections finalize
def _oracle_postprocess(case, n, do_filter_small):
    cnt = case["clamped"][n]
    det = {"pred_boxes": _t(case["boxes"][n, :cnt]), "scores": _t(case["scores"][n, :cnt]), "orientations": _t(case["orient"][n, :cnt])}
    out = O.meta_postprocess(det, case["in_hw"][n], tuple(int(v) for v in case["out_hw"][n]), case["min_box_dim"] if do_filter_small else 0)
    slot = {float(v): j for j, v in enumerate(case["scores"][n, :cnt])}
    kept = [slot[float(v)] for v in out["scores"].tolist()]
    assert torch.equal(out["orientations"], det["orientations"][kept])
    return kept, out["pred_boxes"].numpy()


def _finalize_ref(case, do_filter_small):
    return C.finalize_ref(case["boxes"], case["scores"], case["orient"], None, case["counts"], case["roi_start"], case["scale_xy"],
                          case["out_hw"], case["min_box_dim"], do_filter_small)


@pytest.mark.parametrize("do_filter_small", [True, False])
def test_finalize_ref_equals_meta_postprocess_oracle(do_filter_small):
    for case in (C.finalize_case(), C.finalize_full_case()):
        ref = _finalize_ref(case, do_filter_small)
        for n in range(case["N"]):
            kept, boxes = _oracle_postprocess(case, n, do_filter_small)
            assert ref[n][0].tolist() == kept
            _assert_boxes(ref[n][1], boxes, 1e-5, 1e-4, "finalize_ref vs meta_postprocess")


def test_finalize_case_margins_and_wavefront_teeth():
    case = C.finalize_case()
    assert case["counts"].tolist() == [600, 0, 257, 1000] and case["clamped"] == [600, 0, 257, 600] and case["K"] == 600
    assert case["scale_xy"].tolist() == [[1.5, 2.0], [1.0, 1.0], [0.625, 0.625], [1.5, 2.0]]
    for c in (case, C.finalize_full_case()):
        for n in range(c["N"]):
            for j in range(c["clamped"][n]):
                assert C.finalize_margin_ok(c["boxes"][n, j].astype(np.float64), float(c["scale_xy"][n, 0]), float(c["scale_xy"][n, 1]),
                                            int(c["out_hw"][n, 0]), int(c["out_hw"][n, 1])), (n, j)
    ref = _finalize_ref(case, True)
    counts = [len(k) for k, _ in ref]
    assert counts[1] == 0 and any(c % 8 for c in counts) and counts != [len(k) for k, _ in _finalize_ref(case, False)]
    tables = {n: C.wave_keep_table(ref[n][0], case["clamped"][n]) for n in (0, 2, 3)}
    mixed_chunks = {(n, ch) for n, t in tables.items() for ch in {k[0] for k in t}
                    if all((ch, w) in t and t[(ch, w)][0] > 0 and t[(ch, w)][1] > 0 for w in range(4))}
    assert len({ch for _, ch in mixed_chunks}) >= 2 and (0, 0) in mixed_chunks and (0, 1) in mixed_chunks, mixed_chunks
    assert tables[0][(2, 0)] == (64, 0) and tables[3][(0, 1)] == (0, 64)
    assert tables[2][(1, 0)] == (1, 0)                                          # the lone slot of the second chunk of image 2
    b = case["boxes"]
    edge = [(n, j) for n in (0, 2, 3) for j in ref[n][0] if min(b[n, j, 2], b[n, j, 3]) == case["min_box_dim"]]
    assert len(edge) >= 20                                                      # min(w, h) == min_box_dim exactly is kept
    for a in C.FINALIZE_ANGLES:
        assert (b[0, :600, 4] == np.float32(a)).sum() >= 10
    clipped = sum(1 for n in (0, 2, 3) for j, nb in zip(*ref[n]) if abs(nb[4]) <= 1 and (nb[2] < b[n, j, 2] * case["scale_xy"][n, 0] * 0.999))
    assert clipped >= 20
    full = _finalize_ref(C.finalize_full_case(), True)
    assert [len(k) for k, _ in full] == [1024, 1000]


# ------------------------------------------------------------------------------------------------ chain
def test_chain_case_margins_and_box_inference_oracle():
    case = C.chain_case()
    keep, boxes, fg, o2 = C.chain_ref(case)
    N, P = C.CHAIN["N"], C.CHAIN["P"]
    cfg = types.SimpleNamespace(
        MODEL=types.SimpleNamespace(ROI_BOX_HEAD=types.SimpleNamespace(BBOX_REG_WEIGHTS=C.CHAIN["weights"]),
                                    ROI_HEADS=types.SimpleNamespace(SCORE_THRESH_TEST=C.CHAIN["score_thresh"], NMS_THRESH_TEST=C.CHAIN["nms_thresh"])),
        TEST=types.SimpleNamespace(DETECTIONS_PER_IMAGE=C.CHAIN["topk"]))
    cnt = case["counts"].tolist()
    cat = lambda a: torch.cat([_t(a[n, : cnt[n]]) for n in range(N)])
    dets = O.box_inference(cat(case["cls"]), cat(case["deltas"]), cat(case["orient"]), [_t(case["props"][n, : cnt[n]]) for n in range(N)],
                           [C.CHAIN["hw"]] * N, cfg)
    assert C.orient_margin_ok(case["orient"])
    for n in range(N):
        assert keep[n] == dets[n]["kept"].tolist() and 20 <= len(keep[n]) <= C.CHAIN["topk"]
        want = np.array([C.clip_ref(boxes[n, s], *C.CHAIN["hw"]) for s in keep[n]])
        _assert_boxes(want, dets[n]["pred_boxes"].numpy(), 1e-4, 2e-3, "chain boxes")
        assert np.abs(fg[n, keep[n]] - dets[n]["scores"].numpy()).max() <= 1e-6
        assert np.array_equal(o2[n, keep[n], 0], dets[n]["orientations"][:, 0].numpy())
        assert np.abs(o2[n, keep[n], 1] - dets[n]["orientations"][:, 1].numpy()).max() <= 1e-6
        # margins of the decoded rows
        f = np.sort(fg[n, : cnt[n]])
        assert np.diff(f).min() >= 1e-5 and np.abs(f - float(np.float32(C.CHAIN["score_thresh"]))).min() >= 1e-4
        alive = fg[n, : cnt[n]] > C.CHAIN["score_thresh"]
        E = np.array([C.clip_ref(b, *C.CHAIN["hw"]) for b in boxes[n, : cnt[n]]])
        assert C.iou_margin_violations(E, (C.CHAIN["nms_thresh"],), alive=alive) == []
        assert all(C.clip_margin_ok(b, *C.CHAIN["hw"]) for b in boxes[n, : cnt[n]])
        assert sum(1 for s in keep[n] if abs(boxes[n, s, 4]) <= 1) >= 1 and (~alive).sum() >= 3
    assert len(keep[0]) == C.CHAIN["topk"]                                     # the cap is reached on the full image
