"""GPU: glass_merge_views (csrc/view_merge.hip) through ops.native.merge_views against the float64 reference of
tests/view_merge_cases.py - source slots, count and truncation flag exactly, scores bit for bit, boxes bit for bit against the
float32 replay of the frame transform - and GlassRunner.run_tiled against run_batch and against the same steps done by hand."""
import os

import numpy as np
import pytest
import torch

import view_merge_cases as C

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL = 7.25                      # what the caller's output rows hold before the call (rows beyond the count must keep it)


def _dev():
    return torch.device("cuda:0")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _run(case, max_out=None):
    from glass_amd.ops import native as K
    out = K.merge_views(_t(case["boxes"]), _t(case["scores"]), _t(case["counts"]), _t(case["xform"]), _t(case["keep"]),
                        _t(case["band"]), case["nms_thresh"], case["max_out"] if max_out is None else max_out)
    assert tuple(out) == ("boxes", "scores", "src", "count")
    return {k: v.cpu().numpy() for k, v in out.items()}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _assert_matches(out, ref, what):
    n = ref["count"]
    print(f"[merge_views] {what}: {ref['candidates']} candidates -> {n} kept, flag {ref['flag']}; kernel {out['count'].tolist()}")
    assert out["count"].tolist() == [n, ref["flag"]], what
    assert np.array_equal(out["src"][:n], ref["src"]), what
    assert np.array_equal(_bits(out["scores"][:n]), _bits(ref["scores"])), what
    assert np.array_equal(_bits(out["boxes"][:n]), _bits(ref["boxes"])), what
    assert not out["boxes"][n:].any() and not out["scores"][n:].any() and not out["src"][n:].any(), what     # the zeroed buffer


def test_one_view_identity():
    case = C.one_view_identity()
    out = _run(case)
    _assert_matches(out, case["ref"], "one view")
    assert out["count"].tolist() == [37, 0] and out["src"][:37].tolist() == list(range(37))
    assert np.array_equal(_bits(out["boxes"][:37]), _bits(case["boxes"][0, :37]))
    assert np.array_equal(_bits(out["scores"][:37]), _bits(case["scores"][0, :37]))


def test_two_views_duplicates():
    case = C.two_views_duplicates()
    out = _run(case)
    _assert_matches(out, case["ref"], "two views, every word in both")
    assert out["count"][0] == case["words"]


def test_same_view_pairs_survive():
    case = C.same_view_pairs()
    out = _run(case)
    _assert_matches(out, case["ref"], "IoU 0.9 pairs inside one view")
    assert out["count"][0] == int(case["counts"].sum())
    # the pairs are what a plain NMS would thin out: with the pairs' halves in DIFFERENT views one of each goes
    split = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in case.items()}
    split["boxes"][1, 10:22], split["scores"][1, 10:22] = case["boxes"][0, 1:24:2], case["scores"][0, 1:24:2]
    split["boxes"][0, 1:24:2, 2] = 0.0                                  # (w == 0: no candidate)
    split["counts"] = np.array([24, 22], dtype=np.int32)
    assert _run(split)["count"][0] == case["pairs"] + 10


def test_grid_3x3_plus_full_and_determinism():
    case = C.grid_3x3_plus_full()
    out = _run(case)
    _assert_matches(out, case["ref"], "3 x 3 tiles + the full view")
    again = _run(case)
    for k in out:
        assert np.array_equal(out[k].view(np.uint8), again[k].view(np.uint8)), k


def test_ties_are_ordered_by_view_then_slot():
    case = C.ties()
    _assert_matches(_run(case), case["ref"], "ties")


@pytest.mark.parametrize("cands,survivors", C.CHUNK_TOTALS)
def test_chunk_boundaries(cands, survivors):
    case = C.chunks(cands, survivors)
    out = _run(case)
    _assert_matches(out, case["ref"], f"{cands} candidates, {survivors} survivors")
    assert out["count"].tolist() == [survivors, 0]
    for cap in (survivors - 1, survivors):                             # the cap inside the last chunk / on its last survivor
        ref = C.merge_ref(case["boxes"], case["scores"], case["counts"], case["xform"], case["keep"], case["band"],
                          case["nms_thresh"], cap)
        _assert_matches(_run(case, cap), ref, f"{cands} candidates, max_out {cap}")


def test_cap_8x1024():
    case = C.cap_full()
    assert int(case["counts"].sum()) == 8192
    out = _run(case)
    _assert_matches(out, case["ref"], "8 x 1024, more than 1024 survivors")
    assert out["count"].tolist() == [1024, 1]
    twin = C.cap_exact()
    out = _run(twin)
    _assert_matches(out, twin["ref"], "8 x 1024 slots, exactly 1024 survivors, nothing after")
    assert out["count"].tolist() == [1024, 0]


def test_deep_duplicates():
    case = C.deep_duplicates()
    out = _run(case)
    _assert_matches(out, case["ref"], "400 words in all of 8 views")
    assert out["count"].tolist() == [400, 0]


def test_counts_edges():
    from glass_amd.ops import native as K
    case = C.counts_edges()
    _assert_matches(_run(case), case["ref"], "counts 0, negative, above K")
    dev = _dev()
    z = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)
    out = K.merge_views(z(0, 8, 5), z(0, 8), torch.zeros((0,), dtype=torch.int32, device=dev), z(0, 3), z(0, 4), z(0, 2), 0.5, 16)
    assert out["count"].tolist() == [0, 0] and not out["boxes"].any() and tuple(out["boxes"].shape) == (16, 5)
    empty = dict(case, counts=np.zeros((4,), dtype=np.int32))
    assert _run(empty)["count"].tolist() == [0, 0]


def test_nonfinite_and_empty_rows_are_no_candidates():
    case = C.nonfinite_and_empty()
    _assert_matches(_run(case), case["ref"], "NaN / inf / empty rows")


def test_rows_beyond_the_count_are_left_alone():
    """the C entry point itself, on outputs the caller filled"""
    from glass_amd import _lib
    from glass_amd.ops import native as K
    case = C.two_views_duplicates()
    dev = _dev()
    ob, os_ = torch.full((64, 5), FILL, device=dev), torch.full((64,), FILL, device=dev)
    src, cnt = torch.full((64,), -5, dtype=torch.int32, device=dev), torch.full((2,), -5, dtype=torch.int32, device=dev)
    L = _lib.lib()
    nb = int(L.glass_merge_views_workspace_bytes(2, 64))
    ws = torch.empty((nb,), dtype=torch.uint8, device=dev)
    ins = [_t(case[k]) for k in ("boxes", "scores", "counts", "xform", "keep", "band")]
    _lib.check(L.glass_merge_views(*[t.data_ptr() for t in ins], 2, 64, 0.5, 64, ob.data_ptr(), os_.data_ptr(), src.data_ptr(),
                                   cnt.data_ptr(), ws.data_ptr(), nb, K.stream_handle()))
    n = case["ref"]["count"]
    assert cnt.tolist() == [n, 0] and np.array_equal(src[:n].cpu().numpy(), case["ref"]["src"])
    assert bool((ob[n:] == FILL).all()) and bool((os_[n:] == FILL).all()) and bool((src[n:] == -5).all())


def test_wrapper_refuses():
    from glass_amd.ops import native as K
    case = C.counts_edges()
    good = dict(boxes=_t(case["boxes"]), scores=_t(case["scores"]), counts=_t(case["counts"]), view_xform=_t(case["xform"]),
                keep_rect=_t(case["keep"]), size_range=_t(case["band"]), nms_thresh=0.5, max_out=16)
    K.merge_views(**good)
    dev = _dev()
    bad = [("boxes", good["boxes"].double()), ("boxes", good["boxes"].cpu()), ("boxes", good["boxes"][:, :, :4].contiguous()),
           ("boxes", good["boxes"].reshape(-1, 5)), ("scores", good["scores"][:, :7].contiguous()), ("scores", good["scores"].half()),
           ("counts", good["counts"].long()), ("counts", good["counts"][:3].contiguous()), ("counts", good["counts"].cpu()),
           ("view_xform", good["view_xform"][:, :2].contiguous()), ("keep_rect", good["keep_rect"].cpu()),
           ("keep_rect", good["keep_rect"][:, :3].contiguous()), ("size_range", good["size_range"].double()),
           ("size_range", good["size_range"].t().contiguous()), ("boxes", good["boxes"].transpose(0, 1)),
           ("max_out", 0), ("max_out", 1025), ("nms_thresh", float("nan")), ("boxes", None)]
    for name, val in bad:
        with pytest.raises(ValueError, match="merge_views"):
            K.merge_views(**dict(good, **{name: val}))
    z = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)
    for V, Kk in ((9, 1024), (257, 8), (82, 100), (2, 1025)):
        with pytest.raises(ValueError, match="V \\* K <= 8192"):
            K.merge_views(z(V, Kk, 5), z(V, Kk), torch.zeros((V,), dtype=torch.int32, device=dev), z(V, 3), z(V, 4), z(V, 2), 0.5, 16)


# ------------------------------------------------------------------------------------------------ the runner
def _cfg(opts=()):
    from glass_amd.config import get_glass_cfg
    return get_glass_cfg(os.path.join(ROOT, "configs", "glass_icdar15_mi355x.yaml"), ["MODEL.DEVICE", "cuda:0"] + list(opts))


RUNNER_OPTS = ["INPUT.MIN_SIZE_TEST", 160, "INPUT.MAX_SIZE_TEST", 200, "POST_PROCESSING.TEXT_THRESHOLD", 0.0]


@pytest.fixture(scope="module")
def runner():
    from glass_amd.inference.glass_runner import GlassRunner
    from glass_amd.utils.synth import make_state_dict
    return GlassRunner(None, None, cfg=_cfg(RUNNER_OPTS), state_dict=make_state_dict(1234), post_process=True)


def _same_instances(a, b, what):
    assert len(a) == len(b), (what, len(a), len(b))
    assert a.image_size == b.image_size, what
    assert torch.equal(a.pred_boxes.tensor, b.pred_boxes.tensor) and torch.equal(a.scores, b.scores), what
    assert torch.equal(a.pred_text_prob, b.pred_text_prob), what
    if a.has("orientations") or b.has("orientations"):
        assert torch.equal(a.orientations, b.orientations), what
    if a.has("pred_polygons") or b.has("pred_polygons"):
        assert torch.equal(a.pred_polygons, b.pred_polygons) and a.pred_texts == b.pred_texts, what
        assert torch.equal(a.pred_text_scores, b.pred_text_scores), what


def test_run_tiled_with_one_tile_equals_run_batch(runner):
    """tile >= the resized image, scale = the policy ratio, no full view: the merge is the identity on the detections, and
    the result is run_batch's bit for bit"""
    from glass_amd.utils.synth import make_image
    for seed, (h, w) in ((5, (100, 80)), (9, (250, 180))):              # one image the policy enlarges, one it shrinks
        img = make_image(seed, h, w).numpy()
        rho = runner.get_inference_scale_ratio(img.shape)
        assert rho != 1
        ref = runner.run_batch([img])[0]
        got = runner.run_tiled(img, tile=256, overlap=64, border=8, scale=rho, full_view=False)
        assert len(ref) > 0
        print(f"[run_tiled = run_batch] {h} x {w}, ratio {rho:.3f}: {len(ref)} words")
        _same_instances(got, ref, (h, w))


def _by_hand(runner, img, tile, overlap, border, full_view, post_process, batch_size=8):
    """run_tiled's steps, spelled out: the model on the crops (one call) and on the full view, K.merge_views, the gather,
    process_padded"""
    from glass_amd.inference.tiling import plan_tiles
    from glass_amd.ops import native as K
    from glass_amd.structures.core import Instances, RotatedBoxes
    dev = runner.device
    H, W = img.shape[:2]
    work = runner._image_at_scale(img, 1)
    plan = plan_tiles(H, W, tile, overlap, border)
    L = float(plan.max_whole)
    inf = float("inf")
    crops = [{"image": work[:, t.y0:t.y0 + t.h, t.x0:t.x0 + t.w].contiguous(), "height": t.h, "width": t.w} for t in plan.tiles]
    dets = [runner.model(crops[i:i + batch_size]).batch for i in range(0, len(crops), batch_size)]
    xform = [[t.x0, t.y0, 1.0] for t in plan.tiles]
    keep = [list(t.keep) for t in plan.tiles]
    band = [[-inf, L if full_view else inf] for _ in plan.tiles]
    if full_view:
        full, rho = runner._image_to_tensor(img)
        dets.append(runner.model([{"image": full, "height": full.shape[1], "width": full.shape[2]}]).batch)
        xform.append([0.0, 0.0, 1.0 / rho])
        keep.append([-inf, -inf, inf, inf])
        band.append([L, inf])
    Kd = dets[0].scores.shape[1]
    T, Cc = runner.cfg.MODEL.ROI_RECOGNIZER_HEAD.MAX_WORD_LENGTH + 1, len(runner.cfg.MODEL.ROI_RECOGNIZER_HEAD.CHARACTER_SET) + 2

    def cat(name, tail=()):          # (a call without a single detection has no text rows)
        return torch.cat([getattr(d, name) if getattr(d, name) is not None else torch.zeros((len(d.counts_host), Kd) + tail, device=dev)
                          for d in dets], 0).contiguous()
    boxes, scores, orient, text, counts = cat("boxes"), cat("scores"), cat("orient"), cat("text", (T, Cc)), cat("counts_dev")
    V = scores.shape[0]
    f = lambda a: torch.tensor(a, dtype=torch.float32).to(dev)
    m = K.merge_views(boxes, scores, counts, f(xform), f(keep), f(band), float(runner.cfg.MODEL.ROI_HEADS.NMS_THRESH_TEST), 1024)
    src = m["src"].long()
    orient, text = orient.reshape(V * Kd, 2)[src][None], text.reshape((V * Kd,) + tuple(text.shape[2:]))[src][None]
    n = int(m["count"][0])
    if post_process:
        one = torch.ones((1, 2), dtype=torch.float32, device=dev)
        return runner.post_processor.process_padded(m["boxes"][None], m["scores"][None], m["count"][:1], text, one, [(H, W)],
                                                    {"orientations": orient, "pred_text_dist": None})[0], n, V
    r = Instances((H, W))
    r.pred_boxes, r.scores = RotatedBoxes(m["boxes"][:n]), m["scores"][:n]
    r.orientations, r.pred_text_prob = orient[0, :n], text[0, :n]
    return r, n, V


@pytest.mark.parametrize("full_view", [True, False])
def test_run_tiled_equals_the_steps_by_hand(runner, full_view):
    from glass_amd.utils.synth import make_image
    img = make_image(3, 160, 224).numpy()
    args = dict(tile=128, overlap=64, border=8, full_view=full_view)
    ref, n, V = _by_hand(runner, img, 128, 64, 8, full_view, True)
    assert V == 6 + int(full_view) and n > 0 and len(ref) > 0
    got = runner.run_tiled(img, **args)
    print(f"[run_tiled = by hand] full_view={full_view}: {V} views, {n} merged detections, {len(ref)} words")
    _same_instances(got, ref, full_view)
    assert got.image_size == (160, 224)
    if not full_view:                                                  # the tiles in two model calls of 4 and 2
        ref4, n4, _ = _by_hand(runner, img, 128, 64, 8, full_view, True, batch_size=4)
        assert n4 > 0
        _same_instances(runner.run_tiled(img, batch_size=4, **args), ref4, "batch_size 4")
    raw, n2, _ = _by_hand(runner, img, 128, 64, 8, full_view, False)
    runner.post_process_flag = False
    try:
        got = runner.run_tiled(img, **args)
    finally:
        runner.post_process_flag = True
    assert n2 == n == len(got)
    _same_instances(got, raw, "post_process=False")


def test_run_tiled_refusals(runner):
    from glass_amd.utils.synth import make_image
    img = make_image(3, 160, 224).numpy()
    heads = runner.model.roi_heads
    with pytest.raises(ValueError, match="tile=.* fits"):
        runner.run_tiled(make_image(1, 600, 3000).numpy(), tile=64, overlap=16, border=4)      # 11 x 62 tiles of 100 slots
    heads.mask_inference = True
    try:
        with pytest.raises(NotImplementedError, match="MASK_INFERENCE"):
            runner.run_tiled(img, tile=128, overlap=64, border=8)
    finally:
        heads.mask_inference = False
    head = heads.recognizer_head
    before = head.image_segments
    head.image_segments = torch.zeros((8,), dtype=torch.int32, device=runner.device)
    try:
        with pytest.raises(NotImplementedError, match="image_segments"):
            runner.run_tiled(img, tile=128, overlap=64, border=8)
    finally:
        head.image_segments = before
