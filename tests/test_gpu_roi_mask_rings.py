"""GPU: mask polygons straight from the RoI masks (csrc/mask_rings.hip through ops.native.roi_mask_rings and
MaskPolygonizer.from_rois) against the two-step path on the same build (paste_rotated_masks + mask_rings: bit-equal), against
the reference's own pasted golden traced on the host, and through the model, the writer, run_batch and run_tiled."""
import os
from unittest import mock

import numpy as np
import pytest
import torch

import roi_mask_cases as RC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _two_step(masks, boxes, hw, t):
    from glass_amd.ops import native as K
    pasted = K.paste_rotated_masks(masks, boxes, hw, t)
    return pasted, K.mask_rings(pasted)


def _assert_equal(got, want, what):
    assert got[0].dtype == want[0].dtype == torch.int32 and got[1].dtype == torch.int32, what
    assert torch.equal(got[1], want[1]), (what, "ring_off")
    assert torch.equal(got[0], want[0]), (what, "xy")


@pytest.fixture(scope="module")
def on_device():
    """[(case, masks, boxes, pasted, (xy, ring_off) of the two-step path)], computed once"""
    dev = _dev()
    out = []
    for c in RC.cases():
        masks, boxes = torch.from_numpy(c["masks"]).to(dev), torch.from_numpy(c["boxes"]).to(dev)
        pasted, rings = _two_step(masks, boxes, c["hw"], c["threshold"])
        out.append((c, masks, boxes, pasted, rings))
    return out


def test_batched_rings_windows_and_rectangles_equal_the_two_step_path(on_device):
    from glass_amd.ops import native as K
    rings = nonempty = 0
    for c, masks, boxes, pasted, want in on_device:
        got = K.roi_mask_rings(masks, boxes, c["hw"], c["threshold"])
        _assert_equal(got, want, c["name"])
        # the rectangle the kernels used contains every pasted pixel; so does the host statement
        host = pasted.cpu().numpy()
        rects = K.roi_mask_device_rects(boxes, c["M"], c["hw"]).cpu().numpy()
        assert RC.outside(host, rects) == 0, c["name"]
        assert RC.outside(host, K.roi_mask_rects(c["boxes"], c["M"], c["hw"])) == 0, c["name"]
        bad = ~np.isfinite(c["boxes"]).all(axis=1)
        assert (rects[bad, 2] < rects[bad, 0]).all() and not host[bad].any(), c["name"]
        live = rects[:, 2] >= rects[:, 0]
        assert (rects[live, :2] >= 0).all() and (rects[live, 2] < c["hw"][1]).all() and (rects[live, 3] < c["hw"][0]).all(), c["name"]
        # and the tightened windows are the ones the byte form finds in the pasted tensor
        win = torch.empty((len(boxes), 4), dtype=torch.int32, device=_dev())
        K.check(K.lib().glass_mask_windows(pasted.data_ptr(), len(boxes), c["hw"][0], c["hw"][1], win.data_ptr(), K.stream_handle()))
        assert torch.equal(K.roi_mask_windows(masks, boxes, c["hw"], c["threshold"]), win), c["name"]
        off = want[1].cpu().numpy()
        rings += len(off) - 1
        nonempty += int((np.diff(off) > 0).sum())
    print(f"[roi_mask_rings] {rings} masks, {nonempty} non-empty rings, all equal to paste + mask_rings")
    assert nonempty > 200 and rings - nonempty > 100


def test_one_mask_per_call_equals_the_batch(on_device):
    from glass_amd.ops import native as K
    for c, masks, boxes, pasted, want in on_device:
        xy, off = want[0].cpu(), want[1].cpu().tolist()
        for r in range(len(boxes)):
            got = K.roi_mask_rings(masks[r:r + 1], boxes[r:r + 1], c["hw"], c["threshold"])
            assert got[1].tolist() == [0, off[r + 1] - off[r]], (c["name"], r)
            assert torch.equal(got[0].cpu(), xy[off[r]:off[r + 1]]), (c["name"], r)


def test_the_large_window_takes_the_global_memory_walk_and_the_shapes_are_what_they_claim(on_device):
    import mask_ring_cases as C
    from glass_amd.evaluation import masks_to_polygons
    from glass_amd.ops import native as K
    c, masks, boxes, pasted, want = on_device[-1]
    host = pasted.cpu().numpy()
    assert C.lds_words(host[0]) > K.MASK_RINGS_LDS_WORDS and 0 < C.lds_words(host[3]) <= K.MASK_RINGS_LDS_WORDS
    assert host[3].any(axis=0).sum() > 64                              # wider than one 64-column label segment
    off = want[1].cpu().tolist()
    xy = want[0].cpu().numpy().astype(np.float64)
    rings = [xy[a:b].tolist() for a, b in zip(off[:-1], off[1:])]
    assert rings == masks_to_polygons(host)                            # (the byte form's own tests: here only that the case is live)
    for m, ring in zip(host, rings):
        C.check_ring(m, ring)
    # on the first case: the two-blob mask's ring starts in the second blob, the equal blobs' in the first
    c, masks, boxes, pasted, want = on_device[0]
    host = pasted.cpu().numpy()
    off = want[1].cpu().tolist()
    xy = want[0].cpu().numpy()
    for r in range(len(boxes)):
        C.check_ring(host[r], xy[off[r]:off[r + 1]].astype(np.float64).tolist())


def test_reference_golden_rings(golden_dir):
    """expected values that owe nothing to this repository's kernels: the reference's own pasted masks, traced on the host"""
    from glass_amd.evaluation import MaskPolygonizer, masks_to_polygons
    from glass_amd.ops import native as K
    g = np.load(os.path.join(golden_dir, "mask_paste.npz"), allow_pickle=False)
    masks, boxes, hw = g["masks"].astype(np.float32), g["boxes"].astype(np.float32), (int(g["H"]), int(g["W"]))
    out_bool = np.unpackbits(g["out_bool"])[: len(boxes) * hw[0] * hw[1]].reshape(len(boxes), *hw).astype(bool)
    dev = _dev()
    got = MaskPolygonizer(dev).from_rois(masks, boxes, hw, 0.5)
    want = masks_to_polygons(out_bool)
    pasted = K.paste_rotated_masks(torch.from_numpy(masks).to(dev), torch.from_numpy(boxes).to(dev), hw, 0.5).cpu().numpy()
    same = (pasted == out_bool).reshape(len(masks), -1).all(axis=1)
    print(f"[golden] {len(masks)} masks on {hw}, {int((~same).sum())} with a pasted pixel that differs from the golden")
    assert len(got) == len(want) == len(masks) and sum(1 for r in want if r) > 0
    for r in np.nonzero(same)[0]:
        assert got[r] == want[r], r
    assert same.all(), "a pasted pixel differs from the reference's golden: the rings of those masks could not be compared"


def test_two_calls_return_identical_tensors(on_device):
    from glass_amd.ops import native as K
    for c, masks, boxes, pasted, want in on_device[:1] + on_device[-1:]:
        a = K.roi_mask_rings(masks, boxes, c["hw"], c["threshold"])
        b = K.roi_mask_rings(masks, boxes, c["hw"], c["threshold"])
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and int(a[1][-1]) == a[0].shape[0] > 0


def test_trivial_and_bad_inputs():
    from glass_amd._lib import GlassLibraryError
    from glass_amd.evaluation import MaskPolygonizer
    from glass_amd.ops import native as K
    dev = _dev()
    masks = torch.full((3, 28, 28), 0.9, device=dev)
    boxes = torch.tensor([[20.0, 20, 10, 6, 0]] * 3, device=dev)
    with mock.patch.object(K, "lib", side_effect=AssertionError("launched")):
        xy, off = K.roi_mask_rings(masks[:0], boxes[:0], (40, 60))
        assert tuple(xy.shape) == (0, 2) and xy.dtype == torch.int32 and off.tolist() == [0]
        assert MaskPolygonizer(dev).from_rois(np.zeros((0, 28, 28), np.float32), np.zeros((0, 5), np.float32), (40, 60)) == []
        for args in ((masks.cpu(), boxes, (40, 60)), (masks, boxes.cpu(), (40, 60)), (masks.double(), boxes, (40, 60)),
                     (masks > 0.5, boxes, (40, 60)), (masks[:, :, :14], boxes, (40, 60)), (masks[:, ::2], boxes, (40, 60)),
                     (masks[0], boxes, (40, 60)), (masks, boxes[:2], (40, 60)), (masks, boxes[:, :4], (40, 60)),
                     (masks, boxes, (0, 60)), (masks, boxes, (40, 65536)), (masks, boxes, (65535, 65535)),
                     (masks, boxes, (40, 60), 0.0), (masks, boxes, (40, 60), -0.5), (masks, boxes, (40, 60), float("nan"))):
            with pytest.raises(GlassLibraryError):
                K.roi_mask_rings(*args)
        for bad in (boxes[:, :4].contiguous(), boxes[0], boxes.cpu(), boxes.double()):
            with pytest.raises(GlassLibraryError):
                K.roi_mask_device_rects(bad, 28, (40, 60))
    # every mask empty: zeros, a box outside the image, a non-finite box
    boxes = torch.tensor([[20.0, 20, 10, 6, 0], [-50.0, 20, 10, 6, 0], [float("nan"), 20, 10, 6, 0]], device=dev)
    masks = torch.stack([torch.zeros((28, 28), device=dev), masks[0], masks[0]])
    xy, off = K.roi_mask_rings(masks, boxes, (40, 60))
    assert tuple(xy.shape) == (0, 2) and off.tolist() == [0, 0, 0, 0]
    assert MaskPolygonizer(dev).from_rois(masks, boxes, (40, 60)) == [[], [], []]
    # a known answer: an all-ones mask in an axis-aligned 10 x 6 box covers the pixels whose centres the inflated box holds
    ring = MaskPolygonizer(dev).from_rois(masks[1:2].cpu().numpy(), [[20.0, 20, 10, 6, 0]], (40, 60))
    assert ring == [[[15.0, 17.0], [25.0, 17.0], [25.0, 23.0], [15.0, 23.0], [15.0, 17.0]]]


def test_memory_stays_far_below_the_pasted_tensor():
    """64 small boxes on 4096 x 4096: pasted they are 1 GiB; the RoI form may add R * H * W / 16 bytes = 64 MiB at the most
    (its workspace is 8 bytes per window pixel: at most about 64 x 210^2 x 8 = 22 MiB)"""
    from glass_amd.ops import native as K
    dev = _dev()
    m, b, hw = RC.memory_case()
    masks, boxes = torch.from_numpy(m).to(dev), torch.from_numpy(b).to(dev)
    R, (H, W) = len(boxes), hw
    assert (R, H, W) == (64, 4096, 4096) and b[:, 2].max() <= 200 and b[:, 3].max() <= 40
    K.roi_mask_rings(masks[:2], boxes[:2], hw)                          # (the library is loaded and the allocator warm)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    got = K.roi_mask_rings(masks, boxes, hw)
    torch.cuda.synchronize()
    added = torch.cuda.max_memory_allocated() - before
    print(f"[memory] roi_mask_rings on {R} x {H} x {W}: peak {added / 2 ** 20:.2f} MiB above the inputs (pasted: {R * H * W / 2 ** 20:.0f} MiB)")
    assert added < R * H * W // 16
    assert int(got[1][-1]) > 64 * 4
    _, want = _two_step(masks, boxes, hw, 0.5)                          # afterwards: this is the gigabyte
    _assert_equal(got, want, "memory case")


# ------------------------------------------------------------------------------------------------ through the model
def _cfg(opts=()):
    from glass_amd.config import get_glass_cfg
    return get_glass_cfg(os.path.join(ROOT, "configs", "glass_icdar15_mi355x.yaml"),
                         ["MODEL.DEVICE", "cuda:0", "MODEL.ROI_MASK_HEAD.MASK_INFERENCE", True, "MODEL.MASK_ON", True,
                          "MODEL.ROI_MASK_HEAD.PASTE_MASKS", False] + list(opts))


PARTS = ("backbone", "rpn", "box", "recog", "mask")


def test_end_to_end_paste_masks_false_writes_the_same_det_zip():
    import glass_amd
    from glass_amd.evaluation import MaskPolygonizer, TextResultWriter
    from glass_amd.modeling.recognition.text_encoder import TextEncoder
    from glass_amd.postprocess import build_post_processor
    from glass_amd.utils.synth import make_boxes, make_image, make_state_dict
    dev = _dev()
    cfg = _cfg()
    model = glass_amd.build_model(cfg)
    model.load_state_dict(make_state_dict(1234, parts=PARTS))
    assert model.paste_masks is False
    sizes = [(192, 256), (224, 224)]
    imgs = [make_image(40 + i, h, w).permute(2, 0, 1).float().contiguous() for i, (h, w) in enumerate(sizes)]
    boxes = [make_boxes(50 + i, 6, h, w) for i, (h, w) in enumerate(sizes)]
    inputs = [{"image": im.to(dev), "height": int(h * 1.25), "width": int(w * 1.25), "file_name": f"{i:07d}.jpg"}
              for i, (im, (h, w)) in enumerate(zip(imgs, sizes))]
    enc = TextEncoder(cfg)
    zips, results, outs = [], [], []
    for paste in (False, True):
        model.paste_masks = paste                                      # what MODEL.ROI_MASK_HEAD.PASTE_MASKS sets
        post = model.inference(inputs, override_boxes=[b.to(dev) for b in boxes])
        for o in post:
            # the synthetic recogniser is unsure of every character and the writer drops such words: give every detection a
            # confident text, the same in both runs, so the lines with the polygons reach the det.zip
            inst = o["instances"]
            labels = enc.encode(["word%d" % k for k in range(len(inst))])[:, 1:]
            prob = torch.full((len(inst), labels.shape[1], len(enc.character)), 0.001)
            inst.pred_text_prob = prob.scatter_(2, labels.unsqueeze(-1), 0.9).to(dev)
        outs.append(post)
        writer = TextResultWriter(enc, dataset="totaltext", masks_to_polygons=MaskPolygonizer(dev))
        writer.process(inputs, post)
        results.append(writer.coco_results())
        with mock.patch("time.time", return_value=1_700_000_000.0):
            zips.append(writer.det_zip(writer.to_eval_format(results[-1], 0.0, 0.0)))
    rois, pasted = outs
    for a, b in zip(rois, pasted):
        a, b = a["instances"], b["instances"]
        assert a.has("pred_mask_rois") and a.has("pred_mask_boxes") and not a.has("pred_masks") and a.has("pred_rboxes")
        assert b.has("pred_masks") and not b.has("pred_mask_rois")
        assert tuple(a.pred_mask_rois.shape) == (len(a), 28, 28) and a.pred_mask_rois.dtype == torch.float32
        assert torch.equal(a.pred_mask_boxes, a.pred_boxes.tensor) and torch.equal(a.pred_boxes.tensor, b.pred_boxes.tensor)
        assert MaskPolygonizer(dev).from_rois(a.pred_mask_rois, a.pred_mask_boxes, a.image_size) == MaskPolygonizer(dev)(b.pred_masks)
    print(f"[end to end] {sum(len(o['instances']) for o in rois)} detections, {len(results[0])} records, det.zip of {len(zips[0])} bytes")
    assert results[0] == results[1] and zips[0] == zips[1] and len(results[0]) > 0 and len(zips[0]) > 200
    assert any(len(r["polys"]) > 4 for r in results[0])                # mask rings, not box polygons
    # the word post-processor keeps one row per word, gathered like any other field
    inst = rois[0]["instances"]
    words = build_post_processor(_cfg(["POST_PROCESSING.TEXT_THRESHOLD", 0.0]))(inst)
    assert len(words) > 0 and words.pred_mask_rois.shape[0] == words.pred_mask_boxes.shape[0] == len(words)
    assert tuple(words.pred_mask_rois.shape[1:]) == (28, 28) and isinstance(words.pred_mask_boxes, torch.Tensor)
    rows = {r.numpy().tobytes() for r in inst.pred_mask_rois.cpu()}
    assert all(r.numpy().tobytes() in rows for r in words.pred_mask_rois.cpu())


RUNNER_OPTS = ["INPUT.MIN_SIZE_TEST", 160, "INPUT.MAX_SIZE_TEST", 200, "POST_PROCESSING.TEXT_THRESHOLD", 0.0]


@pytest.fixture(scope="module")
def runner():
    from glass_amd.inference.glass_runner import GlassRunner
    from glass_amd.utils.synth import make_state_dict
    return GlassRunner(None, None, cfg=_cfg(RUNNER_OPTS), state_dict=make_state_dict(1234, parts=PARTS), post_process=True)


def _scaled(boxes, s):
    return boxes * torch.tensor([s, s, s, s, 1.0], dtype=torch.float32, device=boxes.device)


def test_run_batch_carries_the_rois_in_the_original_frame(runner):
    from glass_amd.evaluation import MaskPolygonizer
    from glass_amd.utils.synth import make_image
    dev = runner.device
    img = make_image(9, 250, 180).numpy()                              # the policy shrinks it: the boxes are scaled back
    rho = runner.get_inference_scale_ratio(img.shape)
    assert rho != 1
    got = runner.run_batch([img])[0]
    assert len(got) > 0 and got.image_size == (250, 180) and not got.has("pred_masks")
    assert tuple(got.pred_mask_rois.shape) == (len(got), 28, 28) and tuple(got.pred_mask_boxes.shape) == (len(got), 5)
    # by hand: the model's raw mask rows (a detection is known by its row), and the boxes the model's own post-processing leaves
    # in the resized image's frame (filtered, clipped), scaled to the original image
    t, _ = runner._image_to_tensor(img)
    inputs = [{"image": t, "height": t.shape[1], "width": t.shape[2]}]
    raw = runner.model.inference(inputs, do_postprocess=False)[0]
    assert raw.has("pred_masks") and tuple(raw.pred_masks.shape[1:]) == (1, 28, 28)
    raw_rows = {r.numpy().tobytes() for r in raw.pred_masks[:, 0].cpu()}
    inst = runner.model.inference(inputs)[0]["instances"]
    assert all(r.numpy().tobytes() in raw_rows for r in inst.pred_mask_rois.cpu())
    hand_boxes = _scaled(inst.pred_boxes.tensor, 1.0 / rho)
    poly = MaskPolygonizer(dev)
    hand = poly.from_rois(inst.pred_mask_rois, hand_boxes, (250, 180))
    by_row = {r.numpy().tobytes(): (ring, b) for r, ring, b in zip(inst.pred_mask_rois.cpu(), hand, hand_boxes.cpu())}
    mine = poly.from_rois(got.pred_mask_rois, got.pred_mask_boxes, got.image_size)
    assert len(mine) == len(got)
    for b, row, ring in zip(got.pred_mask_boxes.cpu(), got.pred_mask_rois.cpu(), mine):
        want_ring, want_box = by_row[row.numpy().tobytes()]
        assert ring == want_ring and torch.equal(b, want_box)
    assert any(len(r) > 4 for r in mine)


def test_run_tiled_with_one_tile_equals_run_batch_on_the_mask_fields(runner):
    from glass_amd.utils.synth import make_image
    img = make_image(9, 250, 180).numpy()
    rho = runner.get_inference_scale_ratio(img.shape)
    ref = runner.run_batch([img])[0]
    got = runner.run_tiled(img, tile=256, overlap=64, border=8, scale=rho, full_view=False)
    assert len(ref) == len(got) > 0 and torch.equal(got.pred_boxes.tensor, ref.pred_boxes.tensor)
    assert torch.equal(got.pred_mask_rois, ref.pred_mask_rois) and torch.equal(got.pred_mask_boxes, ref.pred_mask_boxes)


def test_without_word_post_processing_the_mask_boxes_are_the_scaled_boxes_once(runner):
    """post_process_flag False and a scale other than 1: run_batch and run_tiled scale pred_boxes in place; pred_mask_boxes is
    those boxes in the original image's pixels - scaled once, not left in the resized frame, not scaled twice"""
    from glass_amd.evaluation import MaskPolygonizer
    from glass_amd.utils.synth import make_image
    img = make_image(9, 250, 180).numpy()
    rho = runner.get_inference_scale_ratio(img.shape)
    assert rho != 1
    t, _ = runner._image_to_tensor(img)
    inst = runner.model.inference([{"image": t, "height": t.shape[1], "width": t.shape[2]}])[0]["instances"]
    resized = inst.pred_boxes.tensor.clone()                           # the resized image's frame
    runner.post_process_flag = False
    try:
        batch = runner.run_batch([img])[0]
        tiled = runner.run_tiled(img, tile=256, overlap=64, border=8, scale=rho, full_view=False)
    finally:
        runner.post_process_flag = True
    for what, got in (("run_batch", batch), ("run_tiled", tiled)):
        assert len(got) == len(resized) > 0 and got.image_size == (250, 180), what
        assert torch.equal(got.pred_mask_boxes, got.pred_boxes.tensor), what
        assert got.pred_mask_boxes.data_ptr() != got.pred_boxes.tensor.data_ptr(), what
    # centre and extents grew by 1 / rho, once (run_batch keeps the model's order; the merge of run_tiled orders by score)
    ratio = (batch.pred_mask_boxes[:, :4] / resized[:, :4]).cpu().numpy()
    np.testing.assert_allclose(ratio, 1.0 / rho, rtol=1e-5)
    assert torch.equal(batch.pred_mask_rois, inst.pred_mask_rois)
    rows = lambda g: sorted((tuple(b), r.numpy().tobytes()) for b, r in zip(g.pred_mask_boxes.tolist(), g.pred_mask_rois.cpu()))
    assert rows(tiled) == rows(batch)
    rings = MaskPolygonizer(runner.device).from_rois(tiled.pred_mask_rois, tiled.pred_mask_boxes, tiled.image_size)
    assert any(len(r) > 4 for r in rings)


def test_run_tiled_2x2_gathers_the_mask_rows_by_src(runner):
    from glass_amd.inference.tiling import plan_tiles
    from glass_amd.ops import native as K
    from glass_amd.utils.synth import make_image
    dev = runner.device
    img = make_image(3, 192, 192).numpy()
    tile, overlap, border = 128, 64, 8
    plan = plan_tiles(192, 192, tile, overlap, border)
    assert len(plan.tiles) == 4
    work = runner._image_at_scale(img, 1)
    crops = [{"image": work[:, t.y0:t.y0 + t.h, t.x0:t.x0 + t.w].contiguous(), "height": t.h, "width": t.w} for t in plan.tiles]
    det = runner.model(crops).batch
    assert det.mask_rois is not None and tuple(det.mask_rois.shape[2:]) == (28, 28)
    V, Kd = det.scores.shape
    inf = float("inf")
    f = lambda a: torch.tensor(a, dtype=torch.float32).to(dev)
    m = K.merge_views(det.boxes.contiguous(), det.scores.contiguous(), det.counts_dev.contiguous(),
                      f([[t.x0, t.y0, 1.0] for t in plan.tiles]), f([list(t.keep) for t in plan.tiles]), f([[-inf, inf]] * 4),
                      float(runner.cfg.MODEL.ROI_HEADS.NMS_THRESH_TEST), 1024)
    n = int(m["count"][0])
    assert n > 0
    want = det.mask_rois.reshape(V * Kd, 28, 28)[m["src"].long()][:n]
    runner.post_process_flag = False
    try:
        got = runner.run_tiled(img, tile=tile, overlap=overlap, border=border, full_view=False)
    finally:
        runner.post_process_flag = True
    assert len(got) == n and torch.equal(got.pred_mask_rois, want) and torch.equal(got.pred_mask_boxes, m["boxes"][:n])
    print(f"[run_tiled 2 x 2] {n} merged detections from tiles {sorted({int(s) // Kd for s in m['src'][:n].tolist()})}")
    words = runner.run_tiled(img, tile=tile, overlap=overlap, border=border, full_view=False)
    assert len(words) > 0 and words.pred_mask_rois.shape[0] == words.pred_mask_boxes.shape[0] == len(words)
