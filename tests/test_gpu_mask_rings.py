"""GPU: the device mask polygoniser (csrc/mask_rings.hip through ops.native.mask_rings and MaskPolygonizer) against its
two sources of expected values: the host tracer glass_amd.evaluation.masks_to_polygons (whole ring lists equal, vertex for
vertex) and the boundary-free checker of tests/mask_ring_cases.py.  Every generated mask is compared, the empty ones too."""
from unittest import mock

import numpy as np
import pytest
import torch

import mask_ring_cases as C

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _compare(masks, what, check=True):
    """masks bool [R, H, W] (numpy) -> the device rings, after comparing them with both sources"""
    from glass_amd.evaluation import MaskPolygonizer, masks_to_polygons
    got = MaskPolygonizer(_dev())(torch.from_numpy(np.ascontiguousarray(masks)).to(_dev()))
    want = masks_to_polygons(masks)
    assert len(got) == len(want) == len(masks), what
    for r, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"{what}, mask {r}: device ring of {len(g)} vertices, host ring of {len(w)}; first difference at " \
                       f"{next((i for i, (a, b) in enumerate(zip(g, w)) if a != b), min(len(g), len(w)))}"
        if check:
            C.check_ring(masks[r], g)
    return got


def test_hand_made_shapes_one_mask_per_call_and_batched():
    cases = C.hand_made()
    for name, m in cases:
        _compare(m[None], name)
    H, W = max(m.shape[0] for _, m in cases), max(m.shape[1] for _, m in cases)
    batch = np.zeros((len(cases), H + 3, W + 5), dtype=bool)                   # all of them in one call, off the origin
    for k, (_, m) in enumerate(cases):
        batch[k, 2:2 + m.shape[0], 3:3 + m.shape[1]] = m
    rings = _compare(batch, "hand-made batch")
    names = [n for n, _ in cases]
    assert rings[names.index("rectangle")] == [[5.0, 3.0], [9.0, 3.0], [9.0, 6.0], [5.0, 6.0], [5.0, 3.0]]
    assert rings[names.index("empty")] == []
    assert rings[names.index("equal sizes")][0] == [10.0, 3.0]                 # the tie goes to the larger region that starts first
    assert rings[names.index("larger region inside a smaller ring")][0] == [5.0, 4.0]
    assert rings[names.index("smaller region inside a larger ring")][:2] == [[3.0, 2.0], [15.0, 2.0]]
    assert len(rings[names.index("checkerboard")]) == 5


def test_uint8_masks_any_non_zero_value_is_set():
    from glass_amd.evaluation import MaskPolygonizer, masks_to_polygons
    rng = np.random.RandomState(3)
    m = (rng.rand(7, 23, 37) < 0.6) * rng.randint(1, 256, size=(7, 23, 37))
    got = MaskPolygonizer(_dev())(torch.from_numpy(m.astype(np.uint8)).to(_dev()))
    assert got == masks_to_polygons(m != 0)
    assert MaskPolygonizer(_dev())(m != 0) == got                              # a numpy array is uploaded


def test_seeded_noise_every_mask_compared():
    total = empty = 0
    for name, masks in C.noise_batches():
        rings = _compare(masks, name)
        total += len(rings)
        empty += sum(1 for r in rings if r == [])
    assert total > 500 and empty > 10
    assert max(len(masks) for _, masks in C.noise_batches()) == 300


def test_perimeter_of_the_order_of_the_area():
    for name, m in (("serpentine 61 x 67", C.serpentine(61, 67)), ("serpentine 40 x 300", C.serpentine(40, 300)),
                    ("comb 90 x 201", C.comb(90, 201)), ("comb 130 x 64", C.comb(130, 64))):
        ring = np.array(_compare(m[None], name)[0])
        assert np.abs(np.diff(ring, axis=0)).sum() >= m.sum(), name              # the outline is as long as the region is large
    yy, xx = np.mgrid[0:70, 0:70]
    stairs = np.abs(yy - xx) <= 1                                                # a vertex at every pixel corner of the outline
    assert len(_compare(stairs[None], "staircase")[0]) > 250


def test_window_too_large_for_lds_is_traced_from_global_memory():
    from glass_amd.ops import native as K
    big = C.big_window(1600)
    assert C.lds_words(big) == 1600 * 25 > K.MASK_RINGS_LDS_WORDS              # the bitmap does not fit: the fallback runs
    small = np.zeros_like(big); small[100:160, 200:500] = C.comb(60, 300)
    assert 0 < C.lds_words(small) <= K.MASK_RINGS_LDS_WORDS                    # and the LDS path in the same call
    serp = np.zeros_like(big); serp[:600, :700] = C.serpentine(600, 700)       # fallback with a long walk: 600 x 11 words
    assert C.lds_words(serp) > K.MASK_RINGS_LDS_WORDS
    rings = _compare(np.stack([big, small, np.zeros_like(big), serp]), "1600 x 1600")
    assert len(rings[0]) > 1500 and rings[2] == []


def _realistic(dev):
    from glass_amd.ops import native as K
    from glass_amd.utils.synth import make_boxes
    H = W = 1000
    probs = torch.from_numpy(C.word_masks(100, 28, 7))
    boxes = make_boxes(5, 100, H, W)
    return K.paste_rotated_masks(probs.to(dev), boxes.to(dev), (H, W), 0.5)


def test_realistic_pasted_word_masks():
    from glass_amd.evaluation import MaskPolygonizer, masks_to_polygons
    from glass_amd.ops import native as K
    dev = _dev()
    pasted = _realistic(dev)
    assert pasted.dtype == torch.bool and tuple(pasted.shape) == (100, 1000, 1000)
    got = MaskPolygonizer(dev)(pasted)
    host = pasted.cpu().numpy()
    want = masks_to_polygons(host)
    assert got == want
    for m, ring in zip(host, got):
        C.check_ring(m, ring)
    lens = [len(r) for r in got]
    print(f"realistic case: {sum(1 for n in lens if n)} non-empty rings, mean {np.mean(lens):.0f} vertices, longest {max(lens)}; "
          f"largest window {max(C.lds_words(m) for m in host)} LDS words of {K.MASK_RINGS_LDS_WORDS}")
    assert max(lens) > 100 and max(C.lds_words(m) for m in host) <= K.MASK_RINGS_LDS_WORDS   # the common path is the LDS one


def test_two_calls_return_identical_tensors():
    from glass_amd.ops import native as K
    dev = _dev()
    rng = np.random.RandomState(11)
    masks = torch.from_numpy(rng.rand(64, 67, 131) < 0.55).to(dev)
    xy1, off1 = K.mask_rings(masks)
    xy2, off2 = K.mask_rings(masks)
    assert xy1.dtype == off1.dtype == torch.int32 and xy1.shape[1] == 2 and off1.shape == (65,)
    assert torch.equal(xy1, xy2) and torch.equal(off1, off2) and int(off1[-1]) == xy1.shape[0] > 0
    pasted = _realistic(dev)
    a, b = K.mask_rings(pasted), K.mask_rings(pasted)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_no_masks_no_launch_and_bad_input_raises_before_a_launch():
    from glass_amd._lib import GlassLibraryError
    from glass_amd.evaluation import MaskPolygonizer
    from glass_amd.ops import native as K
    dev = _dev()
    ok = torch.zeros((2, 8, 8), dtype=torch.bool, device=dev)
    with mock.patch.object(K, "lib", side_effect=AssertionError("launched")):
        xy, off = K.mask_rings(torch.zeros((0, 8, 8), dtype=torch.bool, device=dev))
        assert tuple(xy.shape) == (0, 2) and off.tolist() == [0]
        assert MaskPolygonizer(dev)(np.zeros((0, 5, 5), dtype=bool)) == []
        for bad in (ok.cpu(), ok.float(), ok.to(torch.int32), torch.zeros((2, 8, 16), dtype=torch.bool, device=dev)[:, :, ::2],
                    ok[0], torch.zeros((2, 0, 8), dtype=torch.bool, device=dev)):
            with pytest.raises(GlassLibraryError):
                K.mask_rings(bad)
    assert MaskPolygonizer(dev)(ok) == [[], []]


def test_writer_totaltext_det_zip_and_scores_equal_the_host_path():
    from glass_amd.evaluation import MaskPolygonizer, RRCScorer, TextResultWriter, masks_to_polygons
    from test_gpu_rrc_score import _writer_case
    dev = _dev()
    enc, inputs, outputs, gt = _writer_case("totaltext", 12, 10, True)
    host = TextResultWriter(enc, dataset="totaltext", masks_to_polygons=masks_to_polygons)
    host.process(inputs, outputs)
    for out in outputs:                                                        # as the model leaves them: on the device
        inst = out["instances"]
        if len(inst):
            inst.pred_masks = inst.pred_masks.to(dev)
    device = TextResultWriter(enc, dataset="totaltext", masks_to_polygons=MaskPolygonizer(dev))
    device.process(inputs, outputs)
    assert device.coco_results() == host.coco_results()
    with mock.patch("time.time", return_value=1_700_000_000.0):
        za = host.det_zip(host.to_eval_format(host.coco_results(), 0.5, 0.4))
        zb = device.det_zip(device.to_eval_format(device.coco_results(), 0.5, 0.4))
    assert za == zb and len(za) > 200
    scorer = RRCScorer(gt, False, dev)
    a, b = host.evaluate(scorer, 0.5, 0.4), device.evaluate(scorer, 0.5, 0.4)
    assert a == b and a["DETECTION_ONLY_RESULTS"]["hmean"] > 0
