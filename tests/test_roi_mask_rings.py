"""CPU: the host side of mask polygons from RoI masks - the per-feature header and its binding, the candidate rectangle
(ops.native.roi_mask_rects) held against the CPU oracle's paste on every seeded case, how instances_to_coco_json hands
`pred_mask_rois` to a callback, the cfg key, and run_tiled's refusal."""
import ctypes
import os
import re
import types
from unittest import mock

import numpy as np
import pytest
import torch

import roi_mask_cases as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["glass_roi_mask_rects", "glass_roi_mask_windows", "glass_roi_mask_rings_count"]


def _header(name):
    with open(os.path.join(ROOT, "include", name)) as fh:
        return fh.read()


def test_header_names_exported_declared_once_and_closed_headers_unchanged():
    from glass_amd import _lib
    text = _header("glass_hip_feature_roimask.h")
    assert '#include "glass_hip.h"' in text
    assert list(_lib.signatures(text)) == NAMES
    for name in NAMES:
        assert _lib.FEATURE_EXPORTS.count(name) == 1 and name not in _lib.EXPORTS + _lib.EXT_EXPORTS + _lib.ADDON_EXPORTS, name
    for other in ("glass_hip.h", "glass_hip_ext.h", "glass_hip_ext_views.h"):
        assert "glass_roi_mask" not in _header(other), other
    assert "glass_hip_feature_roimask.h" in [os.path.basename(p) for p in _lib.feature_headers()]
    # the two closed headers: the same sets of prototypes as before, and the ABI version with them
    assert len(_lib.EXPORTS) == 105 and _lib.ABI_VERSION == 8
    assert _lib.EXT_EXPORTS == ["glass_beam_search_lexicon_workspace_bytes", "glass_beam_search_lexicon"]
    _lib.build_library()
    L = _lib.lib()
    p, i, l, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float
    assert L.glass_roi_mask_rects.argtypes == [p, i, i, i, i, p, p]
    assert L.glass_roi_mask_windows.argtypes == [p, p, i, i, i, i, f, p, p]
    assert L.glass_roi_mask_rings_count.argtypes == [p, p, i, i, i, i, f, p, p, l, p, p, p]
    assert all(getattr(L, n).restype is i for n in NAMES)


def test_every_bad_argument_is_refused_on_the_host():
    """no device needed: every refusal comes before the first runtime call; the pointers are never dereferenced"""
    from glass_amd import _lib
    _lib.build_library()
    L = _lib.lib()
    buf = (ctypes.c_char * 256)()
    a = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16
    ok = dict(R=2, M=28, H=64, W=64, t=0.5)
    for change in (dict(M=0), dict(M=4097), dict(H=0), dict(W=65536), dict(H=65535, W=65535), dict(R=-1), dict(t=0.0), dict(t=-1.0),
                   dict(t=float("nan"))):
        q = {**ok, **change}
        assert L.glass_roi_mask_windows(a, a, q["R"], q["M"], q["H"], q["W"], q["t"], a, None) < 0, change
        assert L.glass_roi_mask_rings_count(a, a, q["R"], q["M"], q["H"], q["W"], q["t"], a, a, 4096, a, a, None) < 0, change
    assert "threshold" in L.glass_last_error().decode()
    assert L.glass_roi_mask_windows(None, a, 2, 28, 64, 64, 0.5, a, None) < 0
    assert L.glass_roi_mask_windows(a, a, 2, 28, 64, 64, 0.5, a + 4, None) < 0               # windows not 16-byte aligned
    assert L.glass_roi_mask_rings_count(a, a, 2, 28, 64, 64, 0.5, a, None, 4096, a, a, None) < 0
    assert L.glass_roi_mask_rings_count(a, a, 2, 28, 64, 64, 0.5, a, a, 8, a, a, None) < 0   # workspace too short for its header
    assert L.glass_roi_mask_rects(a, 2, 0, 64, 64, a, None) < 0
    assert L.glass_roi_mask_windows(None, None, 0, 28, 64, 64, 0.5, None, None) == 0           # R == 0: nothing to do
    assert L.glass_roi_mask_rings_count(None, None, 0, 28, 64, 64, 0.5, None, None, 0, None, None, None) == 0


def test_cpu_tensors_wrong_types_and_thresholds_raise_before_any_launch():
    from glass_amd._lib import GlassLibraryError
    from glass_amd.ops import native as K
    masks, boxes = torch.zeros((2, 28, 28)), torch.zeros((2, 5))
    with mock.patch.object(K, "lib", side_effect=AssertionError("launched")):
        with pytest.raises(GlassLibraryError, match="HIP device"):
            K.roi_mask_rings(masks, boxes, (40, 60))
        for args in ((masks.double(), boxes, (40, 60), 0.5), (masks[:, :, :20], boxes, (40, 60), 0.5), (masks, boxes[:1], (40, 60), 0.5),
                     (masks, boxes, (0, 60), 0.5), (masks, boxes, (40, 60), 0.0), (masks, boxes, (40, 60), -0.5),
                     (masks, boxes, (40, 60), float("nan"))):
            with pytest.raises(GlassLibraryError):
                K._roi_mask_args(*args, "roi_mask_rings")


def test_oracle_paste_sets_no_pixel_outside_the_rectangle():
    """a condition, not a tolerance: on every case the CPU oracle's paste has all of its set pixels inside roi_mask_rects, even
    with no margin at all"""
    from glass_amd.ops import native as K
    from oracle import glass_cpu as O
    nonempty = 0
    for c in RC.cases():
        pasted = O.paste_rotated_masks(torch.from_numpy(c["masks"]), torch.from_numpy(c["boxes"]), c["hw"], c["threshold"]).numpy()
        for margin in (0, K.ROI_MASK_RECT_MARGIN):
            rects = K.roi_mask_rects(c["boxes"], c["M"], c["hw"], margin=margin)
            assert rects.dtype == np.int32 and rects.shape == (len(c["boxes"]), 4)
            assert RC.outside(pasted, rects) == 0, (c["name"], margin)
            live = rects[:, 2] >= rects[:, 0]
            assert (rects[live, 0] >= 0).all() and (rects[live, 1] >= 0).all(), c["name"]
            assert (rects[live, 2] < c["hw"][1]).all() and (rects[live, 3] < c["hw"][0]).all(), c["name"]
        nonempty += int(pasted.any(axis=(1, 2)).sum())
    assert nonempty > 200


def test_the_cases_cover_what_they_claim():
    from glass_amd.ops import native as K
    b = RC.boxes_for(211, 317)
    fin = np.isfinite(b).all(axis=1)
    assert (~fin).sum() == 15 and all(np.isnan(b[:, k]).any() and np.isposinf(b[:, k]).any() and np.isneginf(b[:, k]).any()
                                      for k in range(5))
    assert (b[fin, 2] == 0).any() and (b[fin, 3] == 0).any() and (b[fin, 2] < 0).any()
    assert set(RC.ANGLES) <= set(b[fin, 4].tolist())
    assert b[fin, 2].min() < 0 and np.abs(b[fin, 2:4]).min() == 0 and np.abs(b[fin, 2]).max() > 317
    assert {(c["M"], c["threshold"]) for c in RC.cases()} >= {(28, 0.5), (7, 0.3), (4, 0.9)}
    assert {c["hw"] for c in RC.cases()} == {(211, 317), (37, 53), (640, 704)}
    big = RC.cases()[-1]
    r = K.roi_mask_rects(big["boxes"], 28, big["hw"], margin=0)[0]
    assert (r[3] - r[1] + 1 - 8) * ((r[2] - r[0] + 1 + 63) // 64) > K.MASK_RINGS_LDS_WORDS     # even 8 rows short of the rectangle


def test_non_finite_boxes_give_empty_rectangles():
    from glass_amd.ops import native as K
    ok = [150.0, 100.0, 60.0, 24.0, 15.0]
    rows = [ok]
    for k in range(5):
        for bad in (float("nan"), float("inf"), float("-inf")):
            rows.append(ok[:k] + [bad] + ok[k + 1:])
    rows.append([150.0, 100.0, 60.0, 24.0, 3e38])                      # a huge finite angle is still a box
    r = K.roi_mask_rects(np.asarray(rows, dtype=np.float32), 28, (211, 317))
    # 15 deg on 62.14 x 24.86 (the box times 1 + 1/28): ex = 33.23, ey = 20.05; centres in [116.77, 183.23] x [79.95, 120.05], + 2
    assert r[0].tolist() == [115, 78, 184, 121]
    assert (r[1:16, 2] < r[1:16, 0]).all() and r[1:16].tolist() == [[317, 211, -1, -1]] * 15
    assert r[16, 2] >= r[16, 0]
    far = K.roi_mask_rects(np.asarray([[1e30, 0, 10, 10, 0], [-1e30, 5, 10, 10, 0], [5, 5, 1e30, 1e30, 45]], dtype=np.float32), 28, (50, 70))
    assert far[:2].tolist() == [[70, 50, -1, -1]] * 2 and far[2].tolist() == [0, 0, 69, 49]
    assert K.roi_mask_rects(np.zeros((0, 5), np.float32), 28, (5, 5)).shape == (0, 4)


def _instances(n):
    from glass_amd.config import get_glass_cfg
    from glass_amd.modeling.recognition.text_encoder import TextEncoder
    from glass_amd.structures.core import Instances, RotatedBoxes
    cfg = get_glass_cfg()
    cfg.MODEL.ROI_RECOGNIZER_HEAD.NAME = "RecognizerRCNNHeadV3"
    cfg.MODEL.ROI_RECOGNIZER_HEAD.MAX_WORD_LENGTH = 25
    enc = TextEncoder(cfg)
    inst = Instances((480, 640))
    b = torch.tensor([[20.0 + 5 * i, 20, 10, 6, 0] for i in range(n)])
    inst.pred_boxes, inst.pred_rboxes = RotatedBoxes(b.clone()), RotatedBoxes(b.clone())
    inst.scores = torch.full((n,), 0.9)
    inst.pred_classes = torch.zeros(n, dtype=torch.int64)
    labels = enc.encode(["word"] * n)[:, 1:]                           # text probabilities that decode to "word"
    inst.pred_text_prob = torch.full((n, labels.shape[1], len(enc.character)), 0.001).scatter_(2, labels.unsqueeze(-1), 0.9)
    inst.pred_mask_rois = torch.full((n, 28, 28), 0.9)
    inst.pred_mask_boxes = torch.tensor([[20.0 + 5 * i, 20, 10, 6, 0] for i in range(n)])
    return enc, inst


def test_instances_to_coco_json_calls_from_rois_only_on_a_callback_that_has_it():
    from glass_amd.evaluation import instances_to_coco_json, masks_to_polygons
    from glass_amd.ops import native as K
    enc, inst = _instances(3)
    square = [[1.0, 1.0], [3.0, 1.0], [3.0, 2.0], [1.0, 2.0], [1.0, 1.0]]
    seen = []

    class WithRois:
        takes_device_tensor = True

        def __call__(self, m):
            raise AssertionError("the pasted masks were asked for")

        def from_rois(self, masks, boxes, image_hw, threshold=0.5):
            seen.append(("from_rois", masks, boxes, tuple(image_hw)))
            return [square] * len(masks)

    class Device:
        takes_device_tensor = True

        def __call__(self, m):
            seen.append(("device", m))
            return masks_to_polygons(m.numpy())

    def host(m):
        seen.append(("host", m))
        return masks_to_polygons(m)

    pasted = torch.zeros((3, 480, 640), dtype=torch.bool)
    pasted[:, 1:2, 1:3] = True

    def paste(masks, boxes, image_hw, threshold=0.5):
        seen.append(("paste", masks, boxes, tuple(image_hw), threshold))
        return pasted

    with mock.patch.object(K, "paste_rotated_masks", side_effect=paste):
        a = instances_to_coco_json(inst, "x.jpg", enc, masks_to_polygons=WithRois())
        assert [s[0] for s in seen] == ["from_rois"]
        assert seen[0][1] is inst.pred_mask_rois and seen[0][2] is inst.pred_mask_boxes and seen[0][3] == (480, 640)
        del seen[:]
        b = instances_to_coco_json(inst, "x.jpg", enc, masks_to_polygons=Device())
        assert [s[0] for s in seen] == ["paste", "device"] and seen[1][1] is pasted and seen[0][3:] == ((480, 640), 0.5)
        assert torch.equal(seen[0][1], inst.pred_mask_rois) and torch.equal(seen[0][2], inst.pred_mask_boxes)
        del seen[:]
        c = instances_to_coco_json(inst, "x.jpg", enc, masks_to_polygons=host)
        assert [s[0] for s in seen] == ["paste", "host"] and isinstance(seen[1][1], np.ndarray) and seen[1][1].dtype == bool
        del seen[:]
        d = instances_to_coco_json(inst, "x.jpg", enc)                 # no callback: the box polygon, nothing pasted
        assert seen == [] and len(d) == 3 and len(d[0]["polys"]) == 4
    assert a == b == c and len(a) == 3 and a[0]["polys"] == square


def test_cfg_key_exists_and_defaults_to_true():
    from glass_amd.config import get_glass_cfg
    cfg = get_glass_cfg()
    assert cfg.MODEL.ROI_MASK_HEAD.PASTE_MASKS is True and cfg.MODEL.ROI_MASK_HEAD.MASK_INFERENCE is False
    yaml = os.path.join(ROOT, "configs", "glass_icdar15_mi355x.yaml")
    cfg = get_glass_cfg(yaml, ["MODEL.DEVICE", "cpu", "MODEL.ROI_MASK_HEAD.PASTE_MASKS", False])
    assert cfg.MODEL.ROI_MASK_HEAD.PASTE_MASKS is False
    import glass_amd
    assert glass_amd.build_model(cfg).paste_masks is False                                  # the model reads it
    assert glass_amd.build_model(get_glass_cfg(yaml, ["MODEL.DEVICE", "cpu"])).paste_masks is True


def test_detector_postprocess_carries_the_rois_and_a_copy_of_the_boxes():
    from glass_amd.postprocess.post_processor_academic import detector_postprocess
    from glass_amd.structures.core import Instances, RotatedBoxes
    inst = Instances((100, 200))
    inst.pred_boxes = RotatedBoxes(torch.tensor([[50.0, 40, 30, 10, 20], [120.0, 60, 0, 10, 0], [90.0, 30, 44, 12, -45]]))
    inst.scores = torch.ones(3)
    inst.pred_masks = torch.rand((3, 1, 28, 28), generator=torch.Generator().manual_seed(1))
    want = inst.pred_masks[[0, 2], 0].clone()
    out = detector_postprocess(inst, 150, 300, paste_masks=False)
    assert not out.has("pred_masks") and len(out) == 2                 # the empty box is dropped, its mask row with it
    assert torch.equal(out.pred_mask_rois, want) and out.pred_mask_rois.dtype == torch.float32
    assert torch.equal(out.pred_mask_boxes, out.pred_boxes.tensor) and out.pred_mask_boxes is not out.pred_boxes.tensor
    out.pred_boxes.tensor[:, 2] += 5                                   # what the merge step does later
    assert float(out.pred_mask_boxes[0, 2]) != float(out.pred_boxes.tensor[0, 2])
    assert len(out[torch.tensor([1])].pred_mask_rois) == 1             # the fields index like any other row


def test_run_tiled_refusal_names_the_key():
    from glass_amd.inference.glass_runner import GlassRunner
    model = types.SimpleNamespace(roi_heads=types.SimpleNamespace(mask_inference=True), paste_masks=True)
    with pytest.raises(NotImplementedError, match=r"MODEL\.ROI_MASK_HEAD\.PASTE_MASKS False") as e:
        GlassRunner.run_tiled(types.SimpleNamespace(model=model), np.zeros((8, 8, 3), np.uint8))
    assert "MASK_INFERENCE" in str(e.value)
