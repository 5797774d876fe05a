"""CPU: the host side of the device mask polygoniser (exports, MaskPolygonizer's place in glass_amd.evaluation, how
instances_to_coco_json hands the masks to a callback) and the independent ring checker of tests/mask_ring_cases.py
against the host tracer."""
import os
import re

import numpy as np
import pytest
import torch

import mask_ring_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("glass_mask_windows", "glass_mask_rings_workspace_bytes", "glass_mask_rings_count", "glass_mask_rings_write")


def test_new_symbols_exported_declared_and_abi_unchanged():
    from glass_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "glass_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(glass_[a-z0-9_]+)\s*\(", hdr))
    for name in NAMES:
        assert name in _lib.EXPORTS and name in declared, name
    assert _lib.ABI_VERSION == 8
    from glass_amd.ops import native as K
    assert int(re.search(r"#define GLASS_MASK_RINGS_LDS_WORDS (\d+)", hdr).group(1)) == K.MASK_RINGS_LDS_WORDS


def test_workspace_is_sized_from_the_windows_not_from_the_tensor():
    """host function of the library (no GPU): 8 bytes per window pixel; empty and out-of-image windows count nothing"""
    import ctypes
    from glass_amd import _lib
    _lib.build_library()
    L = _lib.lib()
    win = np.array([[10, 20, 109, 59], [1600, 1600, -1, -1], [0, 0, 1599, 1599], [5, 5, 1600, 9]], dtype=np.int32)
    ptr = ctypes.c_void_p(win.ctypes.data)
    fixed = L.glass_mask_rings_workspace_bytes(ptr, 4, 1600, 1600) - 8 * (100 * 40 + 1600 * 1600)
    assert 0 < fixed <= 4 * 20 + 64
    assert L.glass_mask_rings_workspace_bytes(ptr, 2, 1600, 1600) < 8 * 100 * 40 + 200       # nothing like R * H * W * 4
    assert L.glass_mask_rings_workspace_bytes(ptr, 0, 1600, 1600) == 0


def test_polygonizer_is_exported_next_to_the_host_tracer():
    import glass_amd.evaluation as E
    assert callable(E.masks_to_polygons) and E.MaskPolygonizer.takes_device_tensor is True
    assert not getattr(E.masks_to_polygons, "takes_device_tensor", False)


def test_cpu_tensor_is_refused_before_any_launch():
    from glass_amd._lib import GlassLibraryError
    from glass_amd.ops import native as K
    with pytest.raises(GlassLibraryError):
        K.mask_rings(torch.zeros((2, 4, 4), dtype=torch.bool))


def _instances(masks):
    from test_gpu_rrc_score import _encoder, _instances as make
    enc = _encoder()
    n = len(masks)
    return enc, make(enc, [[20 + 5 * i, 20, 10, 6, 0] for i in range(n)], ["word"] * n, [0.9] * n, masks)


def test_instances_to_coco_json_hands_a_tensor_only_to_a_callback_that_asks_for_it():
    from glass_amd.evaluation import instances_to_coco_json, masks_to_polygons
    masks = np.zeros((3, 40, 60), dtype=bool)
    masks[0, 5:9, 5:20] = masks[1, 10:30, 10:12] = True
    enc, inst = _instances(masks)
    seen = []

    class Device:
        takes_device_tensor = True

        def __call__(self, m):
            seen.append(m)
            return masks_to_polygons(m.cpu().numpy())

    def host(m):
        seen.append(m)
        return masks_to_polygons(m)

    a = instances_to_coco_json(inst, "x.jpg", enc, masks_to_polygons=Device())
    b = instances_to_coco_json(inst, "x.jpg", enc, masks_to_polygons=host)
    assert isinstance(seen[0], torch.Tensor) and seen[0] is inst.pred_masks
    assert isinstance(seen[1], np.ndarray) and seen[1].dtype == bool
    assert a == b and len(a) == 2 and a[0]["polys"] == [[5.0, 5.0], [20.0, 5.0], [20.0, 9.0], [5.0, 9.0], [5.0, 5.0]]
    c = instances_to_coco_json(inst, "x.jpg", enc)                                         # no callback: the box polygon, as before
    assert len(c) == 3 and len(c[0]["polys"]) == 4


def test_checker_accepts_the_host_tracer_on_the_seeded_cases():
    from glass_amd.evaluation import masks_to_polygons
    n = 0
    for name, m in C.hand_made() + [("serpentine", C.serpentine(21, 30)), ("comb", C.comb(16, 41))]:
        C.check_ring(m, masks_to_polygons([m])[0])
        n += 1
    for name, masks in C.noise_batches():
        for m, ring in zip(masks[:12], masks_to_polygons(masks[:12])):
            C.check_ring(m, ring)
            n += 1
    assert n >= 200
    rect = C.hand_made()[0][1]
    ring = masks_to_polygons([rect])[0]
    x, y = np.array(ring).T
    assert int((x[:-1] * y[1:] - x[1:] * y[:-1]).sum()) == 24                              # the rectangle of the known-answer test


def test_checker_rejects_wrong_rings():
    from glass_amd.evaluation import masks_to_polygons
    shapes = dict(C.hand_made())
    m = shapes["L"]
    good = masks_to_polygons([m])[0]
    C.check_ring(m, good)
    moved = [list(p) for p in good]
    moved[2][0] += 1                                                                      # one vertex moved
    wider = [[1.0, 1.0], [4.0, 1.0], [4.0, 3.0], [5.0, 3.0], [5.0, 5.0], [1.0, 5.0], [1.0, 1.0]]   # rectilinear, one pixel too many
    hull = [[1.0, 1.0], [5.0, 1.0], [5.0, 5.0], [1.0, 5.0], [1.0, 1.0]]
    rotated = good[1:-1] + good[:2]                                                        # right geometry, wrong start
    extra = good[:1] + [[2.0, 1.0]] + good[1:]                                            # a vertex where nothing turns
    for bad in (moved, wider, hull, good[::-1], good[:-1], rotated, extra, []):
        with pytest.raises(AssertionError):
            C.check_ring(m, bad)
    with pytest.raises(AssertionError):
        C.check_ring(shapes["empty"], good)
    two = shapes["equal sizes"]                                                            # the other region of a tie is refused
    other = np.zeros_like(two); other[4:6, 1:4] = True
    with pytest.raises(AssertionError):
        C.check_ring(two, masks_to_polygons([other])[0])
    holed = shapes["holed square"]                                                         # the hole's ring is not the exterior
    with pytest.raises(AssertionError):
        C.check_ring(holed, [[2.0, 2.0], [3.0, 2.0], [3.0, 3.0], [2.0, 3.0], [2.0, 2.0]])
