"""Host side of the rotated-image evaluation (glass_amd/data/transforms.py, glass_amd/evaluation/rotated.py): the numpy
statement of PIL.Image.rotate(BILINEAR, expand=True) against Pillow itself and against the committed golden, the output size,
the maps of points, rotated boxes and ground truth, and the inference DatasetMapper on the host."""
import math
import os
import re

import numpy as np
import pytest
import torch

import rotate_cases as C
from glass_amd.data import DatasetMapper, RotationTransform, pil_resize_u8_host, rotate_u8_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_equals_pillow_on_every_case():
    pytest.importorskip("PIL")
    cases = C.all_cases()
    for name, img, angle, fill in cases:
        got, want = rotate_u8_host(img, angle, fill), C.pil_rotate(img, angle, fill)
        assert got.dtype == np.uint8 and got.shape == want.shape, name
        assert np.array_equal(got, want), name
    assert len(cases) > 200


def test_host_equals_golden():
    with np.load(C.GOLDEN) as g:
        assert sorted(g.files) == sorted(C.golden_name(*c) for c in C.GOLDEN_CASES)
        for h, w, a, f in C.GOLDEN_CASES:
            assert np.array_equal(rotate_u8_host(C.make_image(h, w), a, C.FILLS[f]), g[C.golden_name(h, w, a, f)]), (h, w, a, f)
    assert os.path.getsize(C.GOLDEN) < 64 * 1024


def test_golden_is_what_pillow_gives():
    pytest.importorskip("PIL")
    with np.load(C.GOLDEN) as g:
        for h, w, a, f in C.GOLDEN_CASES:
            assert np.array_equal(g[C.golden_name(h, w, a, f)], C.pil_rotate(C.make_image(h, w), a, C.FILLS[f])), (h, w, a, f)


def test_the_four_transposes():
    for h, w in C.SIZES:
        img = C.make_image(h, w)
        for angle, kind in ((0, 0), (360, 0), (-360, 0), (90, 1), (-270, 1), (180, 2), (-180, 2), (270, 3), (-90, 3), (450, 1)):
            t = RotationTransform(h, w, angle)
            assert t.kind == kind and t.out_hw == ((h, w) if kind in (0, 2) else (w, h))
            got = rotate_u8_host(img, angle, (9, 9, 9))
            assert np.array_equal(got, np.rot90(img, kind)) and got.flags.c_contiguous
            # the exact point maps: a pixel centre goes where np.rot90 puts the pixel
            ys, xs = np.mgrid[0:h, 0:w]
            q = t.apply_coords(np.stack([xs + 0.5, ys + 0.5], -1))
            qi = (q - 0.5).astype(np.int64)
            assert np.array_equal(q - 0.5, qi) and np.array_equal(got[qi[..., 1], qi[..., 0]], img)
            assert np.array_equal(t.inverse_coords(q), np.stack([xs + 0.5, ys + 0.5], -1))
        assert RotationTransform(h, w, 89.999).kind == 4 and RotationTransform(h, w, 1e-3).kind == 4
    assert rotate_u8_host(img, 0) is not img


def test_out_hw_equals_pillow_on_a_seeded_grid():
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(20261021)
    for i in range(200):
        h, w = int(rng.integers(1, 80)), int(rng.integers(1, 80))
        angle = float(rng.choice([rng.uniform(-400, 400), float(rng.integers(-8, 9)) * 45.0, rng.uniform(-1e-3, 1e-3), 90 + rng.uniform(-1e-6, 1e-6)]))
        wo, ho = Image.new("RGB", (w, h)).rotate(angle, expand=True).size
        assert RotationTransform(h, w, angle).out_hw == (ho, wo), (h, w, angle)


def test_a_lit_pixel_lands_where_the_point_map_says():
    """A single lit pixel: the intensity centroid of its rotated splat against apply_coords of its centre.  Derived bound: a
    bilinear splat spans at most one pixel either side of the mapped centre, so the centroid is within 1.0 px of it (the inside
    rule clips the splat at the corners, which moves the centroid by less than that).  Largest distance observed: 0.535 px."""
    worst = 0.0
    for h, w in ((40, 64), (33, 17)):
        for px, py in ((0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1), (w // 2, h // 2), (3, h - 5), (w - 4, 7)):
            img = np.zeros((h, w, 3), dtype=np.uint8)
            img[py, px] = 255
            for angle in (15, 30, 45, 60, 75, -170, 33.3):
                t = RotationTransform(h, w, angle)
                out = rotate_u8_host(img, t)[:, :, 0].astype(np.float64)
                assert out.sum() > 0, (h, w, px, py, angle)
                ys, xs = np.mgrid[0:out.shape[0], 0:out.shape[1]]
                cx, cy = (out * (xs + 0.5)).sum() / out.sum(), (out * (ys + 0.5)).sum() / out.sum()
                qx, qy = t.apply_coords([px + 0.5, py + 0.5])
                worst = max(worst, math.hypot(cx - qx, cy - qy))
    print(f"[rotate] lit pixel: largest |centroid - mapped centre| {worst:.3f} px")
    assert worst <= 1.0


def test_point_maps_are_inverse():
    rng = np.random.default_rng(5)
    p = rng.uniform(-8192, 8192, size=(4096, 2))
    worst = 0.0
    for h, w in ((720, 1280), (33, 17), (1, 9)):
        for angle in C.ANGLES + [60 - 1e-9, 1234.5]:
            t = RotationTransform(h, w, angle)
            worst = max(worst, float(np.abs(t.inverse_coords(t.apply_coords(p)) - p).max()),
                        float(np.abs(t.apply_coords(t.inverse_coords(p)) - p).max()))
    print(f"[rotate] inverse(apply(p)) - p: at most {worst:.3e} px")
    assert worst <= 1e-9
    t = RotationTransform(40, 64, 30)                                   # the image's centre goes to the canvas's centre
    assert np.abs(t.apply_coords([32.0, 20.0]) - [t.out_hw[1] / 2, t.out_hw[0] / 2]).max() < 1e-9
    with pytest.raises(ValueError):
        t.apply_coords(np.zeros((3, 3)))


def _corners(b):
    """float64 corners [n, 4, 2] of boxes (cx, cy, w, h, a): width along u = (cos, -sin), height along v = (sin, cos)"""
    b = np.asarray(b, dtype=np.float64)
    th = np.radians(b[:, 4])
    u = np.stack([np.cos(th), -np.sin(th)], -1) * b[:, 2:3] / 2
    v = np.stack([np.sin(th), np.cos(th)], -1) * b[:, 3:4] / 2
    c = b[:, :2]
    return np.stack([c - u - v, c + u - v, c + u + v, c - u + v], 1)


def test_rotated_boxes_follow_their_corners():
    rng = np.random.default_rng(11)
    n = 500
    b = np.stack([rng.uniform(0, 1280, n), rng.uniform(0, 720, n), rng.uniform(1, 300, n), rng.uniform(1, 80, n), rng.uniform(-180, 180, n)], 1)
    worst = back = 0.0
    for angle in C.ANGLES + [60 + 1e-9, 725.0]:
        t = RotationTransform(720, 1280, angle)
        fwd = t.apply_rotated_boxes(b)                                   # float64 in, float64 out: the map without the rounding
        assert fwd.dtype == np.float64 and (fwd[:, 4] >= -180).all() and (fwd[:, 4] < 180).all()
        assert np.array_equal(fwd[:, 2:4], b[:, 2:4])
        worst = max(worst, float(np.abs(_corners(fwd) - t.apply_coords(_corners(b))).max()))
        back = max(back, float(np.abs(t.inverse_rotated_boxes(fwd) - b).max()))
    print(f"[rotate] boxes: corners off by at most {worst:.3e} px, inverse(apply(b)) - b at most {back:.3e}")
    assert worst <= 1e-9 and back <= 1e-9
    t = RotationTransform(100, 200, 30)
    assert t.apply_rotated_boxes(np.array([[5, 5, 2, 1, 170.0]]))[0, 4] == -160.0 and t.inverse_rotated_boxes(np.array([[5, 5, 2, 1, -170.0]]))[0, 4] == 160.0
    assert t.apply_rotated_boxes(np.array([[5, 5, 2, 1, 150.0]]))[0, 4] == -180.0
    f32 = np.array([[10, 20, 30, 5, 45], [np.nan, 1, 2, 3, 4], [1, np.inf, 2, 3, 4], [1, 2, 3, 4, -np.inf], [7, 8, 9, 10, 11]], dtype=np.float32)
    f32[1, 0] = np.array([0x7FC01234], dtype=np.uint32).view(np.float32)[0]       # a NaN with a payload
    for got in (t.apply_rotated_boxes(f32), t.inverse_rotated_boxes(f32)):
        assert got.dtype == np.float32 and np.array_equal(got[1:4].view(np.uint32), f32[1:4].view(np.uint32))
        assert np.isfinite(got[[0, 4]]).all() and not np.array_equal(got[0], f32[0])
    want = t.apply_rotated_boxes(f32.astype(np.float64)[[0, 4]]).astype(np.float32)    # float32 rows: float64, rounded once
    assert np.array_equal(t.apply_rotated_boxes(f32)[[0, 4]], want)
    assert t.apply_rotated_boxes(np.zeros((0, 5), dtype=np.float32)).shape == (0, 5)


def _area2(ring):
    x, y = np.array(ring[0::2], dtype=np.int64), np.array(ring[1::2], dtype=np.int64)
    return int((x * np.roll(y, -1) - np.roll(x, -1) * y).sum())


def test_rotate_ground_truth_on_hand_cases():
    from glass_amd.evaluation import rotate_ground_truth
    quad = [10, 20, 50, 20, 50, 30, 10, 30]
    gt = {"1": ([quad], ["word"]), "2": ([], [])}
    sizes = {"1": (100, 200), "2": (7, 5)}                              # h x w
    # 90 degrees counter-clockwise on a 100 x 200 image: (x, y) -> (y, 200 - x); 180 degrees: (x, y) -> (200 - x, 100 - y)
    r90 = rotate_ground_truth(gt, sizes, 90)
    assert r90["1"] == ([[20, 190, 20, 150, 30, 150, 30, 190]], ["word"]) and r90["2"] == ([], [])
    assert rotate_ground_truth(gt, sizes, 180)["1"][0] == [[190, 80, 150, 80, 150, 70, 190, 70]]
    assert rotate_ground_truth(gt, sizes, 0)["1"][0] == [quad] and rotate_ground_truth(gt, sizes, 360)["1"][0] == [quad]
    assert list(r90) == ["1", "2"] and all(type(v) is int for v in r90["1"][0][0])
    assert gt["1"][0][0] == quad                                         # the input is left alone
    ring12 = [int(round(300 + 100 * math.cos(2 * math.pi * k / 12))) if i == 0 else int(round(200 + 60 * math.sin(2 * math.pi * k / 12)))
              for k in range(12) for i in (0, 1)]
    for angle in (30, 45, 60, -170, 33.3):
        t = RotationTransform(480, 640, angle)
        got = rotate_ground_truth({"7": ([ring12], ["x"])}, {"7": (480, 640)}, angle)["7"][0][0]
        q = t.apply_coords(np.array(ring12, dtype=np.float64).reshape(12, 2))
        assert len(got) == 24 and np.abs(np.array(got).reshape(12, 2) - q).max() <= 0.5       # vertex k stays vertex k
        assert np.array_equal(np.array(got).reshape(12, 2), np.floor(q + 0.5).astype(np.int64))
        assert _area2(got) * _area2(ring12) > 0                          # the orientation's sign
        assert abs(abs(_area2(got)) - abs(_area2(ring12))) < 0.02 * abs(_area2(ring12))
    with pytest.raises(KeyError, match="'2'"):
        rotate_ground_truth(gt, {"1": (100, 200)}, 30)
    with pytest.raises(ValueError, match="2\\^20"):
        rotate_ground_truth({"1": ([[0, 0, 3000000, 0, 3000000, 5, 0, 5]], ["far"])}, sizes, 30)


def _cfg(fmt, short=40, max_size=1000):
    from glass_amd.config import get_glass_cfg
    return get_glass_cfg(None, ["INPUT.FORMAT", fmt, "INPUT.MIN_SIZE_TEST", short, "INPUT.MAX_SIZE_TEST", max_size,
                                "MODEL.DEVICE", "cpu"])


def _grey(img):
    g = np.uint8(0.2125 * img[:, :, 0] + 0.7154 * img[:, :, 1] + 0.0721 * img[:, :, 2])
    return np.repeat(g[:, :, None], 3, axis=2)


@pytest.mark.parametrize("fmt", ["BGR", "GREY"])
@pytest.mark.parametrize("fused", [False, True])
def test_mapper_on_the_host(fmt, fused):
    img = C.make_image(30, 52)
    dd = {"file_name": "img_7.jpg", "image": img, "height": 30, "width": 52, "image_id": 7, "annotations": [{"bbox": [1, 2, 3, 4, 0]}]}
    plain = DatasetMapper(_cfg(fmt), device="cpu", fused=fused)(dd)
    zero = DatasetMapper(_cfg(fmt), device="cpu", fused=fused, rotate=0.0, rotate_fill=(1, 2, 3))(dd)
    assert list(plain) == list(zero) and "rotation" not in zero          # rotate=0: today's dict, key for key
    for k in plain:
        assert torch.equal(plain[k], zero[k]) if isinstance(plain[k], torch.Tensor) else plain[k] == zero[k], k
    mapper = DatasetMapper(_cfg(fmt), device="cpu", fused=fused, rotate=30, rotate_fill=(7, 200, 255))
    out = mapper(dd)
    src = _grey(img) if fmt == "GREY" else img                           # GREY first, then the rotation, then the resize
    rot = rotate_u8_host(src, 30, (7, 200, 255))
    t = out["rotation"]
    assert isinstance(t, RotationTransform) and (t.h, t.w, t.angle, t.out_hw) == (30, 52, 30.0, rot.shape[:2])
    assert (out["height"], out["width"]) == rot.shape[:2] == (52, 62)    # the rotated image's (what Pillow's expand gives); the size check was on 30 x 52
    assert (out["file_name"], out["image_id"]) == ("img_7.jpg", 7) and "annotations" not in out
    want_hw = mapper.resize.get_output_shape(*rot.shape[:2])
    if fused:
        assert set(out) == {"file_name", "height", "width", "image_id", "image_u8", "resize", "rotation"}
        assert tuple(out["resize"]) == want_hw and np.array_equal(out["image_u8"].numpy(), rot)
    else:
        assert set(out) == {"file_name", "height", "width", "image_id", "image", "rotation"}
        assert np.array_equal(out["image"].permute(1, 2, 0).numpy(), pil_resize_u8_host(rot, want_hw))
    mapper.rotate = 0.0                                                  # the attribute may be set between calls
    assert "rotation" not in mapper(dd)


def test_mapper_constructor_refuses_bad_arguments():
    for bad in (float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError, match="rotate"):
            DatasetMapper(_cfg("BGR"), device="cpu", rotate=bad)
    for bad in ((0, 0), (0, 0, 256), (-1, 0, 0), (0.5, 0, 0), "abc", 7, (0, 0, float("nan"))):
        with pytest.raises(ValueError, match="fill"):
            DatasetMapper(_cfg("BGR"), device="cpu", rotate=30, rotate_fill=bad)
    with pytest.raises(ValueError):                                      # the size check is made on the unrotated image
        DatasetMapper(_cfg("BGR"), device="cpu", rotate=90)({"image": C.make_image(8, 9), "height": 9, "width": 8})
    with pytest.raises(ValueError):
        rotate_u8_host(C.make_image(8, 9), float("nan"))
    with pytest.raises(ValueError):
        rotate_u8_host(C.make_image(8, 9), RotationTransform(9, 8, 30))


def test_the_contraction_case_is_one():
    """tests/rotate_cases.py::search_fma_case found it: on this image a fused multiply-add changes a byte, so the device test
    that includes it fails for a kernel compiled with contraction"""
    c = C.FMA_CASE
    img = C.make_image(*c["hw"], c["kind"])
    t = RotationTransform(*c["hw"], c["angle"])
    x, y, ch = c["pixel"]
    assert int(rotate_u8_host(img, t, c["fill"])[y, x, ch]) == c["statement"]
    assert C.contracted_pixel(img, t.matrix, x, y, c["fill"])[ch] == c["contracted"] != c["statement"]
    assert any(name == "fma_case" for name, *_ in C.all_cases())


def test_header_declares_the_two_entry_points():
    from glass_amd import _lib
    with open(os.path.join(ROOT, "include", "glass_hip_feature_rotate.h")) as fh:
        text = fh.read()
    sigs = _lib.signatures(text)
    assert list(sigs) == ["glass_rotate_u8", "glass_rotate_boxes"]
    assert set(sigs) <= set(_lib.FEATURE_EXPORTS)
    assert len(sigs["glass_rotate_u8"][1]) == 12 and len(sigs["glass_rotate_boxes"][1]) == 6
    assert re.search(r"fp contract\(off\)", open(os.path.join(ROOT, "glass-text-spotting_amd", "csrc", "image_rotate.hip")).read())
