"""Host side of the test-time resize (glass_amd/data): the numpy statement of PIL's bilinear resize against PIL itself and
against the committed golden, the ResizeShortestEdge size rule, and the inference DatasetMapper on the host."""
import os

import numpy as np
import pytest
import torch

import resize_pil_cases as C
from glass_amd.data import DatasetMapper, ResizeShortestEdge, pil_bilinear_coeffs, pil_resize_u8_host


@pytest.mark.parametrize("name", list(C.CASES) + ["protocol"])
def test_host_equals_pil(name):
    pytest.importorskip("PIL")
    case = C.PROTOCOL if name == "protocol" else C.CASES[name]
    img = C.make_input(case)
    got = pil_resize_u8_host(img, case[1])
    assert got.dtype == np.uint8 and got.shape == tuple(case[1]) + (3,)
    assert np.array_equal(got, C.pil_resize(img, case[1]))


def test_host_equals_golden():
    with np.load(C.GOLDEN) as g:
        assert sorted(g.files) == sorted(C.GOLDEN_CASES)
        for name in C.GOLDEN_CASES:
            got = pil_resize_u8_host(C.make_input(name), C.CASES[name][1])
            assert np.array_equal(got, g[name]), name
    assert os.path.getsize(C.GOLDEN) < 64 * 1024


def test_golden_is_what_pil_gives():
    pytest.importorskip("PIL")
    with np.load(C.GOLDEN) as g:
        for name in C.GOLDEN_CASES:
            assert np.array_equal(g[name], C.pil_resize(C.make_input(name), C.CASES[name][1])), name


def test_coefficient_tables():
    k, b = pil_bilinear_coeffs(603, 31)
    assert k.dtype == np.int32 and b.dtype == np.int32 and k.shape == (31, 41) and b.shape == (31, 2)
    assert pil_bilinear_coeffs(401, 40)[0].shape == (40, 23)
    for n_in, n_out in ((5, 9), (603, 31), (1, 4), (9, 2), (1280, 1778)):
        k, b = pil_bilinear_coeffs(n_in, n_out)
        assert (b[:, 0] >= 0).all() and (b[:, 1] >= 1).all() and (b[:, 0] + b[:, 1] <= n_in).all() and (b[:, 1] <= k.shape[1]).all()
        assert (k >= 0).all() and (k[np.arange(k.shape[1])[None, :] >= b[:, 1:2]] == 0).all()
        # rows sum to 2^22 up to half a unit of rounding per tap: 255 * sum + 2^21 stays below 2^31
        assert (np.abs(k.sum(1, dtype=np.int64) - (1 << 22)) <= b[:, 1] // 2 + 1).all()
    k, b = pil_bilinear_coeffs(5, 9)                       # upscale: 3 slots, 1 or 2 taps used
    assert k.shape[1] == 3 and set(b[:, 1].tolist()) <= {1, 2}


@pytest.mark.parametrize("hw, short, max_size, want", [
    ((720, 1280), 1000, 1000000, (1000, 1778)),
    ((500, 2000), 1000, 1600, (400, 1600)),
    ((50, 50), 100, 1000, (100, 100)),                     # square
    ((300, 200), 100, 1000, (150, 100)),                   # h > w
    ((2, 3), 5, 100, (5, 8)),                              # 2.5 * 3 = 7.5 rounds up
    ((333, 500), 800, 1333, (800, 1201)),
    ((5, 7), 0, 10, (5, 7)),                               # size 0: no resize
])
def test_output_shape(hw, short, max_size, want):
    assert ResizeShortestEdge(short, max_size).get_output_shape(*hw) == want


def _cfg(fmt, short=40, max_size=1000):
    from glass_amd.config import get_glass_cfg
    return get_glass_cfg(None, ["INPUT.FORMAT", fmt, "INPUT.MIN_SIZE_TEST", short, "INPUT.MAX_SIZE_TEST", max_size,
                                "MODEL.DEVICE", "cpu"])


def _grey(img):
    g = np.uint8(0.2125 * img[:, :, 0] + 0.7154 * img[:, :, 1] + 0.0721 * img[:, :, 2])
    return np.repeat(g[:, :, None], 3, axis=2)


@pytest.mark.parametrize("fmt", ["BGR", "GREY"])
@pytest.mark.parametrize("fused", [False, True])
def test_mapper(fmt, fused):
    pytest.importorskip("PIL")
    img = C.make_input(((30, 52), None, None))
    dd = {"file_name": "img_7.jpg", "image": img, "height": 30, "width": 52, "image_id": 7,
          "annotations": [{"bbox": [1, 2, 3, 4, 0], "text": "a"}]}
    out = DatasetMapper(_cfg(fmt), is_train=False, device="cpu", fused=fused)(dd)
    assert "annotations" in dd and "annotations" not in out             # dropped from the copy only
    assert (out["file_name"], out["height"], out["width"], out["image_id"]) == ("img_7.jpg", 30, 52, 7)
    src = _grey(img) if fmt == "GREY" else img                           # GREY on the host image, before the resize
    want_hw = (40, 69)                                                   # 40 / 30 * 52 = 69.33
    want = C.pil_resize(src, want_hw)
    if fused:
        assert set(out) == {"file_name", "height", "width", "image_id", "image_u8", "resize"}
        assert tuple(out["resize"]) == want_hw
        assert out["image_u8"].dtype == torch.uint8 and np.array_equal(out["image_u8"].numpy(), src)
        assert np.array_equal(pil_resize_u8_host(out["image_u8"].numpy(), out["resize"]), want)
    else:
        assert set(out) == {"file_name", "height", "width", "image_id", "image"}
        assert out["image"].dtype == torch.uint8 and tuple(out["image"].shape) == (3,) + want_hw
        assert np.array_equal(out["image"].permute(1, 2, 0).numpy(), want)


def test_mapper_reads_files(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    img = C.make_input(((20, 24), None, None))
    path = str(tmp_path / "a.png")
    Image.fromarray(img).save(path)
    for fmt, want in (("RGB", img), ("BGR", img[:, :, ::-1]), ("GREY", _grey(img))):
        out = DatasetMapper(_cfg(fmt, short=0), device="cpu", fused=True)({"file_name": path})
        assert np.array_equal(out["image_u8"].numpy(), want) and out["resize"] == (20, 24)
        assert (out["height"], out["width"], out["file_name"]) == (20, 24, path)


def test_mapper_refuses_training_and_wrong_sizes():
    with pytest.raises(NotImplementedError):
        DatasetMapper(_cfg("BGR"), is_train=True)
    with pytest.raises(ValueError):
        DatasetMapper(_cfg("BGR"), device="cpu")({"image": C.make_input(((8, 9), None, None)), "height": 9, "width": 9})
