"""Device side of the rotated-image evaluation: glass_rotate_u8 (csrc/image_rotate.hip) against the numpy statement byte for
byte, guards, determinism and argument checks; glass_rotate_boxes against its statement; the mapper with rotate on the device;
GlassRunner.run_rotated against the same steps done by hand; the scorer's view of rotated ground truth against rotated boxes;
and rotation_sweep on a stub model."""
import ctypes
import functools
import os
from collections import OrderedDict
from fractions import Fraction

import numpy as np
import pytest
import torch

import rotate_cases as C
import rrc_cases as RC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
YAML = os.path.join(ROOT, "configs", "glass_icdar15_mi355x.yaml")
EINVAL = -1


def _dev_u8(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---------------------------------------------------------------------------------------------------- glass_rotate_u8
def test_rotate_equals_the_host_statement_on_every_case():
    from glass_amd.data import rotate_u8_host
    from glass_amd.ops import native as K
    cases = C.all_cases()
    for name, img, angle, fill in cases:
        got = K.rotate_u8(_dev_u8(img), angle, fill)
        want = rotate_u8_host(img, angle, fill)
        assert got.dtype == torch.uint8 and tuple(got.shape) == want.shape and got.is_contiguous(), name
        assert np.array_equal(got.cpu().numpy(), want), name
    assert any(n == "fma_case" for n, *_ in cases) and len(cases) > 200


def _raw_rotate(src, t, dst_ptr, Ho=None, Wo=None, kind=None, matrix=None, fill=(1, 2, 3), H=None, W=None, src_ptr=None):
    from glass_amd import _lib
    from glass_amd.ops import native as K
    m = (ctypes.c_double * 6)(*(t.matrix if matrix is None else matrix)) if matrix is not False else None
    return _lib.lib().glass_rotate_u8(src.data_ptr() if src_ptr is None else src_ptr, src.shape[0] if H is None else H,
                                      src.shape[1] if W is None else W, dst_ptr, t.out_hw[0] if Ho is None else Ho,
                                      t.out_hw[1] if Wo is None else Wo, m, t.kind if kind is None else kind, *fill, K.stream_handle())


@pytest.mark.parametrize("hw, angle", [((130, 257), 33.3), ((130, 257), 90), ((33, 64), 180), ((7, 5), 359.9), ((1, 9), 75), ((64, 64), 270),
                                       ((100, 37), 0)])
def test_guard_bytes_stay_and_two_runs_agree(hw, angle):
    """dst inside a larger buffer at every alignment modulo 4 (the dword grouping follows the address): the bytes before and
    after it keep their poison, and a second run gives the same bytes"""
    from glass_amd.data import RotationTransform, rotate_u8_host
    img = C.make_image(*hw)
    t = RotationTransform(*hw, angle)
    want = rotate_u8_host(img, t, (1, 2, 3))
    src = _dev_u8(img)
    n, pad = want.size, 64
    for off in (0, 1, 2, 3):
        runs = []
        for _ in range(2):
            buf = torch.full((pad + off + n + pad,), 0xA5, dtype=torch.uint8, device=DEV)
            assert _raw_rotate(src, t, buf.data_ptr() + pad + off) == 0
            host = buf.cpu().numpy()
            assert (host[:pad + off] == 0xA5).all() and (host[pad + off + n:] == 0xA5).all(), (hw, angle, off)
            assert np.array_equal(host[pad + off:pad + off + n].reshape(want.shape), want), (hw, angle, off)
            runs.append(host)
        assert np.array_equal(runs[0], runs[1])


def test_bad_arguments_return_einval_and_empty_sizes_launch_nothing():
    from glass_amd import _lib
    from glass_amd.data import RotationTransform
    from glass_amd.ops import native as K
    img = C.make_image(7, 5)
    src = _dev_u8(img)
    t, t90 = RotationTransform(7, 5, 30), RotationTransform(7, 5, 90)
    buf = torch.full((4096,), 0xA5, dtype=torch.uint8, device=DEV)
    d = buf.data_ptr()
    nan, inf = float("nan"), float("inf")
    bad = [dict(src_ptr=0), dict(dst_ptr=0), dict(matrix=False), dict(kind=5), dict(kind=-1), dict(H=-1), dict(W=-1), dict(Ho=-1), dict(Wo=-1),
           dict(matrix=[nan, 0, 0, 0, 1, 0]), dict(matrix=[1, 0, 0, 0, 1, inf]), dict(matrix=[1, 0, -inf, 0, 1, 0]),
           dict(fill=(256, 0, 0)), dict(fill=(0, -1, 0)), dict(fill=(0, 0, 1000)),
           dict(H=32768, W=32768), dict(Ho=32768, Wo=21846),              # 3 * 2^30 and 3 * 715,849,728 >= 2^31
           dict(t=t90, Ho=7, Wo=5), dict(kind=0, Ho=5, Wo=7), dict(kind=2, Ho=7, Wo=6), dict(kind=3, Ho=7, Wo=5), dict(kind=1, Ho=5, Wo=5)]
    for kw in bad:
        kw = dict(kw)
        tt = kw.pop("t", t)
        dst_ptr = kw.pop("dst_ptr", d)
        assert _raw_rotate(src, tt, dst_ptr, **kw) == EINVAL, kw
        assert len(_lib.lib().glass_last_error()) > 0
    assert _raw_rotate(src, t, d, Ho=32768, Wo=21845, H=0, W=5) == 0     # just below 2^31 bytes passes the size check; empty source
    # empty sizes: accepted, nothing launched (null images are fine then), nothing written
    for kw in (dict(H=0, W=5, kind=4), dict(H=7, W=0, kind=4), dict(Ho=0, Wo=9, kind=4), dict(Ho=9, Wo=0, kind=4),
               dict(H=0, W=5, Ho=0, Wo=5, kind=0), dict(H=0, W=5, Ho=5, Wo=0, kind=1), dict(H=0, W=0, Ho=0, Wo=0, kind=2)):
        assert _raw_rotate(src, t, 0, src_ptr=0, **kw) == 0, kw
        assert _raw_rotate(src, t, d, **kw) == 0, kw
    torch.cuda.synchronize()
    assert (buf == 0xA5).all()                                           # none of the calls above wrote a byte
    # the wrapper's own checks
    with pytest.raises(ValueError, match="fill"):
        K.rotate_u8(src, 30, (0, 0, 256))
    with pytest.raises(ValueError):
        K.rotate_u8(src, nan)
    with pytest.raises(ValueError):
        K.rotate_u8(src, RotationTransform(5, 7, 30))
    with pytest.raises(_lib.GlassLibraryError):
        K.rotate_u8(src.cpu(), 30)
    with pytest.raises(_lib.GlassLibraryError):
        K.rotate_u8(src.float(), 30)


def test_protocol_shape_once():
    """720 x 1280 at 33.3 degrees: nothing new in the arithmetic, the widest indices the protocol uses and many workgroups"""
    from glass_amd.data import rotate_u8_host
    from glass_amd.ops import native as K
    img = C.make_image(720, 1280)
    assert np.array_equal(K.rotate_u8(_dev_u8(img), 33.3, (7, 200, 255)).cpu().numpy(), rotate_u8_host(img, 33.3, (7, 200, 255)))


# ---------------------------------------------------------------------------------------------------- glass_rotate_boxes
def _ulps(a, b):
    """float32 arrays -> the largest distance in units in the last place (monotone integer keys)"""
    def key(v):
        i = np.ascontiguousarray(v, dtype=np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return int(np.abs(key(a) - key(b)).max()) if a.size else 0


def _boxes(n, seed=3):
    rng = np.random.default_rng(seed + n)
    b = np.stack([rng.uniform(-50, 1400, n), rng.uniform(-50, 800, n), rng.uniform(0.5, 400, n), rng.uniform(0.5, 90, n),
                  rng.uniform(-720, 720, n)], 1).astype(np.float32)
    for i, (col, v) in enumerate(((0, np.nan), (1, np.inf), (4, -np.inf), (2, np.nan), (3, np.inf))):
        if 5 * i + 2 < n:
            b[5 * i + 2, col] = v
    return b


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1024])
def test_rotate_boxes_equal_the_host_statement(n):
    from glass_amd import _lib
    from glass_amd.data import RotationTransform
    from glass_amd.ops import native as K
    b = _boxes(n)
    worst = 0
    for angle in (33.3, 90, -170, 180, 1e-3, 359.9, 60):
        t = RotationTransform(720, 1280, angle)
        for inverse in (False, True):
            want = t.inverse_rotated_boxes(b) if inverse else t.apply_rotated_boxes(b)
            got = K.rotate_boxes(torch.from_numpy(b).to(DEV), t, inverse=inverse)
            assert got.dtype == torch.float32 and tuple(got.shape) == (n, 5)
            got = got.cpu().numpy()
            bad = ~np.isfinite(b).all(1)
            assert np.array_equal(got[bad].view(np.uint32), b[bad].view(np.uint32))       # copied bit for bit
            assert np.array_equal(got[:, 2:4].view(np.uint32), b[:, 2:4].view(np.uint32))
            worst = max(worst, _ulps(got[~bad], want[~bad]))
            assert ((got[~bad, 4] >= -180) & (got[~bad, 4] <= 180)).all()
    print(f"[rotate] boxes n={n}: worst float32 ulp against the host statement {worst} (bad rows: {int(bad.sum())})")
    assert worst <= 1
    if n:
        # guards around the output, and two runs agree
        t = RotationTransform(720, 1280, 33.3)
        src = torch.from_numpy(b).to(DEV)
        m = (ctypes.c_double * 6)(*t.inverse_matrix)
        runs = []
        for _ in range(2):
            buf = torch.full((8 + n * 5 + 8,), -7.0, dtype=torch.float32, device=DEV)
            assert _lib.lib().glass_rotate_boxes(src.data_ptr(), n, m, t.angle, buf.data_ptr() + 32, K.stream_handle()) == 0
            host = buf.cpu().numpy()
            assert (host[:8] == -7.0).all() and (host[-8:] == -7.0).all()
            runs.append(host)
        assert np.array_equal(runs[0].view(np.uint32), runs[1].view(np.uint32))
        assert np.array_equal(runs[0][8:-8].reshape(n, 5).view(np.uint32), K.rotate_boxes(src, t).cpu().numpy().view(np.uint32))
        nan = float("nan")
        for args in ((src.data_ptr(), -1, m, 1.0, buf.data_ptr()), (0, n, m, 1.0, buf.data_ptr()), (src.data_ptr(), n, m, 1.0, 0),
                     (src.data_ptr(), n, None, 1.0, buf.data_ptr()), (src.data_ptr(), n, m, nan, buf.data_ptr()),
                     (src.data_ptr(), n, (ctypes.c_double * 6)(1, 0, 0, nan, 1, 0), 1.0, buf.data_ptr())):
            assert _lib.lib().glass_rotate_boxes(*args, K.stream_handle()) == EINVAL
    else:
        assert _lib.lib().glass_rotate_boxes(0, 0, (ctypes.c_double * 6)(1, 0, 0, 0, 1, 0), 0.0, 0, K.stream_handle()) == 0
        with pytest.raises(ValueError):
            K.rotate_boxes(torch.zeros((3, 4), device=DEV), RotationTransform(7, 5, 30))
        with pytest.raises(ValueError):
            K.rotate_boxes(torch.zeros((3, 5), device=DEV), 30)
    assert tuple(K.rotate_boxes(torch.from_numpy(b).to(DEV).reshape(1, n, 5), RotationTransform(720, 1280, 30)).shape) == (1, n, 5)


# ---------------------------------------------------------------------------------------------------- the mapper
@functools.lru_cache(maxsize=None)
def _model():
    import glass_amd
    from glass_amd.config import get_glass_cfg
    from glass_amd.utils.synth import make_state_dict
    cfg = get_glass_cfg(YAML, ["MODEL.DEVICE", DEV, "INPUT.MIN_SIZE_TEST", 128, "INPUT.MAX_SIZE_TEST", 1000, "POST_PROCESSING.TEXT_THRESHOLD", 0.0])
    m = glass_amd.build_model(cfg)
    m.load_state_dict(make_state_dict(1234))
    return cfg, m


def test_mapper_rotates_on_the_device_as_on_the_host():
    from glass_amd.data import DatasetMapper, rotate_u8_host
    from glass_amd.utils.synth import make_image
    cfg, model = _model()
    img = make_image(3, 96, 130).numpy()
    dd = {"file_name": "img_3.jpg", "image": img, "height": 96, "width": 130, "annotations": []}
    kw = dict(rotate=33.3, rotate_fill=(7, 200, 255))
    raw = DatasetMapper(cfg, device=DEV, fused=True, **kw)(dd)
    cooked = DatasetMapper(cfg, device=DEV, fused=False, **kw)(dd)
    host_raw = DatasetMapper(cfg, device="cpu", fused=True, **kw)(dd)
    host_cooked = DatasetMapper(cfg, device="cpu", fused=False, **kw)(dd)
    rot = rotate_u8_host(img, 33.3, (7, 200, 255))
    assert raw["image_u8"].is_cuda and cooked["image"].is_cuda and not host_raw["image_u8"].is_cuda
    assert (raw["height"], raw["width"]) == (cooked["height"], cooked["width"]) == (host_raw["height"], host_raw["width"]) == rot.shape[:2]
    assert raw["rotation"].out_hw == rot.shape[:2] and raw["resize"] == host_raw["resize"]
    assert np.array_equal(raw["image_u8"].cpu().numpy(), rot) and np.array_equal(host_raw["image_u8"].numpy(), rot)
    assert torch.equal(cooked["image"].cpu(), host_cooked["image"])                     # device == host, byte for byte
    a, b = model.preprocess_image([raw]), model.preprocess_image([cooked])              # fused == unfused in the padded batch
    assert a.image_sizes == b.image_sizes and torch.equal(a.nhwc4.view(torch.int32), b.nhwc4.view(torch.int32))
    plain = DatasetMapper(cfg, device=DEV, fused=True)(dd)                              # rotate=0: nothing of the feature
    assert set(plain) == {"file_name", "height", "width", "image_u8", "resize"} and (plain["height"], plain["width"]) == (96, 130)


# ---------------------------------------------------------------------------------------------------- run_rotated
def _runner(extra=()):
    from glass_amd.config import get_glass_cfg
    from glass_amd.inference.glass_runner import GlassRunner
    from glass_amd.utils.synth import make_state_dict
    cfg = get_glass_cfg(YAML, ["INPUT.MIN_SIZE_TEST", 160, "INPUT.MAX_SIZE_TEST", 200, "MODEL.DEVICE", DEV,
                               "POST_PROCESSING.TEXT_THRESHOLD", 0.0, "POST_PROCESSING.DETECT_THRESHOLD", 0.0,
                               "POST_PROCESSING.LOW_CONFIDENCE", 0.0, "POST_PROCESSING.VALID_CONFIDENCE", 0.0] + list(extra))
    return GlassRunner(None, None, cfg=cfg, state_dict=make_state_dict(1234), post_process=True)


def _fields_equal(a, b, skip=()):
    assert len(a) == len(b) and a.image_size == b.image_size
    fa, fb = a.get_fields(), b.get_fields()
    assert sorted(fa) == sorted(fb)
    for k, v in fa.items():
        if k in skip:
            continue
        w = fb[k]
        if hasattr(v, "tensor"):
            v, w = v.tensor, w.tensor
        if isinstance(v, torch.Tensor):
            assert v.dtype == w.dtype and torch.equal(v.contiguous().view(torch.uint8), w.contiguous().view(torch.uint8)), k
        elif isinstance(v, (list, tuple, str)):
            assert v == w, k
        else:
            assert np.array_equal(np.asarray(v), np.asarray(w)), k


def test_run_rotated_against_the_steps_by_hand():
    from glass_amd.data import RotationTransform
    from glass_amd.ops import native as K
    from glass_amd.utils.synth import make_image
    run = _runner(["MODEL.ROI_RECOGNIZER_HEAD.CHAR_BOXES", True])
    assert run.input_format != "GREY"                                    # by hand below, the rotated image goes in as a host image
    img = make_image(0, 120, 150).numpy()
    base = run.run_batch([img])[0]
    assert len(base) > 0, "no word survived: the case checks nothing"
    for angle in (0, 360, -720.0):
        _fields_equal(run.run_rotated(img, angle, (5, 6, 7)), base)      # bit for bit, every field
    worst = 0
    for angle in (33.3, 90):
        t = RotationTransform(120, 150, angle)
        got = run.run_rotated(img, angle, (7, 200, 255))
        rotated = K.rotate_u8(torch.from_numpy(img).to(DEV), t, (7, 200, 255)).cpu().numpy()
        hand = run.run_batch([rotated])[0]
        assert hand.image_size == t.out_hw and got.image_size == (120, 150) and len(got) == len(hand) > 0
        hand._image_size = (120, 150)
        mapped = ("pred_boxes", "pred_char_frames")
        assert got.has("pred_char_frames") and got.has("pred_polygons")
        _fields_equal(got, hand, skip=mapped + ("pred_polygons",))
        poly = t.inverse_coords(hand.pred_polygons.cpu().numpy()).astype(np.float32)      # the corners are points
        worst = max(worst, _ulps(got.pred_polygons.cpu().numpy(), poly))
        for name in mapped:
            g, h = got.get(name), hand.get(name)
            g, h = (g.tensor if hasattr(g, "tensor") else g), (h.tensor if hasattr(h, "tensor") else h)
            want = t.inverse_rotated_boxes(h.cpu().numpy())
            worst = max(worst, _ulps(g.cpu().numpy(), want))
            assert not np.array_equal(g.cpu().numpy(), h.cpu().numpy()), name          # it was mapped
        # the boxes are in the original frame: their centres lie inside the original image, up to the box's own extent
        c = got.pred_boxes.tensor.cpu().numpy()
        assert ((c[:, 0] > -100) & (c[:, 0] < 250) & (c[:, 1] > -100) & (c[:, 1] < 220)).all()
    print(f"[rotate] run_rotated: boxes within {worst} float32 ulp of the host inverse map")
    assert worst <= 1
    # the two refusals, named by their keys
    heads = run.model.roi_heads
    before = (getattr(heads, "mask_inference", False), getattr(run.model, "paste_masks", True))
    try:
        heads.mask_inference, run.model.paste_masks = True, True
        with pytest.raises(NotImplementedError, match="PASTE_MASKS"):
            run.run_rotated(img, 30)
    finally:
        heads.mask_inference, run.model.paste_masks = before
    run.cfg.defrost()
    run.cfg.POST_PROCESSING.GROUP_LINES = True
    try:
        with pytest.raises(NotImplementedError, match="GROUP_LINES"):
            run.run_rotated(img, 30)
    finally:
        run.cfg.POST_PROCESSING.GROUP_LINES = False
    with pytest.raises(ValueError):
        run.run_rotated(img, float("nan"))
    with pytest.raises(ValueError, match="fill"):
        run.run_rotated(img, 30, (0, 0, 300))


# ---------------------------------------------------------------------------------------------------- scorer consistency
SIZES6 = [(480, 640), (360, 500), (500, 360), (97, 333), (640, 640), (200, 150)]
SWEEP_ANGLES = [0, 30, 45, 60, 90, -170]


@functools.lru_cache(maxsize=None)
def _quads():
    """6 images' worth of seeded rotated boxes, apart from each other, the integer quads of their corners as ground truth, and a
    word for each.  The short side is at least 12 px (the issue asks for at least 8): a ground-truth corner is rounded twice
    (here, and after the rotation) and a detection's once, at most 0.71 px each time, so an edge moves by at most 1.41 px on
    one side and 0.71 px on the other and the IoU of a 12 px box with itself stays above (12 - 2.83) / (12 + 1.41) = 0.68 along
    its short side.  The test below checks the actual values with the rational checker."""
    import random
    from glass_amd.evaluation import rotated_boxes_to_polygons
    r = random.Random(41)
    words = ["hello", "World", "STOP", "cafe", "exit", "street", "OPEN", "sale"]
    boxes, gt = OrderedDict(), OrderedDict()
    for i, (h, w) in enumerate(SIZES6):
        bs = []
        for k in range(4):
            cx, cy = w * (0.25 + 0.5 * (k % 2)), h * (0.25 + 0.5 * (k // 2))             # one per quadrant: no overlaps
            bs.append([cx + r.uniform(-3, 3), cy + r.uniform(-3, 3), r.uniform(0.2, 0.3) * min(h, w), r.uniform(12, 0.12 * min(h, w) + 8),
                       r.choice([0.0, 15.0, -30.0, 90.0, 7.5])])
        b = np.array(bs, dtype=np.float32)
        key = str(i + 1)
        boxes[key] = b
        q = rotated_boxes_to_polygons(b.astype(np.float64))
        gt[key] = ([[int(np.floor(v + 0.5)) for p in quad for v in p] for quad in q], [words[(i + k) % len(words)] for k in range(4)])
    return boxes, gt


def test_rotated_boxes_score_perfectly_against_rotated_ground_truth():
    from glass_amd.data import RotationTransform
    from glass_amd.evaluation import RRCScorer, normalize_detection_line, rotate_ground_truth, rotated_boxes_to_polygons
    from glass_amd.ops import native as K
    boxes, gt = _quads()
    sizes = {str(i + 1): hw for i, hw in enumerate(SIZES6)}
    low = Fraction(1)
    for angle in SWEEP_ANGLES:
        gt_a = rotate_ground_truth(gt, sizes, angle)
        sub = OrderedDict()
        for key, b in boxes.items():
            t = RotationTransform(*sizes[key], angle)
            moved = K.rotate_boxes(torch.from_numpy(b).to(DEV), t).cpu().numpy()
            q = rotated_boxes_to_polygons(moved.astype(np.float64))
            sub[key] = [normalize_detection_line(",".join(f"{int(np.floor(p[0] + 0.5))},{int(np.floor(p[1] + 0.5))}" for p in quad) + ",####" + word)
                        for quad, word in zip(q, gt[key][1])]
            assert None not in sub[key], (angle, key)
        # the rational checker: every matching pair far above 0.5, every other pair far below, so integer rounding decides nothing
        exact = RC.check_score(gt_a, sub, False)
        for key, s in exact["per_sample"].items():
            for g, row in enumerate(s["iouMat"]):
                for d, v in enumerate(row):
                    assert (v > Fraction(6, 10)) if g == d else (v < Fraction(1, 10)), (angle, key, g, d, float(v))
                    if g == d:
                        low = min(low, v)
        got = RRCScorer(gt_a, False, DEV).score({k + ".txt": v for k, v in sub.items()})
        assert got["e2e_method"] == exact["e2e_method"] == "E2E_RESULTS: precision: 1.0, recall: 1.0, hmean: 1.0", (angle, got["e2e_method"])
        assert got["det_only_method"] == "DETECTION_ONLY_RESULTS: precision: 1.0, recall: 1.0, hmean: 1.0", (angle, got["det_only_method"])
    print(f"[rotate] scorer consistency: lowest exact IoU of a matching pair {float(low):.4f}")


# ---------------------------------------------------------------------------------------------------- rotation_sweep
def _encoder():
    from glass_amd.config import get_glass_cfg
    from glass_amd.modeling.recognition.text_encoder import TextEncoder
    cfg = get_glass_cfg()
    cfg.MODEL.ROI_RECOGNIZER_HEAD.NAME = "RecognizerRCNNHeadV3"
    cfg.MODEL.ROI_RECOGNIZER_HEAD.MAX_WORD_LENGTH = 25
    return TextEncoder(cfg)


class _StubModel:
    """what the driver needs of a model; returns the ground-truth boxes of each image, moved as the image was, as instances"""

    class backbone:
        size_divisibility = 32

    def __init__(self, enc, boxes, words, fail_at=None):
        self.enc, self.boxes, self.words, self.fail_at, self.seen = enc, boxes, words, fail_at, []

    @staticmethod
    def input_size(x):
        return int(x["resize"][0]), int(x["resize"][1])

    def __call__(self, inputs):
        from glass_amd.ops import native as K
        from glass_amd.structures.core import Instances, RotatedBoxes
        outs = []
        for inp in inputs:
            key = str(int(os.path.basename(inp["file_name"])[4:-4]))
            rot = inp.get("rotation")
            self.seen.append((key, None if rot is None else rot.angle, (inp["height"], inp["width"])))
            if self.fail_at is not None and rot is not None and rot.angle == self.fail_at:
                raise RuntimeError("the stub fails here")
            b = torch.from_numpy(self.boxes[key]).to(DEV)
            if rot is not None:
                assert tuple(inp["image_u8"].shape[:2]) == rot.out_hw == (inp["height"], inp["width"])
                b = K.rotate_boxes(b, rot)
            inst = Instances((inp["height"], inp["width"]))
            inst.pred_boxes = RotatedBoxes(b.cpu())
            inst.scores = torch.full((len(b),), 0.9)
            inst.pred_classes = torch.zeros(len(b), dtype=torch.int64)
            labels = self.enc.encode(self.words[key])[:, 1:]
            # 0.99 per character: the word score is the product over the steps and must pass the 0.5 text threshold
            inst.pred_text_prob = torch.full((len(b), labels.shape[1], len(self.enc.character)), 0.0001).scatter_(2, labels.unsqueeze(-1), 0.99)
            outs.append({"instances": inst})
        return outs


def test_rotation_sweep_on_a_stub_model():
    from glass_amd.config import get_glass_cfg
    from glass_amd.data import DatasetMapper
    from glass_amd.evaluation import TextResultWriter, rotation_sweep
    boxes, gt = _quads()
    enc = _encoder()
    cfg = get_glass_cfg(YAML, ["MODEL.DEVICE", DEV, "INPUT.MIN_SIZE_TEST", 64, "INPUT.MAX_SIZE_TEST", 128])
    dds = [{"file_name": f"/data/set_9/img_{i + 1}.jpg", "image": C.make_image(h, w), "height": h, "width": w} for i, (h, w) in enumerate(SIZES6)]
    mapper = DatasetMapper(cfg, device=DEV, fused=True, rotate=12.5)
    writer = TextResultWriter(enc, dataset="icdar15")
    model = _StubModel(enc, boxes, {k: v[1] for k, v in gt.items()})
    got = rotation_sweep(model, dds, mapper, writer, gt, SWEEP_ANGLES, batch_size=4)
    assert list(got) == SWEEP_ANGLES and mapper.rotate == 12.5           # put back
    perfect = {"precision": 1.0, "recall": 1.0, "hmean": 1.0}
    for angle, res in got.items():
        assert res == OrderedDict([("E2E_RESULTS", perfect), ("DETECTION_ONLY_RESULTS", perfect)]), (angle, res)
    assert len(model.seen) == len(SWEEP_ANGLES) * len(dds)
    assert {a for _, a, _ in model.seen} == {None, 30.0, 45.0, 60.0, 90.0, 190.0}      # angle 0: the untouched path
    assert all(hw == SIZES6[int(k) - 1] for k, a, hw in model.seen if a is None)
    assert all(hw == SIZES6[int(k) - 1][::-1] for k, a, hw in model.seen if a == 90.0)
    # a wrong ground truth does not score: the sweep is not vacuous
    shifted = OrderedDict((k, ([[v + 1000 for v in ring] for ring in rings], texts)) for k, (rings, texts) in gt.items())
    assert rotation_sweep(model, dds, mapper, writer, shifted, [30], batch_size=4)[30]["DETECTION_ONLY_RESULTS"]["hmean"] < 0.5
    # put back after an exception, too
    failing = _StubModel(enc, boxes, {k: v[1] for k, v in gt.items()}, fail_at=45.0)
    with pytest.raises(RuntimeError, match="the stub fails here"):
        rotation_sweep(failing, dds, mapper, writer, gt, [30, 45, 60])
    assert mapper.rotate == 12.5
    with pytest.raises(KeyError, match="'7'"):
        rotation_sweep(model, dds, mapper, writer, OrderedDict(list(gt.items()) + [("7", ([], []))]), [30])
    assert mapper.rotate == 12.5
