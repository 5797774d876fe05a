"""Device side of the test-time resize: the two PIL-bilinear passes (csrc/resize_pil.hip) against the numpy statement
byte for byte, the fused write into the batch against resize + cast + preprocess_image bit for bit, the argument checks,
and the raw input form through the model and the evaluation driver."""
import functools
import os

import numpy as np
import pytest
import torch

import resize_pil_cases as C

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"


def _gpu_resize(img, out_hw):
    from glass_amd.ops import native as K
    return K.pil_resize_u8(torch.from_numpy(img).to(DEV), out_hw).cpu().numpy()


@pytest.mark.parametrize("name", list(C.CASES))
def test_resize_equals_host(name):
    from glass_amd.data import pil_resize_u8_host
    (_, out_hw, _), img = C.CASES[name], C.make_input(name)
    got = _gpu_resize(img, out_hw)
    assert got.dtype == np.uint8 and got.shape == tuple(out_hw) + (3,)
    assert np.array_equal(got, pil_resize_u8_host(img, out_hw))


def test_resize_protocol_shape():
    """720 x 1280 -> 1000 x 1778 once: nothing new in the arithmetic, only the widest indices the protocol uses"""
    from glass_amd.data import pil_resize_u8_host
    img = C.make_input(C.PROTOCOL)
    assert np.array_equal(_gpu_resize(img, C.PROTOCOL[1]), pil_resize_u8_host(img, C.PROTOCOL[1]))


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("name", ["up_7x5", "down_37x53", "x_only", "y_only", "same", "wide"])
def test_into_batch_equals_resize_then_preprocess(name, flip):
    from glass_amd.ops import native as K
    (_, (Ho, Wo), _) = C.CASES[name]
    img = torch.from_numpy(C.make_input(name)).to(DEV)
    mean, std = [103.53, 116.28, 123.675], [57.375, 57.12, 58.395]
    Hp, Wp = Ho + 5, Wo + 11                                       # both larger than the image: a pad region on each axis
    got = torch.full((3, Hp, Wp, 4), float("nan"), dtype=torch.float32, device=DEV)
    K.pil_resize_into_batch(img, (Ho, Wo), mean, std, got, 1, flip_channels=flip)
    u8 = K.pil_resize_u8(img, (Ho, Wo))
    if flip:
        u8 = u8.flip(2)
    want = torch.full_like(got, float("nan"))
    K.preprocess_image(u8.permute(2, 0, 1).float().contiguous(), mean, std, want, 1)
    got, want = got.cpu(), want.cpu()
    assert torch.isnan(got[0]).all() and torch.isnan(got[2]).all()             # the neighbours are untouched
    assert torch.equal(got[1].view(torch.int32), want[1].view(torch.int32))    # bit-equal, -0.0 and all
    assert (got[1, Ho:] == 0).all() and (got[1, :, Wo:] == 0).all() and (got[1, :, :, 3] == 0).all()
    assert not torch.isnan(got[1]).any()


def test_argument_checks_raise_before_launch():
    from glass_amd._lib import GlassLibraryError
    from glass_amd.ops import native as K
    img = torch.from_numpy(C.make_input("down_37x53")).to(DEV)
    out_hw = C.CASES["down_37x53"][1]
    small = torch.empty((37 * 31 * 3 - 1,), dtype=torch.uint8, device=DEV)
    with pytest.raises(GlassLibraryError, match="workspace"):
        K.pil_resize_u8(img, out_hw, workspace=small)
    batch = torch.zeros((1, 32, 32, 4), dtype=torch.float32, device=DEV)
    with pytest.raises(GlassLibraryError, match="workspace"):
        K.pil_resize_into_batch(img, out_hw, [0, 0, 0], [1, 1, 1], batch, 0, workspace=small)
    with pytest.raises(GlassLibraryError, match="does not fit"):               # Ho = 20 > Hp = 16
        K.pil_resize_into_batch(img, out_hw, [0, 0, 0], [1, 1, 1], torch.zeros((1, 16, 32, 4), device=DEV), 0)
    with pytest.raises(GlassLibraryError, match="slot"):
        K.pil_resize_into_batch(img, out_hw, [0, 0, 0], [1, 1, 1], batch, 1)
    with pytest.raises(GlassLibraryError):
        K.pil_resize_u8(img.cpu(), out_hw)
    torch.cuda.synchronize()
    assert (batch == 0).all()                                                  # nothing was launched


# ---------------------------------------------------------------- the raw form through the model
@functools.lru_cache(maxsize=None)
def _model():
    import glass_amd
    from glass_amd.config import get_glass_cfg
    from glass_amd.utils.synth import make_state_dict
    cfg = get_glass_cfg(os.path.join(ROOT, "configs", "glass_icdar15_mi355x.yaml"),
                        ["MODEL.DEVICE", DEV, "INPUT.MIN_SIZE_TEST", 128, "INPUT.MAX_SIZE_TEST", 1000,
                         "POST_PROCESSING.TEXT_THRESHOLD", 0.0])
    m = glass_amd.build_model(cfg)
    m.load_state_dict(make_state_dict(1234))
    return cfg, m


def _dataset(sizes):
    from glass_amd.utils.synth import make_image
    return [{"file_name": f"img_{i}.jpg", "image": make_image(i, h, w).numpy(), "annotations": []} for i, (h, w) in enumerate(sizes)]


def test_model_takes_the_raw_form():
    from glass_amd.data import DatasetMapper
    from glass_amd.utils.synth import make_boxes
    cfg, model = _model()
    dd = _dataset([(96, 128)])[0]
    raw = DatasetMapper(cfg, device=DEV, fused=True)(dd)
    cooked = DatasetMapper(cfg, device=DEV, fused=False)(dd)
    assert raw["resize"] == (128, 171) and tuple(cooked["image"].shape) == (3, 128, 171)      # it is resized
    a, b = model.preprocess_image([raw]), model.preprocess_image([cooked])
    assert a.image_sizes == b.image_sizes == [(128, 171)] and tuple(a.nhwc4.shape) == (1, 128, 192, 4)
    assert torch.equal(a.nhwc4.view(torch.int32), b.nhwc4.view(torch.int32))
    boxes = [(make_boxes(0, 3, 128, 171) * torch.tensor([1, 1, 0.3, 0.5, 1.0])).to(DEV)]
    outs = []
    for inp in (raw, cooked):
        o = model.inference([inp], do_postprocess=False, override_boxes=boxes)
        outs.append((o[0], o.batch))
    (ia, da), (ib, db) = outs
    assert ia.pred_text_prob.shape == (3, 26, 97) and torch.equal(ia.pred_text_prob, ib.pred_text_prob)
    assert torch.equal(da.boxes, db.boxes) and torch.equal(da.scores, db.scores) and torch.equal(da.counts_dev, db.counts_dev)
    for x, y in zip(da.proposals, db.proposals):                               # the RPN's own boxes, logits and counts
        assert torch.equal(x, y)
    assert int(da.proposals[2][0]) > 0
    if da.detected is not None:                                                # the box head's own detections
        assert torch.equal(da.detected.boxes, db.detected.boxes) and torch.equal(da.detected.scores, db.detected.scores)
        assert torch.equal(da.detected.counts_dev, db.detected.counts_dev)


def _same_instances(a, b, exact):
    """exact: the two came from calls of the same batch size, so from the same kernels: torch.equal.  Otherwise a layer may
    have taken another kernel (which one depends on how many output pixels the call has: fp32 summation order), and "the
    same" is the bar tests/test_gpu_e_host_tail.py sets for GlassRunner.run_batch against image-by-image calls: the same
    detections in the same order, boxes within 1e-3 px, every other float within 1e-4, integers and texts identical."""
    assert len(a) == len(b) and a.image_size == b.image_size
    fa, fb = a.get_fields(), b.get_fields()
    assert sorted(fa) == sorted(fb)
    for k, v in fa.items():
        w = fb[k]
        if hasattr(v, "tensor"):
            v, w = v.tensor, w.tensor
        if not isinstance(v, torch.Tensor):
            assert np.array_equal(np.asarray(v), np.asarray(w)), k
        elif exact or not v.is_floating_point():
            assert torch.equal(v, w), k
        else:
            np.testing.assert_allclose(v.cpu().numpy(), w.cpu().numpy(), rtol=0, atol=1e-3 if ("box" in k or "polygon" in k) else 1e-4, err_msg=k)   # pixels / the rest


@pytest.mark.parametrize("fused", [True, False])
def test_inference_on_dataset_equals_image_by_image(fused):
    from glass_amd.data import DatasetMapper
    from glass_amd.evaluation import inference_on_dataset
    cfg, model = _model()
    dds = _dataset([(96, 128), (96, 160), (96, 130)])              # -> 128 x 171 / 213 / 173: padded 192, 224, 192 wide
    mapper = DatasetMapper(cfg, device=DEV, fused=fused)

    class Writer:
        def __init__(self):
            self.seen = []

        def process(self, inputs, outputs):
            assert len(inputs) == len(outputs)
            self.seen.append([i["file_name"] for i in inputs])

    w = Writer()
    got = inference_on_dataset(model, dds, mapper, writer=w, batch_size=8)
    assert w.seen == [["img_0.jpg", "img_2.jpg"], ["img_1.jpg"]]  # grouped by padded shape
    w1 = Writer()
    got1 = inference_on_dataset(model, dds, mapper, writer=w1, batch_size=1)
    assert w1.seen == [["img_0.jpg"], ["img_1.jpg"], ["img_2.jpg"]]
    assert len(got) == len(got1) == 3
    assert sum(len(g["instances"]) for g in got) > 0
    for dd, g, g1 in zip(dds, got, got1):
        one = model([mapper(dd)])[0]
        assert g["instances"].image_size == (96, dd["image"].shape[1])         # back at the original size
        _same_instances(g1["instances"], one["instances"], exact=True)         # input order, one image per call
        _same_instances(g["instances"], one["instances"], exact=False)         # img_0 and img_2 shared a call
