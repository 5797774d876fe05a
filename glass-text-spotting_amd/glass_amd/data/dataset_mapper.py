"""`DatasetMapper(cfg, is_train=False)`: the reference's test-time mapper on the HIP pipeline.

Mirrors reference glass/data/dataset_mapper.py:17-168 for inference: read the image in cfg.INPUT.FORMAT
(`_read_and_verify_image` :161-168, GREY through rgb2grey on the host uint8 image), resize it with
`ResizeShortestEdge(INPUT.MIN_SIZE_TEST, INPUT.MAX_SIZE_TEST)` (`utils.build_transform_gen(cfg, False)` :45
[d2-recall]) and hand the model a uint8 CHW "image" (:110).  The resize is PIL's bilinear on the uint8 image, done on the
device byte for byte (ops.native.pil_resize_u8).  With `fused=True` the mapper only uploads the image and names the target
size; the model's preprocess_image then resizes, normalises and pads in one launch pair (ops.native.pil_resize_into_batch).
Ground-truth annotations are dropped, not transformed; training (crop, random rotation, annotation transforms) is out of
scope.  `rotate` (degrees, counter-clockwise) is the rotated-image evaluation: the decoded uint8 image is rotated before the
resize as `PIL.Image.rotate(angle, BILINEAR, expand=True, fillcolor=rotate_fill)` rotates it, on the device byte for byte
(ops.native.rotate_u8), and the output carries the `RotationTransform` that moves ground truth and boxes with it
(evaluation/rotated.py).
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch

from ..ops import native as K
from .transforms import ResizeShortestEdge, RotationTransform, check_fill, pil_resize_u8_host, rotate_u8_host


def rgb2grey_three_channels(image: np.ndarray) -> np.ndarray:
    """reference glass/utils/common_utils.py:29-43 (rgb2grey, three_channels=True): Y'709 weights on channels 0,1,2,
    truncated to uint8, replicated three times (as GlassRunner._image_to_tensor does)"""
    g = np.uint8(0.2125 * image[:, :, 0] + 0.7154 * image[:, :, 1] + 0.0721 * image[:, :, 2])
    return np.repeat(g[:, :, None], 3, axis=2)


def read_image(file_name: str, fmt: str) -> np.ndarray:
    """detectron2 detection_utils.read_image [d2-recall]: PIL decode, EXIF orientation applied, RGB, channels reversed
    for BGR -> uint8 HWC"""
    try:
        from PIL import Image, ImageOps
    except ImportError as e:            # decoding is the one thing here that needs PIL
        raise RuntimeError("decoding a 'file_name' needs PIL; pass an already decoded 'image' instead") from e
    with Image.open(file_name) as im:
        im = ImageOps.exif_transpose(im)
        a = np.array(im.convert("RGB"))
    return a[:, :, ::-1] if fmt == "BGR" else a


class DatasetMapper:
    """`mapper(dataset_dict)` -> the model's input dict.  The dict names a "file_name" to decode, or carries an already
    decoded "image": uint8 HWC in cfg.INPUT.FORMAT channel order (for GREY: RGB, converted here as GlassRunner converts its
    input).  "annotations" are dropped; "file_name" and every other key are kept, "height" / "width" are the original
    image's.  fused=False: "image" = the resized uint8 CHW tensor, the reference mapper's output.  fused=True: the raw
    form {"image_u8": uint8 [H,W,3] on the device, "resize": (Ho, Wo)} that GeneralizedRCNN.preprocess_image resizes.
    rotate != 0 (degrees; the attribute may be set between calls): the image is rotated after the GREY conversion and the size
    check and before the resize, "height" / "width" are the ROTATED image's (the model and the writer see the rotated file),
    and "rotation" is the RotationTransform.  rotate == 0: the dict is what it is without the feature and nothing is launched."""

    def __init__(self, cfg, is_train: bool = False, device=None, fused: bool = True, rotate: float = 0.0, rotate_fill=(0, 0, 0)):
        if is_train:
            raise NotImplementedError("glass_amd builds the inference hot path only; training is out of scope")
        self.img_format = cfg.INPUT.FORMAT
        assert self.img_format in ("RGB", "BGR", "GREY"), self.img_format
        self.resize = ResizeShortestEdge(cfg.INPUT.MIN_SIZE_TEST, cfg.INPUT.MAX_SIZE_TEST)
        self.device = torch.device(device if device is not None else cfg.MODEL.DEVICE)
        self.fused = bool(fused)
        self.is_train = False
        self.rotate = self.check_rotate(rotate)
        self.rotate_fill = check_fill(rotate_fill)

    @staticmethod
    def check_rotate(angle) -> float:
        angle = float(angle)
        if not np.isfinite(angle):
            raise ValueError(f"rotate {angle}: needs a finite angle in degrees")
        return angle

    def _host_image(self, dataset_dict: Dict) -> np.ndarray:
        if dataset_dict.get("image") is not None:
            image = dataset_dict["image"]
            image = image.cpu().numpy() if isinstance(image, torch.Tensor) else np.asarray(image)
            if self.img_format == "GREY":
                image = rgb2grey_three_channels(image)
        elif self.img_format == "GREY":
            image = rgb2grey_three_channels(read_image(dataset_dict["file_name"], "RGB"))
        else:
            image = read_image(dataset_dict["file_name"], self.img_format)
        if image.dtype != np.uint8 or image.ndim != 3 or image.shape[2] != 3:
            raise ValueError(f"expected a uint8 HWC image with 3 channels, got {image.dtype} {image.shape}")
        return np.ascontiguousarray(image)

    def __call__(self, dataset_dict: Dict) -> Dict:
        image = self._host_image(dataset_dict)
        h, w = image.shape[:2]
        for key in ("height", "width"):            # detection_utils.check_image_size [d2-recall]
            if key in dataset_dict and int(dataset_dict[key]) != (h, w)[key == "width"]:
                raise ValueError(f"{dataset_dict.get('file_name')}: {key} {dataset_dict[key]} does not match the image {h}x{w}")
        out = {k: v for k, v in dataset_dict.items() if k not in ("annotations", "image")}
        rotation = None
        if self.check_rotate(self.rotate) != 0.0:
            rotation = RotationTransform(h, w, self.rotate)
            h, w = rotation.out_hw
            out["rotation"] = rotation
        out["height"], out["width"] = h, w
        out_hw = self.resize.get_output_shape(h, w)
        if rotation is not None and self.device.type != "cuda":
            image = rotate_u8_host(image, rotation, self.rotate_fill)
        u8 = torch.from_numpy(image).to(self.device)
        if rotation is not None and self.device.type == "cuda":
            u8 = K.rotate_u8(u8, rotation, self.rotate_fill)
        if self.fused:
            out["image_u8"], out["resize"] = u8, out_hw
        elif self.device.type == "cuda":
            out["image"] = K.pil_resize_u8(u8, out_hw).permute(2, 0, 1).contiguous()
        else:       # a mapper explicitly placed on the host (a loader worker without a GPU): the numpy statement, same bytes
            out["image"] = torch.from_numpy(pil_resize_u8_host(image, out_hw)).permute(2, 0, 1).contiguous()
        return out
