"""Test-time image transform of the evaluation protocol: detectron2's `ResizeShortestEdge` on a uint8 image, which is
`PIL.Image.resize(..., BILINEAR)` [d2-recall: detectron2 v0.6 data/transforms/augmentation_impl.py ResizeShortestEdge,
transform.py ResizeTransform.apply_image; detectron2 is not vendored in the reference], stated in numpy.

`pil_bilinear_coeffs` makes the per-axis tables the device kernels (csrc/resize_pil.hip) read; `pil_resize_u8_host` is the
readable form of the whole resize and the cross-check of the kernels, byte for byte equal to PIL (tests/test_resize_pil.py).
"""
from __future__ import annotations

import functools
import math
from typing import Tuple

import numpy as np

PRECISION_BITS = 32 - 8 - 2          # PIL src/libImaging/Resample.c: 8 bits of pixel, 2 of headroom


class ResizeShortestEdge:
    """The size rule of detectron2's ResizeShortestEdge(short_edge_length, max_size) at test time (one length, no
    sampling) [d2-recall: ResizeShortestEdge.get_output_shape].  `short == 0` means no resize."""

    def __init__(self, short: int, max_size: int):
        self.short, self.max_size = int(short), int(max_size)

    def get_output_shape(self, h: int, w: int) -> Tuple[int, int]:
        h, w = int(h), int(w)
        size = self.short
        if size == 0:
            return h, w
        scale = size * 1.0 / min(h, w)
        if h < w:
            newh, neww = size, scale * w
        else:
            newh, neww = scale * h, size
        if max(newh, neww) > self.max_size:
            scale = self.max_size * 1.0 / max(newh, neww)
            newh = newh * scale
            neww = neww * scale
        return int(newh + 0.5), int(neww + 0.5)


@functools.lru_cache(maxsize=64)
def pil_bilinear_coeffs(in_size: int, out_size: int) -> Tuple[np.ndarray, np.ndarray]:
    """PIL's `precompute_coeffs` + `normalize_coeffs_8bpc` for the triangle filter (support 1) on one axis:
    k int32 [out, ksize] (22-bit fixed point, zero past a row's taps) and bounds int32 [out, 2] = (first tap, tap count).
    float64 in PIL's own order of operations; cached per (in, out) - the arrays are read-only."""
    in_size, out_size = int(in_size), int(out_size)
    assert in_size > 0 and out_size > 0
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = 1.0 * fs
    ss = 1.0 / fs
    ksize = int(np.ceil(support)) * 2 + 1
    center = (np.arange(out_size, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)          # C truncation, as (int) in PIL
    xmax = np.minimum((center + support + 0.5).astype(np.int64), in_size)
    n = xmax - xmin
    x = np.arange(ksize, dtype=np.int64)[None, :]
    a = np.abs((x + xmin[:, None] - center[:, None] + 0.5) * ss)
    w = np.where((a < 1.0) & (x < n[:, None]), 1.0 - a, 0.0)
    ww = np.zeros(out_size, dtype=np.float64)
    for t in range(ksize):               # the running sum in tap order (np.sum adds pairwise); the zeros past n add nothing
        ww = ww + w[:, t]
    w = np.where(ww[:, None] != 0.0, w / np.where(ww != 0.0, ww, 1.0)[:, None], w)
    k = (0.5 + w * float(1 << PRECISION_BITS)).astype(np.int32)             # w >= 0: PIL's negative branch never fires
    k[x >= n[:, None]] = 0
    bounds = np.stack([xmin, n], axis=1).astype(np.int32)
    k.setflags(write=False)
    bounds.setflags(write=False)
    return k, bounds


def _pass(img: np.ndarray, axis: int, out_size: int) -> np.ndarray:
    """one separable pass over `axis` (0 vertical, 1 horizontal) of a uint8 [H,W,C] image"""
    in_size = img.shape[axis]
    k, bounds = pil_bilinear_coeffs(in_size, out_size)
    shape = list(img.shape)
    shape[axis] = out_size
    acc = np.full(shape, 1 << (PRECISION_BITS - 1), dtype=np.int64)
    for t in range(k.shape[1]):
        idx = np.minimum(bounds[:, 0] + t, in_size - 1)        # taps past a row's count have k == 0
        kt = k[:, t].astype(np.int64)
        if axis == 1:
            acc += kt[None, :, None] * img[:, idx, :]
        else:
            acc += kt[:, None, None] * img[idx, :, :]
    return np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)


def pil_resize_u8_host(img: np.ndarray, out_hw: Tuple[int, int]) -> np.ndarray:
    """`PIL.Image.fromarray(img).resize((Wo, Ho), BILINEAR)` of a uint8 HWC image in numpy: the horizontal pass first,
    a uint8 image between the passes, a pass whose axis keeps its size skipped."""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 3, (img.dtype, img.shape)
    Ho, Wo = int(out_hw[0]), int(out_hw[1])
    if img.shape[:2] == (Ho, Wo):
        return np.array(img, order="C")
    if img.shape[1] != Wo:
        img = _pass(img, 1, Wo)
    if img.shape[0] != Ho:
        img = _pass(img, 0, Ho)
    return np.ascontiguousarray(img)


# ------------------------------------------------------------------ rotation: PIL.Image.rotate(angle, BILINEAR, expand=True, fillcolor)
def _affine(x: float, y: float, m) -> Tuple[float, float]:
    """PIL's `transform(x, y, matrix)` of Image.rotate: Python floats, two products and two additions left to right"""
    return m[0] * x + m[1] * y + m[2], m[3] * x + m[4] * y + m[5]


class RotationTransform:
    """`PIL.Image.rotate(angle, expand=True)` of an h x w image as a map of images, points and rotated boxes: the rotation
    about the centre by `angle` degrees counter-clockwise on an enlarged canvas.  Everything is float64 on the host and is
    the statement the device kernels (csrc/image_rotate.hip, include/glass_hip_feature_rotate.h) equal.

    .angle           angle % 360.0
    .kind            0..3 where the reduced angle is 0, 90, 180, 270: PIL takes its copy / transpose shortcuts there and the
                     rotated image is np.rot90(image, kind); 4 otherwise (the affine bilinear form)
    .matrix          6 floats, OUTPUT -> INPUT in continuous coordinates (a pixel centre is +0.5), built as PIL builds it:
                     cos and sin rounded to 15 decimals, the centre (w/2, h/2), the canvas from the four mapped corners
    .inverse_matrix  INPUT -> OUTPUT, the float64 inverse (for kind 0..3 both are the exact transpose maps)
    .out_hw          the rotated image's (height, width)"""

    def __init__(self, h: int, w: int, angle: float):
        h, w, angle = int(h), int(w), float(angle)
        if h < 1 or w < 1:
            raise ValueError(f"RotationTransform: a {h}x{w} image")
        if not math.isfinite(angle):
            raise ValueError(f"RotationTransform: angle {angle}")
        self.h, self.w = h, w
        self.angle = angle % 360.0
        self.kind = {0.0: 0, 90.0: 1, 180.0: 2, 270.0: 3}.get(self.angle, 4)
        if self.kind < 4:
            self.out_hw = (h, w) if self.kind in (0, 2) else (w, h)
            W, H = float(w), float(h)
            m, inv = {0: ([1, 0, 0, 0, 1, 0], [1, 0, 0, 0, 1, 0]),
                      1: ([0, -1, W, 1, 0, 0], [0, 1, 0, -1, 0, W]),          # out[i, j] = in[j, w - 1 - i]
                      2: ([-1, 0, W, 0, -1, H], [-1, 0, W, 0, -1, H]),
                      3: ([0, 1, 0, -1, 0, H], [0, -1, H, 1, 0, 0])}[self.kind]   # out[i, j] = in[h - 1 - j, i]
            self.matrix = tuple(float(v) for v in m)
            self.inverse_matrix = tuple(float(v) for v in inv)
            return
        a = -math.radians(self.angle)
        m = [round(math.cos(a), 15), round(math.sin(a), 15), 0.0, round(-math.sin(a), 15), round(math.cos(a), 15), 0.0]
        cx, cy = w / 2, h / 2
        m[2], m[5] = _affine(-cx, -cy, m)
        m[2] += cx
        m[5] += cy
        xx, yy = zip(*(_affine(x, y, m) for x, y in ((0, 0), (w, 0), (w, h), (0, h))))
        nw = math.ceil(max(xx)) - math.floor(min(xx))
        nh = math.ceil(max(yy)) - math.floor(min(yy))
        m[2], m[5] = _affine(-(nw - w) / 2.0, -(nh - h) / 2.0, m)
        self.out_hw = (int(nh), int(nw))
        self.matrix = tuple(m)
        det = m[0] * m[4] - m[1] * m[3]
        i0, i1, i3, i4 = m[4] / det, -m[1] / det, -m[3] / det, m[0] / det
        self.inverse_matrix = (i0, i1, -(i0 * m[2] + i1 * m[5]), i3, i4, -(i3 * m[2] + i4 * m[5]))

    @staticmethod
    def _map(pts, m) -> np.ndarray:
        p = np.asarray(pts, dtype=np.float64)
        if p.shape[-1:] != (2,):
            raise ValueError(f"points {p.shape}: the last axis must be (x, y)")
        x, y = p[..., 0], p[..., 1]
        return np.stack([m[0] * x + m[1] * y + m[2], m[3] * x + m[4] * y + m[5]], axis=-1)

    def apply_coords(self, pts) -> np.ndarray:
        """points [..., 2] of the original image -> the rotated image (float64, continuous coordinates)"""
        return self._map(pts, self.inverse_matrix)

    def inverse_coords(self, pts) -> np.ndarray:
        """points [..., 2] of the rotated image -> the original image"""
        return self._map(pts, self.matrix)

    @staticmethod
    def map_rotated_boxes(boxes, m, theta: float) -> np.ndarray:
        """rows (cx, cy, w, h, a) [..., 5]: the centre through `m`, w and h kept, a + theta wrapped into [-180, 180)
        [reference glass/data/transforms/transform.py:21-29 rotate_rotated_box: the angle adds]; every value widened to
        float64, the result rounded to float32 once; a row with a non-finite value is copied bit for bit.  The statement of
        glass_rotate_boxes.  A float64 array stays float64 (nothing is rounded): the map itself, for checks below float32."""
        boxes = np.asarray(boxes)
        dtype = np.float64 if boxes.dtype == np.float64 else np.float32
        src = np.ascontiguousarray(boxes, dtype=dtype)
        if src.shape[-1:] != (5,):
            raise ValueError(f"boxes {src.shape}: the last axis must be (cx, cy, w, h, angle)")
        b = src.astype(np.float64)
        with np.errstate(invalid="ignore", over="ignore"):
            a = b[..., 4] + float(theta)
            a = a - 360.0 * np.floor((a + 180.0) / 360.0)
            out = np.stack([m[0] * b[..., 0] + m[1] * b[..., 1] + m[2], m[3] * b[..., 0] + m[4] * b[..., 1] + m[5],
                            b[..., 2], b[..., 3], a], axis=-1).astype(dtype)
        keep = ~np.isfinite(src).all(axis=-1)
        out[keep] = src[keep]                      # same dtype: the bits as they are
        return out

    def apply_rotated_boxes(self, boxes) -> np.ndarray:
        """rotated boxes of the original image -> the rotated image"""
        return self.map_rotated_boxes(boxes, self.inverse_matrix, self.angle)

    def inverse_rotated_boxes(self, boxes) -> np.ndarray:
        """rotated boxes of the rotated image -> the original image (the angle subtracts)"""
        return self.map_rotated_boxes(boxes, self.matrix, -self.angle)

    def __repr__(self) -> str:
        return f"RotationTransform(h={self.h}, w={self.w}, angle={self.angle!r})"


def check_fill(fill) -> Tuple[int, int, int]:
    """three integers in 0..255 (ValueError otherwise)"""
    try:
        f = tuple(fill)
        ok = len(f) == 3 and all(float(v) == int(v) and 0 <= int(v) <= 255 for v in f)
    except (TypeError, ValueError, OverflowError):
        ok = False
    if not ok:
        raise ValueError(f"fill {fill!r}: needs three integers in 0..255")
    return tuple(int(v) for v in f)


def rotate_u8_host(img: np.ndarray, angle, fill=(0, 0, 0)) -> np.ndarray:
    """`PIL.Image.fromarray(img).rotate(angle, BILINEAR, expand=True, fillcolor=fill)` of a uint8 HWC RGB image in numpy
    float64, byte for byte (tests/test_rotate.py); `angle` may be a RotationTransform of the image's size.  For an output
    pixel (x, y): (xin, yin) = matrix applied to (x + 0.5, y + 0.5); outside [0, w) x [0, h) (or not a number) the fill;
    otherwise PIL's bilinear filter around (xin - 0.5, yin - 0.5) with clipped neighbours, v1 + (v2 - v1) * dy truncated.
    Every product and sum is rounded on its own (no fused multiply-add)."""
    img = np.asarray(img)
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3:
        raise ValueError(f"expected a uint8 HWC image with 3 channels, got {img.dtype} {img.shape}")
    fill = check_fill(fill)
    h, w = img.shape[:2]
    t = angle if isinstance(angle, RotationTransform) else RotationTransform(h, w, angle)
    if (t.h, t.w) != (h, w):
        raise ValueError(f"{t!r} on a {h}x{w} image")
    if t.kind < 4:
        return np.ascontiguousarray(np.rot90(img, t.kind))
    m = t.matrix
    Ho, Wo = t.out_hw
    xc = (np.arange(Wo, dtype=np.float64) + 0.5)[None, :]
    yc = (np.arange(Ho, dtype=np.float64) + 0.5)[:, None]
    with np.errstate(invalid="ignore", over="ignore"):
        xin = m[0] * xc + m[1] * yc + m[2]
        yin = m[3] * xc + m[4] * yc + m[5]
    inside = (xin >= 0.0) & (xin < w) & (yin >= 0.0) & (yin < h)
    xin = np.where(inside, xin, 0.5) - 0.5
    yin = np.where(inside, yin, 0.5) - 0.5
    x0 = np.floor(xin)
    y0 = np.floor(yin)
    dx = (xin - x0)[..., None]
    dy = (yin - y0)[..., None]
    x0 = x0.astype(np.int64)
    y0 = y0.astype(np.int64)
    xa, xb = np.clip(x0, 0, w - 1), np.clip(x0 + 1, 0, w - 1)
    ya = np.clip(y0, 0, h - 1)
    src = img.astype(np.float64)
    a, b = src[ya, xa], src[ya, xb]
    v1 = a + (b - a) * dx
    below = (y0 + 1 >= 0) & (y0 + 1 < h)
    yb = np.where(below, y0 + 1, ya)
    a, b = src[yb, xa], src[yb, xb]
    v2 = np.where(below[..., None], a + (b - a) * dx, v1)
    v = v1 + (v2 - v1) * dy
    out = np.where(inside[..., None], v.astype(np.uint8), np.array(fill, dtype=np.uint8))
    return np.ascontiguousarray(out.astype(np.uint8))
