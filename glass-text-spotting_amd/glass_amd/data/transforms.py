"""Test-time image transform of the evaluation protocol: detectron2's `ResizeShortestEdge` on a uint8 image, which is
`PIL.Image.resize(..., BILINEAR)` [d2-recall: detectron2 v0.6 data/transforms/augmentation_impl.py ResizeShortestEdge,
transform.py ResizeTransform.apply_image; detectron2 is not vendored in the reference], stated in numpy.

`pil_bilinear_coeffs` makes the per-axis tables the device kernels (csrc/resize_pil.hip) read; `pil_resize_u8_host` is the
readable form of the whole resize and the cross-check of the kernels, byte for byte equal to PIL (tests/test_resize_pil.py).
"""
from __future__ import annotations

import functools
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
