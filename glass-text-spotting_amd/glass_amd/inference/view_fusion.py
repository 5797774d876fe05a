"""The view plan of fused multi-view inference (GlassRunner.run_views): an image shown to the model at several rotations and
scales, and for each view the eight doubles with which ops.native.fuse_views (glass_fuse_views,
include/glass_hip_feature_fuse.h) brings its detections back to the image's frame.  Pure Python and numpy: no device.

A view of angle `angle` and scale `scale` is the image rotated as `PIL.Image.rotate(angle, expand=True)` rotates it
(data.transforms.RotationTransform, ops.native.rotate_u8) and then resized by rho = scale * ratio_of(rotated size), where
`ratio_of` is the runner's own resize policy - so a scale of 1.0 is what `GlassRunner.__call__` would feed for the rotated
image.  A pixel p of the view is the pixel p / rho of the rotated image, and M = rotation.matrix maps that to the original
(the rotated-to-original matrix run_rotated passes with inverse=True), so the row is

    (M0 / rho, M1 / rho, M2, M3 / rho, M4 / rho, M5, 1 / rho, -angle)

: the matrix of view pixel -> image pixel, the image pixels per view pixel, and the degrees to add to a box angle (the
angle reduced mod 360, `rotation.angle`, as run_rotated passes it).
"""
from __future__ import annotations

import math
from typing import Callable, List, NamedTuple, Sequence, Tuple

from ..data.transforms import RotationTransform

MAX_VIEWS = 64       # ops.native.FUSE_VIEWS_MAX_VIEWS: a view is a bit of the 64-bit view mask


class View(NamedTuple):
    angle: float                 # degrees counter-clockwise, as given
    scale: float                 # as given
    rotation: RotationTransform
    rho: float                   # view pixels per pixel of the rotated image
    affine: Tuple[float, ...]    # m0..m5, s, dtheta


def plan_views(height: int, width: int, angles: Sequence[float], scales: Sequence[float],
               ratio_of: Callable[[Tuple[int, int]], float]) -> List[View]:
    """the views of a height x width image, angle-major and scale-minor.  ValueError for an empty or non-finite list, a scale
    <= 0, two views of one (angle mod 360, scale) and more than 64 views."""
    try:
        angles, scales = [float(a) for a in angles], [float(s) for s in scales]
    except TypeError as e:
        raise ValueError(f"plan_views: angles and scales must be sequences of numbers ({e})") from None
    if not angles or not scales:
        raise ValueError(f"plan_views: angles={angles} scales={scales}: neither may be empty")
    if not all(math.isfinite(a) for a in angles) or not all(math.isfinite(s) for s in scales):
        raise ValueError(f"plan_views: angles={angles} scales={scales}: every value must be finite")
    if any(s <= 0 for s in scales):
        raise ValueError(f"plan_views: scales={scales}: every scale must be > 0")
    pairs = [(a % 360.0, s) for a in angles for s in scales]
    if len(set(pairs)) != len(pairs):
        raise ValueError(f"plan_views: angles={angles} scales={scales}: two views of one (angle mod 360, scale)")
    if len(pairs) > MAX_VIEWS:
        raise ValueError(f"plan_views: {len(pairs)} views (at most {MAX_VIEWS})")
    views = []
    for angle in angles:
        rotation = RotationTransform(height, width, angle)
        ratio = float(ratio_of(rotation.out_hw))
        if not (ratio > 0 and math.isfinite(ratio)):
            raise ValueError(f"plan_views: ratio_of({rotation.out_hw}) = {ratio}")
        m = rotation.matrix
        for scale in scales:
            rho = scale * ratio
            views.append(View(angle, scale, rotation, rho,
                              (m[0] / rho, m[1] / rho, m[2], m[3] / rho, m[4] / rho, m[5], 1.0 / rho, -rotation.angle)))
    return views
