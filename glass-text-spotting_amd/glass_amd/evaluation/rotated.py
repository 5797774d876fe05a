"""Rotated-image evaluation: the protocol of the Rotated ICDAR13 sets (reference glass/evaluation/text_evaluator.py:63-70 names
`icdar2013_r45` / `icdar2013_r60`, which were distributed as pre-rotated files) built here from unrotated data: the mapper
rotates every image as `PIL.Image.rotate(angle, BILINEAR, expand=True)` does (data.DatasetMapper(rotate=...)), the ground
truth goes through the same matrix (`rotate_ground_truth`), and `rotation_sweep` scores one run per angle.  The published
files' bytes (another library, a lossy format) are not reproduced; the construction is."""
from __future__ import annotations

import math
import os
import re
from collections import OrderedDict
from typing import Callable, Dict, Mapping, Optional, Sequence, Tuple

from ..data.transforms import RotationTransform

MAX_COORDINATE = 1 << 20        # a rotated ground-truth coordinate beyond this is a mistake in the sizes, not a text


def rotate_ground_truth(gt: Mapping[str, Tuple[Sequence[Sequence[int]], Sequence[str]]], sizes: Mapping[str, Tuple[int, int]],
                        angle: float) -> "OrderedDict[str, Tuple[list, list]]":
    """`gt` as `load_gt_zip` returns it ({key: (rings, transcriptions)}, a ring = [x1, y1, ..., xn, yn]) -> the same for the
    images rotated by `angle`: every ring goes through `RotationTransform(h, w, angle).apply_coords` with (h, w) = sizes[key]
    and every coordinate becomes floor(v + 0.5) as a Python int (RRCScorer takes integers).  Vertex order and transcriptions
    are kept.  A key without a size is a KeyError naming it; a coordinate beyond 2^20 in magnitude is a ValueError."""
    out = OrderedDict()
    for key, (rings, texts) in gt.items():
        if key not in sizes:
            raise KeyError(f"rotate_ground_truth: no image size for ground-truth sample {key!r}")
        h, w = sizes[key]
        t = RotationTransform(h, w, angle)
        moved = []
        for ring in rings:
            if len(ring) % 2:
                raise ValueError(f"rotate_ground_truth: sample {key!r}: a ring of {len(ring)} numbers")
            q = t.apply_coords([[float(ring[i]), float(ring[i + 1])] for i in range(0, len(ring), 2)]) if len(ring) else []
            flat = [int(math.floor(float(v) + 0.5)) for p in q for v in p]
            if any(abs(v) > MAX_COORDINATE for v in flat):
                raise ValueError(f"rotate_ground_truth: sample {key!r}: a rotated coordinate beyond 2^20 (image {h}x{w}, "
                                 f"angle {angle})")
            moved.append(flat)
        out[key] = (moved, list(texts))
    return out


def default_key_of(dataset_dict: Dict) -> str:
    """the last run of digits in the basename of the dict's "file_name" (img_12.jpg -> "12"), the key of both gt.zip layouts"""
    runs = re.findall(r"\d+", os.path.basename(str(dataset_dict["file_name"])))
    if not runs:
        raise ValueError(f"no digits in the file name {dataset_dict['file_name']!r}: pass key_of")
    return runs[-1]


def rotation_sweep(model, dataset_dicts: Sequence[Dict], mapper, writer, gt, angles: Sequence[float],
                   key_of: Optional[Callable[[Dict], str]] = None, word_spotting: bool = False, device=None,
                   text_cf_th: float = 0.5, detection_cf_th: float = 0.0, **driver_kwargs) -> "OrderedDict[float, dict]":
    """"How does hmean fall with the angle": one evaluation run per angle of `angles` -> OrderedDict{angle: results}, the
    results as `TextResultWriter.evaluate` returns them.  Each run sets `mapper.rotate`, resets `writer`, runs
    `inference_on_dataset(model, dataset_dicts, mapper, writer, **driver_kwargs)` (the model and the writer see the rotated
    images, as with the pre-rotated files of the protocol) and scores against `rotate_ground_truth(gt, sizes, angle)` with an
    `RRCScorer` on `device` (default: the mapper's).  `gt`: what `load_gt_zip` returns; `key_of`: dataset dict -> its key in
    `gt` (default `default_key_of`); the sizes are the unrotated images' as the mapper decoded them.  Angle 0 takes the
    untouched path: no rotation, the ground truth as given.  `mapper.rotate` is put back afterwards, also on an exception."""
    from .driver import inference_on_dataset
    from .rrc_score import RRCScorer
    key_of = key_of or default_key_of
    device = device if device is not None else mapper.device
    results = OrderedDict()
    before = mapper.rotate
    try:
        for angle in angles:
            sizes: Dict[str, Tuple[int, int]] = {}

            def mapped(dd, _sizes=sizes):
                out = mapper(dd)
                rot = out.get("rotation")
                if rot is not None:
                    _sizes[key_of(dd)] = (rot.h, rot.w)
                return out

            mapper.rotate = mapper.check_rotate(angle)
            writer.reset()
            inference_on_dataset(model, dataset_dicts, mapped, writer, **driver_kwargs)
            gt_a = gt if mapper.rotate == 0.0 else rotate_ground_truth(gt, sizes, angle)
            scorer = RRCScorer(gt_a, word_spotting, device)
            results[angle] = writer.evaluate(scorer, text_cf_th, detection_cf_th)
    finally:
        mapper.rotate = before
    return results
