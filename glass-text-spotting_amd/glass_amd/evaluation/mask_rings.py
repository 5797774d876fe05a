"""`masks_to_polygons` on the device: the pasted instance masks (`pred_masks`, bool [R, H, W]) become polygons without
leaving the GPU (csrc/mask_rings.hip through ops.native.mask_rings; reference glass/evaluation/text_evaluator.py:464-492).
The host tracer `text_evaluator.masks_to_polygons` is the definition: same regions, same rings, vertex for vertex."""
from __future__ import annotations

import numpy as np
import torch


class MaskPolygonizer:
    """Callable for `TextResultWriter(..., masks_to_polygons=MaskPolygonizer(device))` / `instances_to_coco_json`:
    masks (a bool / uint8 device tensor [R, H, W], or a host tensor / numpy array, which is uploaded) -> what
    `masks_to_polygons` returns, one closed ring [[x, y], ...] of floats per mask, [] for an empty mask.
    `takes_device_tensor` tells `instances_to_coco_json` to hand over `pred_masks` as it is instead of a numpy copy."""

    takes_device_tensor = True

    def __init__(self, device=None):
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())

    def __call__(self, masks) -> list:
        from ..ops import native
        if not isinstance(masks, torch.Tensor):
            masks = torch.from_numpy(np.ascontiguousarray(masks))
        if masks.dtype not in (torch.bool, torch.uint8):
            masks = masks != 0
        masks = masks.to(self.device).contiguous()
        xy, ring_off = native.mask_rings(masks)
        pts = xy.cpu().numpy().astype(np.float64)
        off = ring_off.cpu().tolist()
        return [pts[a:b].tolist() for a, b in zip(off[:-1], off[1:])]
