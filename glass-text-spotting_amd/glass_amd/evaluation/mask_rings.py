"""`masks_to_polygons` on the device: the pasted instance masks (`pred_masks`, bool [R, H, W]) become polygons without
leaving the GPU (csrc/mask_rings.hip through ops.native.mask_rings; reference glass/evaluation/text_evaluator.py:464-492).
The host tracer `text_evaluator.masks_to_polygons` is the definition: same regions, same rings, vertex for vertex.
`from_rois` gives the same rings from the RoI masks and their boxes (`pred_mask_rois` / `pred_mask_boxes`,
MODEL.ROI_MASK_HEAD.PASTE_MASKS False), without the pasted tensor (ops.native.roi_mask_rings)."""
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
        return self._rings(*native.mask_rings(masks))

    @staticmethod
    def _rings(xy, ring_off) -> list:
        pts = xy.cpu().numpy().astype(np.float64)
        off = ring_off.cpu().tolist()
        return [pts[a:b].tolist() for a, b in zip(off[:-1], off[1:])]

    def from_rois(self, masks, boxes, image_hw, threshold=0.5) -> list:
        """The rings `__call__` returns for `paste_rotated_masks(masks, boxes, image_hw, threshold)`, from the RoI masks
        themselves (float [R, M, M] probabilities, `pred_mask_rois`) and the boxes they were predicted in ([R, 5], image pixels,
        `pred_mask_boxes`): the pasted [R, H, W] tensor is never made (ops.native.roi_mask_rings).  Host tensors / numpy arrays
        are uploaded."""
        from ..ops import native
        as_dev = lambda t: (t if isinstance(t, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(t))).to(
            self.device, torch.float32).contiguous()
        masks, boxes = as_dev(masks), as_dev(boxes)
        return self._rings(*native.roi_mask_rings(masks, boxes, (int(image_hw[0]), int(image_hw[1])), threshold))
