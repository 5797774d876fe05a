"""`masks_to_polygons` on the device: the pasted instance masks (`pred_masks`, bool [R, H, W]) become polygons without
leaving the GPU (csrc/mask_rings.hip through ops.native.mask_rings; reference glass/evaluation/text_evaluator.py:464-492).
The host tracer `text_evaluator.masks_to_polygons` is the definition: same regions, same rings, vertex for vertex.
`from_rois` gives the same rings from the RoI masks and their boxes (`pred_mask_rois` / `pred_mask_boxes`,
MODEL.ROI_MASK_HEAD.PASTE_MASKS False), without the pasted tensor (ops.native.roi_mask_rings)."""
from __future__ import annotations

import numpy as np
import torch

from .ring_simplify import tolerance_q4


class MaskPolygonizer:
    """Callable for `TextResultWriter(..., masks_to_polygons=MaskPolygonizer(device))` / `instances_to_coco_json`:
    masks (a bool / uint8 device tensor [R, H, W], or a host tensor / numpy array, which is uploaded) -> what
    `masks_to_polygons` returns, one closed ring [[x, y], ...] of floats per mask, [] for an empty mask.
    `takes_device_tensor` tells `instances_to_coco_json` to hand over `pred_masks` as it is instead of a numpy copy.
    `simplify`: None (the traced rings, as ever) or a tolerance in pixels, a multiple of 1/4 in [0, 1024]: the rings are then
    simplified on the device before the download (ops.native.simplify_rings; the statement is `simplify_ring`, exact
    Douglas-Peucker), and only the simplified vertices cross to the host.  `keep_valid` (with `simplify` only): the simplified
    rings are checked on the device by the rule of `normalize_detection_line` (ops.native.ring_check: fewer than 3 points, zero
    area, two properly crossing sides); a ring that fails while its traced form passes is returned as traced, so switching
    `simplify` on never removes a detection the unsimplified path would have scored.  `restored` counts those rings."""

    takes_device_tensor = True

    def __init__(self, device=None, simplify=None, keep_valid=True):
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        if simplify is not None:
            tolerance_q4(simplify)                                     # ValueError now, not at the first image
        self.simplify, self.keep_valid = simplify, bool(keep_valid)
        self.restored = 0                                              # rings `keep_valid` has returned unsimplified so far

    def __call__(self, masks) -> list:
        from ..ops import native
        if not isinstance(masks, torch.Tensor):
            masks = torch.from_numpy(np.ascontiguousarray(masks))
        if masks.dtype not in (torch.bool, torch.uint8):
            masks = masks != 0
        masks = masks.to(self.device).contiguous()
        return self._rings(*native.mask_rings(masks))

    def _rings(self, xy, ring_off) -> list:
        if self.simplify is not None:
            return self._simplified(xy, ring_off)
        pts = xy.cpu().numpy().astype(np.float64)
        off = ring_off.cpu().tolist()
        return [pts[a:b].tolist() for a, b in zip(off[:-1], off[1:])]

    def _simplified(self, xy, ring_off) -> list:
        """The rings of (xy, ring_off), device tensors of a tracer, simplified on the device; with `keep_valid` a ring whose
        simplified form `normalize_detection_line` would drop while it keeps the traced form is returned as traced."""
        from ..ops import native
        xy_s, off_s = native.simplify_rings(xy, ring_off, self.simplify)
        R = int(ring_off.shape[0]) - 1
        both = torch.cat([off_s, ring_off]).cpu().tolist()             # one download for both offset tables
        off, off_t = both[:R + 1], both[R + 1:]
        pts = xy_s.cpu().numpy().astype(np.float64)
        rings = [pts[a:b].tolist() for a, b in zip(off[:-1], off[1:])]
        if not self.keep_valid or R == 0:
            return rings
        verdict = native.ring_check(xy_s, off)[0].cpu().numpy()
        bad = [r for r in np.nonzero(verdict == 0)[0].tolist() if off_t[r + 1] > off_t[r]]      # an empty ring stays empty
        if not bad:
            return rings
        # the traced form of those rings only: gathered on the device, checked there, downloaded
        traced = torch.cat([xy[off_t[r]:off_t[r + 1]] for r in bad])
        t_off = np.concatenate([[0], np.cumsum([off_t[r + 1] - off_t[r] for r in bad])])
        t_verdict = native.ring_check(traced, t_off)[0].cpu().numpy()
        t_pts = traced.cpu().numpy().astype(np.float64)
        for k, r in enumerate(bad):
            if t_verdict[k] != 0:
                rings[r] = t_pts[t_off[k]:t_off[k + 1]].tolist()
                self.restored += 1
        return rings

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
