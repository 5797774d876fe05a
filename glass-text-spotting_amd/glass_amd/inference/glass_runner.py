"""`GlassRunner`: the single-image predictor the reference ships, on the HIP pipeline.

`run_tiled` is the large-image form: overlapping tiles at full resolution as one batch, merged on the device.
`run_views` is test-time augmentation: rotated and rescaled views of one image, fused on the device.

Mirrors reference glass/inference/glass_runner.py:20-153: cfg set-up (:31-39), model build and
checkpoint load (:52-60), channel handling (:83-87), on-device bilinear resize policy
(`get_inference_scale_ratio` :111-121, `_image_to_tensor` :123-148), model call (:93-96),
un-scaling of boxes (:100-102) and post-processing (:106).
`run_batch` is the throughput form: many images per step, identical per-image results.
"""
from __future__ import annotations

import logging
from typing import List, Optional, Sequence

import numpy as np
import torch

from ..config import get_glass_cfg
from ..modeling.meta_arch.glass_rcnn import build_model
from ..modeling.recognition.text_encoder import TextEncoder
from ..ops import native as K
from ..postprocess import build_post_processor
from ..structures.core import Instances, RotatedBoxes
from ..utils.host import limit_host_threads
from .tiling import plan_tiles


def _char_boxes_on(model) -> bool:
    """MODEL.ROI_RECOGNIZER_HEAD.CHAR_BOXES of the model's recogniser head (a model without one: off)"""
    return bool(getattr(getattr(getattr(model, "roi_heads", None), "recognizer_head", None), "char_boxes", False))


class GlassRunner:
    def __init__(self, model_path: Optional[str], config_path: Optional[str], opts: List[str] = None, post_process=True,
                 cfg=None, state_dict=None):
        self.logger = logging.getLogger(__name__)
        limit_host_threads()                                  # utils/host.py: the host side is launch glue
        self.cfg = (cfg if cfg is not None else get_glass_cfg(config_path, opts)).clone()
        self.model_path, self.config_path, self.post_process_flag = model_path, config_path, post_process
        self.model = build_model(self.cfg)
        self.model.eval()
        self.device = self.model.device
        if state_dict is not None:
            self.model.load_state_dict(state_dict)
        elif model_path:
            self.model.load_checkpoint(model_path)
        self.min_target_size = self.cfg.INPUT.MIN_SIZE_TEST
        self.max_target_size = self.cfg.INPUT.MAX_SIZE_TEST
        self.max_upscale_ratio = self.cfg.INPUT.MAX_UPSCALE_RATIO
        self.input_format = self.cfg.INPUT.FORMAT
        assert self.input_format in ["RGB", "BGR", "GREY"], self.input_format
        self.text_encoder = TextEncoder(self.cfg)
        self.post_processor = build_post_processor(self.cfg)

    def get_inference_scale_ratio(self, image_shape):
        height, width = image_shape[:2]
        m = max(height, width)
        if m > self.max_target_size:
            return self.max_target_size / m
        if m < self.min_target_size:
            return min(self.max_upscale_ratio, self.min_target_size / m)
        return 1

    def _image_to_tensor(self, original_image: np.ndarray):
        """uint8 HWC on host -> float CHW on device, resized by the reference policy; one H2D copy
        of the uint8 image and one fused convert+resize kernel."""
        scale_ratio = self.get_inference_scale_ratio(original_image.shape)
        return self._image_at_scale(original_image, scale_ratio), scale_ratio

    def _grey(self, original_image: np.ndarray) -> np.ndarray:
        if self.input_format == "GREY":
            # reference glass/utils/common_utils.py:29-43 (rgb2grey, three_channels=True), on the host uint8 image as
            # the reference does: Y'709 weights on channels 0,1,2, truncated to uint8, replicated three times
            g = np.uint8(0.2125 * original_image[:, :, 0] + 0.7154 * original_image[:, :, 1] + 0.0721 * original_image[:, :, 2])
            original_image = np.repeat(g[:, :, None], 3, axis=2)
        return original_image

    def _image_at_scale(self, original_image, scale_ratio):
        """the device image `_image_to_tensor` makes, at a ratio of the caller's choice.  A uint8 HWC tensor already on the
        device (run_rotated's rotated image: converted to grey before it was uploaded) skips the conversion and the upload."""
        if isinstance(original_image, torch.Tensor):
            u8 = original_image
        else:
            u8 = torch.from_numpy(np.ascontiguousarray(self._grey(original_image))).to(self.device)
        height, width = (int(v) for v in u8.shape[:2])
        if scale_ratio != 1:
            nh, nw = int(np.round(scale_ratio * height)), int(np.round(scale_ratio * width))
        else:
            nh, nw = height, width
        return K.image_u8hwc_to_chw(u8, (nh, nw), flip_channels=(self.input_format == "RGB"))

    @staticmethod
    def _scaled_boxes(boxes: torch.Tensor, scale_xy: torch.Tensor) -> torch.Tensor:
        """padded boxes [N, K, 5] times the per-image (sx, sy) [N, 2].  The runner only scales uniformly (sx == sy): centre and
        extents are multiplied (one float32 product each), the angle is kept."""
        sx, sy = scale_xy[:, None, 0:1], scale_xy[:, None, 1:2]
        return torch.cat([boxes[..., 0:1] * sx, boxes[..., 1:2] * sy, boxes[..., 2:3] * sx, boxes[..., 3:4] * sy, boxes[..., 4:5]], -1)

    def run_batch(self, images: Sequence[np.ndarray]) -> List[Instances]:
        """Many images per step with per-image results identical to image-by-image calls.  detectron2
        pads a batch to its largest image and the pad region is visible to the backbone/RPN, so images
        are grouped by their own padded shape (multiple of 32) and each group is one model call."""
        inputs, ratios, shapes = [], [], []
        for im in images:
            t, r = self._image_to_tensor(im)
            inputs.append({"image": t, "height": t.shape[1], "width": t.shape[2]})
            ratios.append(r)
            shapes.append(tuple(int(v) for v in im.shape[:2]))
        d = self.model.backbone.size_divisibility
        groups = {}
        for i, inp in enumerate(inputs):
            key = ((inp["height"] + d - 1) // d * d, (inp["width"] + d - 1) // d * d)
            groups.setdefault(key, []).append(i)
        out = [None] * len(inputs)
        for idxs in groups.values():
            raw = self.model([inputs[i] for i in idxs])
            det = getattr(raw, "batch", None)          # this call's padded device-resident batch (pipeline.StepOutput)
            if self.post_process_flag and det is not None:
                # un-scale + the whole word post-processing for the group in one kernel (no per-image host loop)
                if det.text is None and sum(det.counts_host) > 0:
                    raise RuntimeError("recognizer output missing")
                sc = torch.tensor([[1.0 / ratios[i], 1.0 / ratios[i]] for i in idxs], dtype=torch.float32).to(self.device)
                text = det.text
                if text is None:          # no detections in the whole group
                    T = self.cfg.MODEL.ROI_RECOGNIZER_HEAD.MAX_WORD_LENGTH + 1
                    C = len(self.cfg.MODEL.ROI_RECOGNIZER_HEAD.CHARACTER_SET) + 2
                    text = torch.zeros(tuple(det.scores.shape) + (T, C), dtype=torch.float32, device=self.device)
                # (BEAM_DISTRIBUTIONS: the full distribution rows are gathered with the survivors, like the orientations)
                extra = {"orientations": det.orient, "pred_text_dist": getattr(det, "text_dist", None)}
                rois = getattr(det, "mask_rois", None)
                if rois is not None:
                    # MODEL.ROI_MASK_HEAD.PASTE_MASKS False: the mask rows ride along with the boxes they were predicted in,
                    # scaled to the original image's pixels (the masks' frame; pred_boxes may be enlarged by the merge step)
                    extra["pred_mask_rois"] = rois
                    extra["pred_mask_boxes"] = self._scaled_boxes(det.boxes, sc)
                chars = getattr(det, "chars", None)
                if _char_boxes_on(self.model):
                    # MODEL.ROI_RECOGNIZER_HEAD.CHAR_BOXES: the (normalised) character rows ride along like the distributions, with
                    # the boxes the recogniser pooled, scaled to the original image's pixels, as their frame (pred_boxes may be
                    # enlarged by the merge step; the characters' frame stays)
                    from ..postprocess.char_boxes import unpack_chars
                    if chars is None:     # no detections in the whole group
                        chars = torch.zeros(tuple(det.scores.shape) + (text.shape[2] + 1, 3), dtype=torch.float32, device=self.device)
                    extra.update(unpack_chars(chars))
                    extra["pred_char_frames"] = self._scaled_boxes(det.boxes, sc)
                res = self.post_processor.process_padded(det.boxes, det.scores, det.counts_dev, text, sc, [shapes[i] for i in idxs],
                                                         extra)
                for i, r in zip(idxs, res):
                    out[i] = r
            else:
                for i, res in zip(idxs, raw):
                    preds = res["instances"]
                    if ratios[i] != 1:
                        preds.pred_boxes.scale(1 / ratios[i], 1 / ratios[i])
                        if preds.has("pred_mask_boxes"):
                            # PASTE_MASKS False: the masks' frame follows pred_boxes into the original image's pixels (no word
                            # post-processing on this path, so the two are the same boxes)
                            preds.pred_mask_boxes = preds.pred_boxes.tensor.clone()
                        if preds.has("pred_char_frames"):        # CHAR_BOXES: the same for the characters' frame
                            preds.pred_char_frames = preds.pred_boxes.tensor.clone()
                    preds._image_size = tuple(shapes[i])
                    out[i] = preds
        for r in out:
            self.logger.info(f"Post-processing output is {len(r)} word instances")
        return out

    def run_tiled(self, image: np.ndarray, tile: int = 1024, overlap: int = 256, border: int = 16, scale: float = 1.0,
                  full_view: bool = True, nms_thresh: Optional[float] = None, batch_size: int = 8,
                  merge_case: Optional[bool] = None) -> Instances:
        """One large image at (`scale` times) its own resolution: `__call__` shrinks an image whose long side exceeds
        INPUT.MAX_SIZE_TEST, and the small words of a scan or a receipt are gone before the RPN sees them.  Here the image is cut
        into overlapping tiles (tiling.plan_tiles) that run through the model as batches of at most `batch_size`; with
        `full_view`, the input `__call__` would feed runs as one more view, for the words too large to lie whole in a tile.
        ops.native.merge_views (glass_merge_views) makes ONE detection set of them on the device: a tile's word counts if its
        corners keep `border` pixels from the tile's interior edges and (with the full view) its extent is at most
        L = overlap - 2*border, a word of the full view if its extent is above L, and of the copies of a word that several views
        hold the best-scored one stays (rotated IoU >= `nms_thresh`, default MODEL.ROI_HEADS.NMS_THRESH_TEST, between boxes of
        different views).  The merged set - at most 1024 detections - then takes the ordinary way through the word
        post-processor, with the boxes in the original image's pixels.
        `merge_case` (None: the recogniser head's own setting): run every view with the head's pattern searched fold-merged
        (True) or unmerged (False) - `RecognizerRCNNHeadV3.set_pattern(merge_case=...)` for this call only; ValueError if the
        head has no pattern."""
        heads = self.model.roi_heads
        if _char_boxes_on(self.model):
            raise NotImplementedError("run_tiled: MODEL.ROI_RECOGNIZER_HEAD.CHAR_BOXES is on; the character rows are not carried "
                                      "through the cross-tile merge (use run_batch, or switch the key off)")
        if merge_case is not None:
            head = getattr(heads, "recognizer_head", None)
            if getattr(head, "pattern", None) is None:
                raise ValueError("run_tiled: merge_case needs a pattern on the recogniser head (set_pattern, or "
                                 "set_lexicon(trie, merge_case=True))")
            before = head.merge_case
            head.merge_case = bool(merge_case)
            try:
                return self.run_tiled(image, tile, overlap, border, scale, full_view, nms_thresh, batch_size)
            finally:
                head.merge_case = before
        with_masks = bool(getattr(heads, "mask_inference", False))
        if with_masks and getattr(self.model, "paste_masks", True):
            raise NotImplementedError("run_tiled: MODEL.ROI_MASK_HEAD.MASK_INFERENCE is on and the masks are pasted per tile frame, "
                                      "which cannot be merged; set MODEL.ROI_MASK_HEAD.PASTE_MASKS False to carry the RoI masks "
                                      "(pred_mask_rois / pred_mask_boxes) instead")
        if getattr(getattr(heads, "recognizer_head", None), "image_segments", None) is not None:
            raise NotImplementedError("run_tiled: the recogniser head carries per-image lexicon segments (image_segments); the "
                                      "views of a tiled image are not images of that list - set the lexicon with one segment "
                                      "(the same holds for a pattern's segments)")
        height, width = image.shape[:2]
        scale = float(scale)
        if not (scale > 0 and np.isfinite(scale)):
            raise ValueError(f"run_tiled: scale={scale}")
        work = self._image_at_scale(image, scale if scale != 1.0 else 1)
        plan = plan_tiles(work.shape[1], work.shape[2], tile, overlap, border)
        L = float(plan.max_whole)
        inf = float("inf")
        with_full = bool(full_view) and len(plan.tiles) > 1
        Kdet = int(self.cfg.TEST.DETECTIONS_PER_IMAGE)
        V = len(plan.tiles) + int(with_full)
        if V * Kdet > K.MERGE_VIEWS_MAX_SLOTS or V > K.MERGE_VIEWS_MAX_VIEWS:
            fit = tile
            while fit < (1 << 20):
                fit += 32
                p = plan_tiles(work.shape[1], work.shape[2], fit, overlap, border)
                n = len(p.tiles) + int(bool(full_view) and len(p.tiles) > 1)
                if n * Kdet <= K.MERGE_VIEWS_MAX_SLOTS and n <= K.MERGE_VIEWS_MAX_VIEWS:
                    break
            raise ValueError(f"run_tiled: {V} views of {Kdet} detections each exceed the {K.MERGE_VIEWS_MAX_SLOTS} slots (and "
                             f"{K.MERGE_VIEWS_MAX_VIEWS} views) of one merge; tile={fit} fits this image")
        # ---- the views: (input, frame transform, keep rectangle, size band)
        inputs, xform, keep, band = [], [], [], []
        for t in plan.tiles:
            crop = work[:, t.y0:t.y0 + t.h, t.x0:t.x0 + t.w]
            inputs.append({"image": crop, "height": t.h, "width": t.w})
            xform.append([float(t.x0), float(t.y0), 1.0])
            keep.append(list(t.keep))
            band.append([-inf, L if with_full else inf])       # (one tile has no full view beside it: it keeps every size)
        calls = [inputs[i:i + max(int(batch_size), 1)] for i in range(0, len(inputs), max(int(batch_size), 1))]
        if with_full:
            full, rho = self._image_to_tensor(image)
            calls.append([{"image": full, "height": full.shape[1], "width": full.shape[2]}])
            xform.append([0.0, 0.0, scale / rho])
            keep.append([-inf, -inf, inf, inf])
            band.append([L, inf])
        # ---- the model, call by call; the padded device batches joined along the view axis
        dets = []
        for call in calls:
            det = getattr(self.model(call), "batch", None)
            if det is None:
                raise RuntimeError("run_tiled needs the model's padded device batch (POST_PROCESSING.INFLATE_RATIO / DROP_OVERLAPPING "
                                   "take the list-wise path, which has none)")
            if tuple(det.scores.shape) != (len(call), Kdet):
                raise RuntimeError(f"run_tiled: a batch of scores {tuple(det.scores.shape)}, expected {(len(call), Kdet)}")
            dets.append(det)
        dev = self.device

        def joined(name, tail):
            parts = [getattr(d, name, None) for d in dets]
            if all(p is None for p in parts):
                return None
            return torch.cat([p if p is not None else torch.zeros((d.scores.shape[0], Kdet) + tail, dtype=torch.float32, device=dev)
                              for p, d in zip(parts, dets)], 0)
        T = self.cfg.MODEL.ROI_RECOGNIZER_HEAD.MAX_WORD_LENGTH + 1
        C = len(self.cfg.MODEL.ROI_RECOGNIZER_HEAD.CHARACTER_SET) + 2
        boxes, scores = joined("boxes", (5,)), joined("scores", ())
        orient, text, text_dist = joined("orient", (2,)), joined("text", (T, C)), joined("text_dist", (T, C))
        counts = torch.cat([d.counts_dev for d in dets], 0)
        if text is None and sum(sum(d.counts_host) for d in dets) > 0:
            raise RuntimeError("recognizer output missing")
        # PASTE_MASKS False: the views' mask rows [n, K, M, M] (a call without a detection has none: zeros in its place)
        rois = None
        if with_masks:
            have = [d.mask_rois for d in dets if getattr(d, "mask_rois", None) is not None]
            rois = joined("mask_rois", tuple(have[0].shape[2:])) if have else None
        # ---- the merge, and the survivors' rows gathered by their source slot
        thr = float(nms_thresh or self.cfg.MODEL.ROI_HEADS.NMS_THRESH_TEST)
        m = K.merge_views(boxes.contiguous(), scores.contiguous(), counts.contiguous(), K.upload(xform, torch.float32, dev),
                          K.upload(keep, torch.float32, dev), K.upload(band, torch.float32, dev), thr, K.MERGE_VIEWS_MAX_OUT)
        src = m["src"].long()
        gather = lambda t: None if t is None else t.reshape((V * Kdet,) + tuple(t.shape[2:])).index_select(0, src).unsqueeze(0)
        orient, text, text_dist, rois = gather(orient), gather(text), gather(text_dist), gather(rois)
        n_out, truncated = m["count"].tolist()                      # the one read of out_count
        if truncated:
            self.logger.warning(f"run_tiled: more than {K.MERGE_VIEWS_MAX_OUT} merged detections; the lowest-scored are cut off")
        if self.post_process_flag:
            if text is None:          # no detections in any view
                text = torch.zeros((1, K.MERGE_VIEWS_MAX_OUT, T, C), dtype=torch.float32, device=dev)
            sc = torch.tensor([[1.0 / scale, 1.0 / scale]], dtype=torch.float32).to(dev)
            extra = {"orientations": orient, "pred_text_dist": text_dist}
            if rois is not None:
                # the masks' frame: the merged boxes, before word post-processing, in the original image's pixels
                extra["pred_mask_rois"] = rois
                extra["pred_mask_boxes"] = self._scaled_boxes(m["boxes"].unsqueeze(0), sc)
            res = self.post_processor.process_padded(m["boxes"].unsqueeze(0), m["scores"].unsqueeze(0), m["count"][:1], text, sc,
                                                     [(height, width)], extra)[0]
        else:
            res = Instances((height, width))
            res.pred_boxes = RotatedBoxes(m["boxes"][:n_out])
            res.scores = m["scores"][:n_out]
            res.pred_classes = torch.zeros((n_out,), dtype=torch.int64, device=dev)
            for name, t in (("orientations", orient), ("pred_text_prob", text), ("pred_text_dist", text_dist)):
                if t is not None:
                    res.set(name, t[0, :n_out])
            if scale != 1:
                res.pred_boxes.scale(1 / scale, 1 / scale)
            if rois is not None:
                # no word post-processing here: the masks' frame is pred_boxes as they now stand, in original pixels (a copy,
                # taken AFTER the in-place scale above, which also went through m["boxes"])
                res.pred_mask_rois = rois[0, :n_out]
                res.pred_mask_boxes = res.pred_boxes.tensor.clone()
        self.logger.info(f"Tiled inference: {len(plan.tiles)} tiles{' + the full view' if with_full else ''}, {n_out} merged "
                         f"detections, {len(res)} word instances")
        return res

    def run_rotated(self, image: np.ndarray, angle: float, fill=(0, 0, 0)) -> Instances:
        """The robustness probe and the deskewing primitive: the words of `image` as the model reads them when the image is
        turned by `angle` degrees (counter-clockwise) first, returned in the ORIGINAL image's frame.  The image is converted to
        grey on the host where the format asks for it, uploaded once and rotated on the device as
        `PIL.Image.rotate(angle, BILINEAR, expand=True, fillcolor=fill)` rotates it (ops.native.rotate_u8, byte for byte); the
        front end, the model and the post-processor then run on the rotated image exactly as `run_batch` runs them, in the
        rotated frame, and `pred_boxes` - and, where present, `pred_mask_boxes` and `pred_char_frames` - come back through the
        inverse map (ops.native.rotate_boxes: the centre through the matrix, the angle minus `angle`, wrapped into
        [-180, 180)); the corners in `pred_polygons` go through the same matrix as points.  The image size of the result is the original's.  At angle % 360 == 0 this is `run_batch([image])[0]`.
        Pasted masks (rasters in the rotated frame) and the line, block, row and table fields are not mapped:
        NotImplementedError with MODEL.ROI_MASK_HEAD.MASK_INFERENCE and PASTE_MASKS True, and with
        POST_PROCESSING.GROUP_LINES."""
        from ..data.transforms import RotationTransform, check_fill
        angle = float(angle)
        if not np.isfinite(angle):
            raise ValueError(f"run_rotated: angle {angle}")
        fill = check_fill(fill)
        if angle % 360.0 == 0.0:
            return self.run_batch([image])[0]
        if bool(getattr(self.model.roi_heads, "mask_inference", False)) and getattr(self.model, "paste_masks", True):
            raise NotImplementedError("run_rotated: MODEL.ROI_MASK_HEAD.MASK_INFERENCE is on and the masks are pasted in the rotated "
                                      "image's frame; set MODEL.ROI_MASK_HEAD.PASTE_MASKS False to carry the RoI masks "
                                      "(pred_mask_rois / pred_mask_boxes) instead")
        if bool(self.cfg.POST_PROCESSING.GROUP_LINES):
            raise NotImplementedError("run_rotated: POST_PROCESSING.GROUP_LINES is on; the line, block, row and table boxes (and "
                                      "their padding rows) are not mapped back from the rotated frame")
        height, width = image.shape[:2]
        rotation = RotationTransform(height, width, angle)
        u8 = torch.from_numpy(np.ascontiguousarray(self._grey(image))).to(self.device)
        res = self.run_batch([K.rotate_u8(u8, rotation, fill)])[0]
        res.pred_boxes = RotatedBoxes(K.rotate_boxes(res.pred_boxes.tensor.contiguous(), rotation, inverse=True))
        for name in ("pred_mask_boxes", "pred_char_frames"):
            if res.has(name):
                res.set(name, K.rotate_boxes(res.get(name).contiguous(), rotation, inverse=True))
        if res.has("pred_polygons"):
            # the words' corners [R, 4, 2] are points: through the matrix itself, in float64, rounded once (a few small
            # launches; RotationTransform.inverse_coords is the same statement on the host)
            p, m = res.pred_polygons.double(), rotation.matrix
            x, y = p[..., 0], p[..., 1]
            res.pred_polygons = torch.stack([m[0] * x + m[1] * y + m[2], m[3] * x + m[4] * y + m[5]], -1).float()
        res._image_size = (int(height), int(width))
        return res

    def run_views(self, image: np.ndarray, angles=(0.0, 90.0, 180.0, 270.0), scales=(1.0,), fill=(0, 0, 0), rank: str = "product",
                  min_votes: int = 1, nms_thresh: Optional[float] = None, batch_size: int = 8) -> Instances:
        """Test-time augmentation: the image at every rotation of `angles` (degrees counter-clockwise, rotated on the device as
        run_rotated rotates it) times every scale of `scales` (1.0: what `__call__` would feed for the rotated image), fused
        into ONE detection set in the original image's frame (view_fusion.plan_views, ops.native.fuse_views =
        glass_fuse_views).  Of the copies of a word that several views hold (rotated IoU >= `nms_thresh`, default
        MODEL.ROI_HEADS.NMS_THRESH_TEST, between boxes of different views) the one with the best key stays: `rank` "product"
        = detection score times word score, "word" = the word score alone, "detection" = the detection score alone - the
        upside-down copy of a word is detected as well as the upright one but read badly.  A detection whose centre lies
        outside the image (the fill corners of a rotated canvas) is dropped, and so is one that fewer than `min_votes` views
        found.  The fused set - at most 1024 detections - takes the ordinary way through the word post-processor, with the
        boxes in the original image's pixels.  Per word: `pred_view_votes` (how many views found it), `pred_view` (the view of
        the copy that was kept: index into the angle-major, scale-minor list) and `pred_view_mask` (bit v: view v), all int64;
        `orientations` are carried as that view emitted them, in its frame."""
        from ..data.transforms import check_fill
        from .view_fusion import plan_views
        heads = self.model.roi_heads
        if _char_boxes_on(self.model):
            raise NotImplementedError("run_views: MODEL.ROI_RECOGNIZER_HEAD.CHAR_BOXES is on; the character rows are not carried "
                                      "through the fusion of views (use run_rotated, or switch the key off)")
        with_masks = bool(getattr(heads, "mask_inference", False))
        if with_masks and getattr(self.model, "paste_masks", True):
            raise NotImplementedError("run_views: MODEL.ROI_MASK_HEAD.MASK_INFERENCE is on and the masks are pasted per view frame, "
                                      "which cannot be fused; set MODEL.ROI_MASK_HEAD.PASTE_MASKS False to carry the RoI masks "
                                      "(pred_mask_rois / pred_mask_boxes) instead")
        if getattr(getattr(heads, "recognizer_head", None), "image_segments", None) is not None:
            raise NotImplementedError("run_views: the recogniser head carries per-image lexicon segments (image_segments); the "
                                      "views of one image are not images of that list - set the lexicon with one segment")
        if getattr(self.model, "inflate_ratio", None) or getattr(self.model, "drop_overlapping_boxes", None):
            raise NotImplementedError("run_views needs the model's padded device batch; POST_PROCESSING.INFLATE_RATIO / "
                                      "POST_PROCESSING.DROP_OVERLAPPING take the list-wise path, which has none")
        if rank not in ("detection", "product", "word"):
            raise ValueError(f"run_views: rank={rank!r} (one of detection, product, word)")
        fill = check_fill(fill)
        height, width = (int(v) for v in image.shape[:2])
        views = plan_views(height, width, angles, scales, self.get_inference_scale_ratio)
        V, Kdet, min_votes = len(views), int(self.cfg.TEST.DETECTIONS_PER_IMAGE), int(min_votes)
        if V * Kdet > K.FUSE_VIEWS_MAX_SLOTS:
            raise ValueError(f"run_views: {V} views of {Kdet} detections each exceed the {K.FUSE_VIEWS_MAX_SLOTS} slots of one "
                             f"fusion (at most {K.FUSE_VIEWS_MAX_SLOTS // Kdet} views at TEST.DETECTIONS_PER_IMAGE {Kdet})")
        if not 1 <= min_votes <= V:
            raise ValueError(f"run_views: min_votes={min_votes} with {V} views (1..{V})")
        dev = self.device
        # ---- the views: one upload, a rotation per angle, the front end per view
        u8 = torch.from_numpy(np.ascontiguousarray(self._grey(image))).to(dev)
        rotated, inputs = {}, []
        for view in views:
            key = id(view.rotation)
            if key not in rotated:
                rotated[key] = u8 if view.rotation.kind == 0 else K.rotate_u8(u8, view.rotation, fill)
            t = self._image_at_scale(rotated[key], view.rho)
            inputs.append({"image": t, "height": t.shape[1], "width": t.shape[2]})
        # ---- the model: views grouped by padded shape (run_batch), calls of at most batch_size, joined along the view axis
        d = self.model.backbone.size_divisibility
        groups = {}
        for i, inp in enumerate(inputs):
            groups.setdefault(((inp["height"] + d - 1) // d * d, (inp["width"] + d - 1) // d * d), []).append(i)
        step = max(int(batch_size), 1)
        calls = [idxs[i:i + step] for idxs in groups.values() for i in range(0, len(idxs), step)]
        dets = []
        for call in calls:
            det = getattr(self.model([inputs[i] for i in call]), "batch", None)
            if det is None:
                raise RuntimeError("run_views needs the model's padded device batch")
            if tuple(det.scores.shape) != (len(call), Kdet):
                raise RuntimeError(f"run_views: a batch of scores {tuple(det.scores.shape)}, expected {(len(call), Kdet)}")
            dets.append(det)
        perm = [i for call in calls for i in call]                 # row r of the joined batches is view perm[r]
        back = None
        if perm != list(range(V)):
            back = K.upload(np.argsort(np.asarray(perm)), torch.int64, dev)

        def joined(name, tail):
            parts = [getattr(dt, name, None) for dt in dets]
            if all(p is None for p in parts):
                return None
            t = torch.cat([p if p is not None else torch.zeros((dt.scores.shape[0], Kdet) + tail, dtype=torch.float32, device=dev)
                           for p, dt in zip(parts, dets)], 0)
            return t if back is None else t.index_select(0, back)
        T = self.cfg.MODEL.ROI_RECOGNIZER_HEAD.MAX_WORD_LENGTH + 1
        C = len(self.cfg.MODEL.ROI_RECOGNIZER_HEAD.CHARACTER_SET) + 2
        boxes, scores = joined("boxes", (5,)), joined("scores", ())
        orient, text, text_dist = joined("orient", (2,)), joined("text", (T, C)), joined("text_dist", (T, C))
        counts = torch.cat([dt.counts_dev for dt in dets], 0)
        counts = (counts if back is None else counts.index_select(0, back)).contiguous()
        if text is None and sum(sum(dt.counts_host) for dt in dets) > 0:
            raise RuntimeError("recognizer output missing")
        rois = None
        if with_masks:       # PASTE_MASKS False: the views' mask rows [n, K, M, M] (a call without a detection has none)
            have = [dt.mask_rois for dt in dets if getattr(dt, "mask_rois", None) is not None]
            rois = joined("mask_rois", tuple(have[0].shape[2:])) if have else None
        # ---- the keys' text rows, the fusion, and the survivors' rows gathered by their source slot
        arg = mx = None
        if rank != "detection":
            if text is not None:
                arg, mx = K.text_argmax(text.contiguous(), counts)
            else:            # no detection in any view
                arg = torch.zeros((V, Kdet, T), dtype=torch.int32, device=dev)
                mx = torch.zeros((V, Kdet, T), dtype=torch.float32, device=dev)
        thr = float(self.cfg.MODEL.ROI_HEADS.NMS_THRESH_TEST if nms_thresh is None else nms_thresh)
        stop = self.post_processor.text_encoder.character.index("[s]")
        m = K.fuse_views(boxes.contiguous(), scores.contiguous(), counts, K.upload([list(v.affine) for v in views], torch.float64, dev),
                         K.upload([0.0, 0.0, float(width), float(height)], torch.float32, dev), thr, arg, mx, stop, rank,
                         min_votes, K.FUSE_VIEWS_MAX_OUT)
        src = m["src"].long()
        gather = lambda t: None if t is None else t.reshape((V * Kdet,) + tuple(t.shape[2:])).index_select(0, src).unsqueeze(0)
        orient, text, text_dist, rois = gather(orient), gather(text), gather(text_dist), gather(rois)
        votes, view_of, mask = m["votes"].long().unsqueeze(0), (src // Kdet).unsqueeze(0), m["views"].unsqueeze(0)
        n_out, truncated, n_kept = m["count"].tolist()             # the one read of out_count
        if truncated:
            self.logger.warning(f"run_views: more than {K.FUSE_VIEWS_MAX_OUT} fused detections; the lowest-ranked are cut off")
        if self.post_process_flag:
            if text is None:          # no detections in any view
                text = torch.zeros((1, K.FUSE_VIEWS_MAX_OUT, T, C), dtype=torch.float32, device=dev)
            one = torch.ones((1, 2), dtype=torch.float32, device=dev)
            extra = {"orientations": orient, "pred_text_dist": text_dist, "pred_view_votes": votes, "pred_view": view_of,
                     "pred_view_mask": mask}
            if rois is not None:      # the masks' frame: the fused boxes, before word post-processing, in the original's pixels
                extra["pred_mask_rois"] = rois
                extra["pred_mask_boxes"] = m["boxes"].unsqueeze(0)
            res = self.post_processor.process_padded(m["boxes"].unsqueeze(0), m["scores"].unsqueeze(0), m["count"][:1], text, one,
                                                     [(height, width)], extra)[0]
        else:
            res = Instances((height, width))
            res.pred_boxes = RotatedBoxes(m["boxes"][:n_out])
            res.scores = m["scores"][:n_out]
            res.pred_classes = torch.zeros((n_out,), dtype=torch.int64, device=dev)
            for name, t in (("orientations", orient), ("pred_text_prob", text), ("pred_text_dist", text_dist),
                            ("pred_view_votes", votes), ("pred_view", view_of), ("pred_view_mask", mask)):
                if t is not None:
                    res.set(name, t[0, :n_out])
            if rois is not None:
                res.pred_mask_rois = rois[0, :n_out]
                res.pred_mask_boxes = res.pred_boxes.tensor.clone()
        self.logger.info(f"Fused views: {V} views, {n_kept} distinct detections, {n_out} with at least {min_votes} votes, "
                         f"{len(res)} word instances")
        return res

    def __call__(self, original_image: np.ndarray) -> Instances:
        return self.run_batch([original_image])[0]

    def preds_boxes_to_polygons(self, pred_boxes):
        return self.post_processor.boxes_to_polygons(boxes=pred_boxes.tensor)
