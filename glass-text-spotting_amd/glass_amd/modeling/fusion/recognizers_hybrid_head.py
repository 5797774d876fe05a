"""The GLASS ROI head (`MaskRotatedRecognizerHybridHead`), inference path, on HIP kernels.

Mirrors reference glass/modeling/fusion/recognizers_hybrid_head.py: constructor wiring
(`_init_box_head` :183-216, `_init_recognizer_head` :445-511), `forward` eval branch
(:176-181), `_forward_box` (:291-339), `_forward_recognizer` (:513-569) and
`forward_with_given_boxes` (:571-609; 3-argument form).  The rotated mask branch (`_forward_mask`, :378-442) is
off at inference in every shipped config (`MASK_INFERENCE: false`) and runs when the eval CLI's
`MODEL.ROI_MASK_HEAD.MASK_INFERENCE True` is set.

Two surfaces:
  * the reference's: `forward(images, features, proposals, targets=None) -> (list[Instances], {})`
    with logical-NCHW feature tensors, so it drops into a detectron2-style meta-arch;
  * `forward_batched(...)`: the device-resident path GlassRCNN uses — padded proposal slots in,
    one host sync (the per-image detection counts), all RoIs of all images batched through the
    recognition branch.  Per-image results are identical to calling the reference image by image.
"""
from __future__ import annotations

import os
from typing import Dict, List, Optional, Tuple

import torch

from ...utils.module import InferenceModule
from ...utils.pipeline import ReadBack, drive

from ...ops import native as K
from ...structures.core import ImageList, Instances, RotatedBoxes, ShapeSpec
from ...utils.registry import ROI_HEADS_REGISTRY
from ..backbone.resnet_fpn import as_nhwc
from ..recognition.recognizer_head_v2 import build_recognizer_head, split_text_rows
from ..roi_heads.box_head import build_box_head
from ..roi_heads.rotated_fast_rcnn import RotatedFastRCNNOutputLayers
from .fusion_modules import P2P3Fusion, build_hybrid_feature_fusion
from .local_feature_extraction import build_hybrid_feature_extractor


class InjectedBoxes:
    """word boxes handed to the recognizer instead of the detections (synthetic workloads, teacher-forced parity), padded to
    [N, kmax, 5] with unit scores - built ONCE by `prepare_injected_boxes` when the same boxes are injected step after step"""
    __slots__ = ("boxes", "scores", "orient", "counts_dev", "counts_host", "flat", "roi_image")


def prepare_injected_boxes(box_list, device) -> InjectedBoxes:
    inj = InjectedBoxes()
    N = len(box_list)
    counts = [len(b) for b in box_list]
    kmax = max(counts + [1])
    pb = torch.zeros((N, kmax, 5), dtype=torch.float32, device=device)
    sc = torch.zeros((N, kmax), dtype=torch.float32, device=device)
    for n, b in enumerate(box_list):
        if len(b):
            pb[n, : len(b)] = b.to(device).float()
            sc[n, : len(b)] = 1.0
    inj.boxes, inj.scores, inj.orient = pb, sc, torch.zeros((N, kmax, 2), device=device)
    inj.counts_dev, inj.counts_host = K.upload(counts, torch.int32, device), tuple(counts)
    inj.flat = (torch.cat([pb[n, :c] for n, c in enumerate(counts)], 0).contiguous() if sum(counts) else torch.zeros((0, 5), device=device))
    inj.roi_image = K.upload(torch.repeat_interleave(torch.arange(N, dtype=torch.int32), torch.tensor(counts)), torch.int32, device)
    return inj


class BatchedDetections:
    """Padded, device-resident detections of one step: boxes [N,K,5], scores [N,K], orient [N,K,2]|None,
    counts (device int32 [N] + host list), text [sum counts, T, C]|None with per-image row offsets."""

    def __init__(self, boxes, scores, orient, counts_dev, counts_host, image_sizes):
        self.boxes, self.scores, self.orient = boxes, scores, orient
        self.counts_dev, self.counts_host, self.image_sizes = counts_dev, list(counts_host), list(image_sizes)
        self.text = None
        self.text_dist = None         # BEAM_DISTRIBUTIONS: the best hypothesis's full per-step rows, laid out like `text`
        self.chars = None             # CHAR_BOXES: the packed character rows (postprocess.char_boxes.pack_chars), laid out like `text`
        self.char_frames = None       # CHAR_BOXES: the boxes the characters lie in, padded [N,K,5] (None: `boxes` themselves)
        self.masks = None             # [sum counts, 1, M, M] mask probabilities (MASK_INFERENCE), or padded [N,K,M,M]
        self.kept_index = None        # [N,K] int32: index into the image's proposal list each detection came from
        self.detected = None          # with override_boxes: the box head's own detections (this object holds the overrides)
        self.proposals = None         # (boxes [N,P,5], logits [N,P], counts [N]) of the RPN, set by the meta-arch
        self.handoff = None           # ops.native.HandoffGuard of the recognizer call that produced `text` (until resolved)
        self.roi_start_host = [0]
        for c in self.counts_host[:-1]:
            self.roi_start_host.append(self.roi_start_host[-1] + c)

    def to_instances(self) -> List[Instances]:
        """per-image views, no kernels besides one zero-fill for pred_classes"""
        N, K = self.scores.shape
        classes = torch.zeros((N, K), dtype=torch.int64, device=self.scores.device)
        out = []
        for n, size in enumerate(self.image_sizes):
            c = self.counts_host[n]
            r = Instances(size)
            r.pred_boxes = RotatedBoxes(self.boxes[n, :c])
            r.scores = self.scores[n, :c]
            r.pred_classes = classes[n, :c]
            if self.orient is not None:
                r.orientations = self.orient[n, :c]
            if self.text is not None:
                if self.text.dim() == 4:                      # padded [N,K,T,C] (after the finalize kernel)
                    r.pred_text_prob = self.text[n, :c]
                else:
                    s0 = self.roi_start_host[n]
                    r.pred_text_prob = self.text[s0:s0 + c]
            if self.text_dist is not None:
                if self.text_dist.dim() == 4:
                    r.pred_text_dist = self.text_dist[n, :c]
                else:
                    s0 = self.roi_start_host[n]
                    r.pred_text_dist = self.text_dist[s0:s0 + c]
            if self.chars is not None:
                from ...postprocess.char_boxes import attach_chars
                s0 = self.roi_start_host[n]
                frames = self.boxes if self.char_frames is None else self.char_frames
                attach_chars(r, self.chars[n, :c] if self.chars.dim() == 4 else self.chars[s0:s0 + c], frames[n, :c])
            if self.masks is not None:                        # forward_with_given_boxes, :595-606
                s0 = self.roi_start_host[n]
                r.pred_masks = self.masks[s0:s0 + c]
                r.pred_rboxes = r.pred_boxes
            out.append(r)
        return out


def images_nhwc4(images: ImageList) -> torch.Tensor:
    """NHWC4 batch behind an ImageList (ours carry it; a foreign one is converted once)."""
    t = getattr(images, "nhwc4", None)
    if t is not None:
        return t
    x = images.tensor.permute(0, 2, 3, 1)
    if x.shape[-1] == 3:
        x = torch.nn.functional.pad(x, (0, 1))
    return x.contiguous()


@ROI_HEADS_REGISTRY.register()
class MaskRotatedRecognizerHybridHead(InferenceModule):
    def __init__(self, cfg, input_shape: Dict[str, ShapeSpec]):
        super().__init__()
        # ---- box branch (:183-216)
        self.box_in_features = list(cfg.MODEL.ROI_HEADS.IN_FEATURES)
        self.box_pooler_resolution = cfg.MODEL.ROI_BOX_HEAD.POOLER_RESOLUTION
        self.box_pooler_scales = tuple(1.0 / input_shape[k].stride for k in self.box_in_features)
        self.box_sampling_ratio = cfg.MODEL.ROI_BOX_HEAD.POOLER_SAMPLING_RATIO
        assert cfg.MODEL.ROI_BOX_HEAD.POOLER_TYPE in ["ROIAlignRotated"], cfg.MODEL.ROI_BOX_HEAD.POOLER_TYPE
        in_channels = [input_shape[f].channels for f in self.box_in_features][0]
        r = self.box_pooler_resolution
        self.box_head = build_box_head(cfg, ShapeSpec(channels=in_channels, height=r, width=r))
        self.box_predictor = RotatedFastRCNNOutputLayers(cfg, self.box_head.output_shape)
        # ---- recognizer branch (:445-511)
        self.recognizer_on = bool(cfg.MODEL.RECOGNIZER_ON)
        rc = cfg.MODEL.ROI_RECOGNIZER_HEAD
        self.recognizer_in_features = list(rc.IN_FEATURES)
        assert rc.POOLER_TYPE in ["ROIAlignRotated"], rc.POOLER_TYPE
        if rc.RECOGNIZER_HEAD.POOLER_PAD.NAME:
            # reference recognizer_pooler_pad.py:28-95 (FeatPadV2): pads AXIS-ALIGNED pooled boxes (it indexes x1,y1,x2,y2);
            # the GLASS head pools rotated boxes and every shipped config leaves the name empty
            raise NotImplementedError(
                f"POOLER_PAD.NAME={rc.RECOGNIZER_HEAD.POOLER_PAD.NAME!r}: FeatPadV2 (reference recognizer_pooler_pad.py:28-95) is "
                "written for axis-aligned boxes and is unusable with the rotated pooler of this head; not built")
        assert len(self.recognizer_in_features) == 2, "recognizer expects [p2, p3] (all reference configs)"
        self.rec_ph, self.rec_pw = rc.POOLER_RESOLUTION_HEIGHT, rc.POOLER_RESOLUTION_WIDTH
        self.rec_scale = 1.0 / input_shape[self.recognizer_in_features[0]].stride
        self.rec_sampling_ratio = rc.POOLER_SAMPLING_RATIO
        rin = input_shape[self.recognizer_in_features[0]].channels
        self.recognizer_feature_fusion = P2P3Fusion(rin)
        shape = ShapeSpec(channels=rin, width=self.rec_pw, height=self.rec_ph)
        self.img_pooler_size = (self.rec_ph * 16, self.rec_pw * 4)
        self.img_sampling_ratio = cfg.MODEL.ROI_BOX_HEAD.POOLER_SAMPLING_RATIO
        self.hybrid_net = build_hybrid_feature_extractor(cfg, shape)
        self.fusion_net = build_hybrid_feature_fusion(cfg, shape)
        self.recognizer_head = build_recognizer_head(cfg, shape)
        # ---- mask branch (:342-376): pooler over ROI_HEADS.IN_FEATURES, built only when it will run
        self.mask_inference = bool(cfg.MODEL.ROI_MASK_HEAD.MASK_INFERENCE)
        self.mask_head = None
        if self.mask_inference:
            assert cfg.MODEL.MASK_ON, "MASK_INFERENCE needs MODEL.MASK_ON (the checkpoint must carry roi_heads.mask_head.*)"
            from ..roi_heads.rotated_mask_head import build_mask_head
            self.mask_pooler_resolution = cfg.MODEL.ROI_MASK_HEAD.POOLER_RESOLUTION
            self.mask_sampling_ratio = cfg.MODEL.ROI_MASK_HEAD.POOLER_SAMPLING_RATIO
            mr = self.mask_pooler_resolution
            self.mask_head = build_mask_head(cfg, ShapeSpec(channels=in_channels, height=mr, width=mr))
        self.local_ch = cfg.MODEL.LOCAL_FEATURE_EXTRACTOR.NUM_FEATURES
        self.two_stream_local = os.environ.get("GLASS_SINGLE_STREAM", "0") != "1"
        self._streams = None

    def import_weights(self, sd, device, prefix: str = "roi_heads.") -> None:
        self.box_head.import_weights(sd, device, prefix + "box_head.")
        self.box_predictor.import_weights(sd, device, prefix + "box_predictor.")
        self.recognizer_feature_fusion.import_weights(sd, device, prefix + "recognizer_feature_fusion.")
        self.hybrid_net.import_weights(sd, device, prefix + "hybrid_net.")
        self.fusion_net.import_weights(sd, device, prefix + "fusion_net.")
        self.recognizer_head.import_weights(sd, device, prefix + "recognizer_head.")
        if self.mask_head is not None:
            self.mask_head.import_weights(sd, device, prefix + "mask_head.")

    # ================================================================== device-resident path
    def box_branch_batched(self, feats: Dict[str, torch.Tensor], prop_boxes: torch.Tensor, prop_counts: torch.Tensor,
                           image_hw_dev: torch.Tensor):
        """feats: NHWC level tensors by name; prop_boxes [N,P,5] (padded), prop_counts int32 [N]."""
        N, P, _ = prop_boxes.shape
        device = prop_boxes.device
        bidx = torch.arange(N, dtype=torch.int32, device=device).repeat_interleave(P)
        fl = [feats[f] for f in self.box_in_features]
        r = self.box_pooler_resolution
        pooled = K.roi_align_rotated(fl, self.box_pooler_scales, prop_boxes.view(-1, 5), bidx, (r, r), self.box_sampling_ratio)
        x = self.box_head.forward_nhwc(pooled)
        preds = self.box_predictor(x)
        return self.box_predictor.inference_batched(preds, prop_boxes, prop_counts, image_hw_dev)

    def recognizer_branch_batched(self, img_nhwc4: torch.Tensor, feats: Dict[str, torch.Tensor], boxes: torch.Tensor,
                                  roi_image: torch.Tensor, num_images: int, return_intermediates: bool = False, guard=None):
        """boxes [R,5], roi_image int32 [R] -> pred_text_prob [R,26,97] (R > 0; with BEAM_DISTRIBUTIONS the pair
        (pred_text_prob, pred_text_dist), with CHAR_BOXES the triple, see recognizer_head_v2.split_text_rows).  `guard`: ops.native.HandoffGuard the caller
        resolves at its next read-back (None: the recognizer head reads the hand-off status itself, synchronising)."""
        R = boxes.shape[0]
        p2, p3 = feats[self.recognizer_in_features[0]], feats[self.recognizer_in_features[1]]
        fus = self.recognizer_feature_fusion
        # channel-interleaved cat(local, global): local -> even channels, global -> odd channels
        if hasattr(fus, "can_pool") and fus.can_pool(p2, p3, R, self.rec_ph * self.rec_pw):
            # pool first, fuse the pooled bins (P2P3Fusion.pooled_nhwc: both stages are linear)
            C = fus.out_channels
            xcat = torch.empty((R, self.rec_ph, self.rec_pw, self.local_ch + C), dtype=torch.float32, device=boxes.device)
            fus.pooled_nhwc(p2, p3, self.rec_scale, boxes, roi_image, (self.rec_ph, self.rec_pw), self.rec_sampling_ratio,
                            out=xcat, out_coff=1, out_cstride=2)
        else:
            g = fus.forward_nhwc(p2, p3)
            C = g.shape[-1]
            xcat = torch.empty((R, self.rec_ph, self.rec_pw, self.local_ch + C), dtype=torch.float32, device=boxes.device)
            K.roi_align_rotated([g], [self.rec_scale], boxes, roi_image, (self.rec_ph, self.rec_pw), self.rec_sampling_ratio,
                                out=xcat, out_coff=1, out_cstride=2)
        crops = K.roi_align_rotated([img_nhwc4], [1.0], boxes, roi_image, self.img_pooler_size, self.img_sampling_ratio,
                                    channels=4)
        self._local_extractor_streams(crops, xcat)
        inter = {"xcat": xcat.clone(), "crops": crops} if return_intermediates else None
        fused = self.fusion_net.forward_interleaved(xcat)
        probs = self.recognizer_head.forward_nhwc(fused, roi_image, num_images, guard=guard)
        if return_intermediates:
            inter["fused"] = fused
            return probs, inter
        return probs

    def mask_branch_batched(self, feats: Dict[str, torch.Tensor], boxes: torch.Tensor, roi_image: torch.Tensor) -> torch.Tensor:
        """`_forward_mask` at inference (:378-442) for all RoIs of the step: ROIAlignRotated 14x14 over
        ROI_HEADS.IN_FEATURES on the rotated boxes, mask head, sigmoid -> pred_masks [R,1,28,28]."""
        fl = [feats[f] for f in self.box_in_features]
        r = self.mask_pooler_resolution
        pooled = K.roi_align_rotated(fl, self.box_pooler_scales, boxes, roi_image, (r, r), self.mask_sampling_ratio)
        return self.mask_head.forward_nhwc(pooled)

    def _local_extractor_streams(self, crops: torch.Tensor, xcat: torch.Tensor) -> None:
        """Local extractor on all RoIs.  RoIs are independent, so the batch is split in two halves enqueued on
        two HIP streams: every layer's grid (e.g. 2112 tiles on 768 resident slots at 16x33) ends in a partial
        wave of tiles, and with two independent streams the idle CUs of one half's tail run the other half's
        next layer instead of waiting (measured +3.5 % on the whole step: 115.0 vs 111.1 images/s, 3 runs each)."""
        R = crops.shape[0]
        if R < 64 or not self.two_stream_local:
            self.hybrid_net.forward_nhwc(crops, out=xcat, out_coff=0, out_cstride=2)
            return
        if self._streams is None:
            self._streams = (torch.cuda.Stream(device=crops.device), torch.cuda.Stream(device=crops.device))
        cur = torch.cuda.current_stream()
        ready = torch.cuda.Event()
        ready.record(cur)
        h = (R // 2 + 7) // 8 * 8                       # keep both halves' pixel counts tile-friendly
        parts = ((0, h), (h, R))
        for st, (a, b) in zip(self._streams, parts):
            st.wait_event(ready)
            with torch.cuda.stream(st):
                self.hybrid_net.forward_nhwc(crops[a:b], out=xcat[a:b], out_coff=0, out_cstride=2)
                crops.record_stream(st)
                xcat.record_stream(st)
        for st in self._streams:
            cur.wait_stream(st)

    def forward_batched(self, img_nhwc4: torch.Tensor, feats: Dict[str, torch.Tensor], prop_boxes: torch.Tensor,
                        prop_counts: torch.Tensor, image_sizes: List[Tuple[int, int]],
                        override_boxes: Optional[List[torch.Tensor]] = None) -> BatchedDetections:
        return drive(self.forward_batched_g(img_nhwc4, feats, prop_boxes, prop_counts, image_sizes, override_boxes))

    def box_branch_detections(self, feats, prop_boxes, prop_counts, image_hw_dev):
        """box branch + the orientation rows of the kept detections: device tensors only, static shapes (the part of
        the ROI head that the meta-arch captures into its hipGraph)."""
        ob, os_, oi, orient2, oc = self.box_branch_batched(feats, prop_boxes, prop_counts, image_hw_dev)
        orient = None
        if orient2 is not None:
            orient = torch.gather(orient2, 1, oi.long().unsqueeze(-1).expand(-1, -1, 2))
        return ob, os_, oi, orient, oc

    def forward_batched_g(self, img_nhwc4: torch.Tensor, feats: Dict[str, torch.Tensor], prop_boxes: torch.Tensor,
                          prop_counts: torch.Tensor, image_sizes: List[Tuple[int, int]],
                          override_boxes: Optional[List[torch.Tensor]] = None, box_out=None):
        """Generator form (utils/pipeline.py): yields a ReadBack where the host needs the detection counts.
        `box_out`: (boxes, scores, kept index, orientations, counts) when the caller already ran the box branch."""
        device = prop_boxes.device
        if box_out is None:
            hw = K.upload(image_sizes, torch.int32, device)
            box_out = self.box_branch_detections(feats, prop_boxes, prop_counts, hw)
        ob, os_, oi, orient, oc = box_out
        orient2 = orient
        counts = (yield ReadBack(oc))[0].tolist()     # host read-back: per-image detection counts size the recognizer batch
        det = BatchedDetections(ob, os_, orient, oc, counts, image_sizes)
        det.kept_index = oi
        if override_boxes is not None:
            real = det
            # synthetic-workload hook (bench / teacher-forced parity): recognise these boxes instead.  A caller that injects
            # the same boxes step after step (bench.py: they are INPUTS, resident in HBM like the images) prepares the padded
            # batch once with `prepare_injected_boxes`; a plain list is padded here, per call
            inj = override_boxes if isinstance(override_boxes, InjectedBoxes) else prepare_injected_boxes(override_boxes, device)
            det = BatchedDetections(inj.boxes, inj.scores, inj.orient if orient2 is not None else None, inj.counts_dev,
                                    list(inj.counts_host), image_sizes)
            det.flat_boxes = (inj.flat, inj.roi_image)
            det.detected = real
        return self.recognize_batched(img_nhwc4, feats, det)

    def recognize_batched(self, img_nhwc4, feats, det: BatchedDetections) -> BatchedDetections:
        if not self.recognizer_on:
            return det
        counts = det.counts_host
        R = sum(counts)
        if R == 0:
            return det          # reference: recognizer_head returns the instances untouched (recognizer_head_v2.py:151)
        device = img_nhwc4.device
        flat = getattr(det, "flat_boxes", None)            # (prepared injected boxes carry their flattened form)
        if flat is not None:
            boxes, roi_image = flat
        else:
            boxes = torch.cat([det.boxes[n, :c] for n, c in enumerate(counts)], 0).contiguous()
            roi_image = K.upload(torch.repeat_interleave(torch.arange(len(counts), dtype=torch.int32), torch.tensor(counts)), torch.int32, device)
        # the one-launch recurrent kernels report a hand-off that gave up into det.handoff.status; the meta-arch reads it with
        # the surviving counts (its next read-back) and, if set, replaces det.text by det.handoff.retry() - the step kernels
        det.handoff = K.HandoffGuard(device)
        det.text, det.text_dist, det.chars = split_text_rows(
            self.recognizer_branch_batched(img_nhwc4, feats, boxes, roi_image, len(counts), guard=det.handoff), chars=True)
        if self.mask_inference:
            det.masks = self.mask_branch_batched(feats, boxes, roi_image)
        return det

    def _recognize_into(self, img_nhwc4, feats, results: List[Instances]) -> List[Instances]:
        counts = [len(r) for r in results]
        R = sum(counts)
        device = img_nhwc4.device
        boxes = roi_image = None
        if R > 0:
            boxes = torch.cat([r.pred_boxes.tensor for r in results], 0).contiguous()
            roi_image = K.upload(torch.repeat_interleave(torch.arange(len(counts), dtype=torch.int32), torch.tensor(counts)), torch.int32, device)
        # reference: with no boxes the recognizer head returns the instances untouched (recognizer_head_v2.py:151)
        if self.recognizer_on and R > 0:
            probs, dist, chars = split_text_rows(self.recognizer_branch_batched(img_nhwc4, feats, boxes, roi_image, len(counts)),
                                                 chars=True)
            for p, r in zip(probs.split(counts, dim=0), results):
                r.pred_text_prob = p
            if chars is not None:              # CHAR_BOXES: the characters' frame is the box that was pooled
                from ...postprocess.char_boxes import attach_chars
                for ch, r in zip(chars.split(counts, dim=0), results):
                    attach_chars(r, ch, r.pred_boxes.tensor)
            if dist is not None:
                for d, r in zip(dist.split(counts, dim=0), results):
                    r.pred_text_dist = d
        if self.mask_inference:            # forward_with_given_boxes, :594-606
            if R > 0:
                masks = self.mask_branch_batched(feats, boxes, roi_image).split(counts, dim=0)
            else:
                m = 2 * self.mask_pooler_resolution
                masks = [torch.zeros((0, 1, m, m), dtype=torch.float32, device=device) for _ in results]
            for mk, r in zip(masks, results):
                r.pred_masks = mk
                r.pred_rboxes = r.pred_boxes
        return results

    # ================================================================== reference surface
    def _nhwc_feats(self, features: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        return {k: as_nhwc(v) for k, v in features.items()}

    def forward(self, images: ImageList, features: Dict[str, torch.Tensor], proposals: List[Instances], targets=None):
        assert not self.training and targets is None, "inference only (training is out of scope)"
        pred_instances = self._forward_box(features, proposals)
        pred_instances = self.forward_with_given_boxes(images, features, pred_instances)
        return pred_instances, {}

    def _forward_box(self, features: Dict[str, torch.Tensor], proposals: List[Instances]) -> List[Instances]:
        feats = self._nhwc_feats({f: features[f] for f in self.box_in_features})
        device = feats[self.box_in_features[0]].device
        counts = [len(p) for p in proposals]
        N, P = len(proposals), max(counts + [1])
        pb = torch.zeros((N, P, 5), dtype=torch.float32, device=device)
        for n, p in enumerate(proposals):
            pb[n, : counts[n]] = p.proposal_boxes.tensor
        hw = K.upload([p.image_size for p in proposals], torch.int32, device)
        cnt = K.upload(counts, torch.int32, device)
        ob, os_, oi, orient2, oc = self.box_branch_batched(feats, pb, cnt, hw)
        results, _ = self.box_predictor.to_instances(ob, os_, oi, orient2, oc, [p.image_size for p in proposals])
        return results

    def _forward_recognizer(self, images: ImageList, features: Dict[str, torch.Tensor], instances: List[Instances]):
        feats = self._nhwc_feats({f: features[f] for f in self.recognizer_in_features})
        return self._recognize_into(images_nhwc4(images), feats, instances)

    def forward_with_given_boxes(self, images: ImageList, features: Dict[str, torch.Tensor], instances: List[Instances]):
        assert not self.training
        assert instances[0].has("pred_boxes") and instances[0].has("pred_classes")
        return self._forward_recognizer(images, features, instances)
