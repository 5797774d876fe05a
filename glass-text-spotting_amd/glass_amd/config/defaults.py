"""Config defaults for the GLASS inference path.

`get_cfg()` restates the subset of detectron2 v0.6 `config/defaults.py` that the
inference path reads [d2-recall: detectron2 is not vendored in the reference and not
installed here]; the `add_*` functions carry the same names, keys and default values as
reference glass/config.py:10-214 so that the reference's predictor set-up sequence
(glass/inference/glass_runner.py:31-39) works unchanged against this package.
"""
from __future__ import annotations

from .cfgnode import CfgNode as CN

_CHARSET = ('0123456789abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ'
            '!"#$%&\'()*+,-./:;<=>?@[\\]^_`{|}~ ')

_D2_DEFAULTS = {
    "VERSION": 2,
    "VIS_PERIOD": 0,
    "SEED": -1,
    "OUTPUT_DIR": "./output",
    "MODEL": {
        "LOAD_PROPOSALS": False, "MASK_ON": False, "KEYPOINT_ON": False,
        "DEVICE": "cuda", "META_ARCHITECTURE": "GeneralizedRCNN", "WEIGHTS": "",
        "PIXEL_MEAN": [103.530, 116.280, 123.675], "PIXEL_STD": [1.0, 1.0, 1.0],
        "BACKBONE": {"NAME": "build_resnet_backbone", "FREEZE_AT": 2},
        "FPN": {"IN_FEATURES": [], "OUT_CHANNELS": 256, "NORM": "", "FUSE_TYPE": "sum"},
        "PROPOSAL_GENERATOR": {"NAME": "RPN", "MIN_SIZE": 0},
        "ANCHOR_GENERATOR": {
            "NAME": "DefaultAnchorGenerator", "SIZES": [[32, 64, 128, 256, 512]],
            "ASPECT_RATIOS": [[0.5, 1.0, 2.0]], "ANGLES": [[-90, 0, 90]], "OFFSET": 0.0},
        "RPN": {
            "HEAD_NAME": "StandardRPNHead", "IN_FEATURES": ["res4"], "BOUNDARY_THRESH": -1,
            "IOU_THRESHOLDS": [0.3, 0.7], "IOU_LABELS": [0, -1, 1], "BATCH_SIZE_PER_IMAGE": 256,
            "POSITIVE_FRACTION": 0.5, "BBOX_REG_LOSS_TYPE": "smooth_l1",
            "BBOX_REG_LOSS_WEIGHT": 1.0, "BBOX_REG_WEIGHTS": (1.0, 1.0, 1.0, 1.0),
            "SMOOTH_L1_BETA": 0.0, "LOSS_WEIGHT": 1.0, "PRE_NMS_TOPK_TRAIN": 12000,
            "PRE_NMS_TOPK_TEST": 6000, "POST_NMS_TOPK_TRAIN": 2000, "POST_NMS_TOPK_TEST": 1000,
            "NMS_THRESH": 0.7, "CONV_DIMS": [-1]},
        "ROI_HEADS": {
            "NAME": "Res5ROIHeads", "NUM_CLASSES": 80, "IN_FEATURES": ["res4"],
            "IOU_THRESHOLDS": [0.5], "IOU_LABELS": [0, 1], "BATCH_SIZE_PER_IMAGE": 512,
            "POSITIVE_FRACTION": 0.25, "SCORE_THRESH_TEST": 0.05, "NMS_THRESH_TEST": 0.5,
            "PROPOSAL_APPEND_GT": True},
        "ROI_BOX_HEAD": {
            "NAME": "", "BBOX_REG_LOSS_TYPE": "smooth_l1", "BBOX_REG_LOSS_WEIGHT": 1.0,
            "BBOX_REG_WEIGHTS": (10.0, 10.0, 5.0, 5.0), "SMOOTH_L1_BETA": 0.0,
            "POOLER_RESOLUTION": 14, "POOLER_SAMPLING_RATIO": 0, "POOLER_TYPE": "ROIAlignV2",
            "NUM_FC": 0, "FC_DIM": 1024, "NUM_CONV": 0, "CONV_DIM": 256, "NORM": "",
            "CLS_AGNOSTIC_BBOX_REG": False, "TRAIN_ON_PRED_BOXES": False},
        "ROI_MASK_HEAD": {
            "NAME": "MaskRCNNConvUpsampleHead", "POOLER_RESOLUTION": 14,
            "POOLER_SAMPLING_RATIO": 0, "NUM_CONV": 0, "CONV_DIM": 256, "NORM": "",
            "CLS_AGNOSTIC_MASK": False, "POOLER_TYPE": "ROIAlignV2"},
        "RESNETS": {
            "DEPTH": 50, "OUT_FEATURES": ["res4"], "NUM_GROUPS": 1, "NORM": "FrozenBN",
            "WIDTH_PER_GROUP": 64, "STRIDE_IN_1X1": True, "RES5_DILATION": 1,
            "RES2_OUT_CHANNELS": 256, "STEM_OUT_CHANNELS": 64,
            "DEFORM_ON_PER_STAGE": [False, False, False, False]},
    },
    "INPUT": {
        "MIN_SIZE_TRAIN": (800,), "MIN_SIZE_TRAIN_SAMPLING": "choice", "MAX_SIZE_TRAIN": 1333,
        "MIN_SIZE_TEST": 800, "MAX_SIZE_TEST": 1333, "FORMAT": "BGR", "MASK_FORMAT": "polygon"},
    "DATASETS": {"TRAIN": (), "TEST": ()},
    "DATALOADER": {"NUM_WORKERS": 4, "ASPECT_RATIO_GROUPING": True},
    "SOLVER": {"IMS_PER_BATCH": 16},
    "TEST": {"EVAL_PERIOD": 0, "DETECTIONS_PER_IMAGE": 100},
}


def get_cfg() -> CN:
    """Work-alike of `detectron2.config.get_cfg()` for the keys the inference path reads."""
    return CN(_D2_DEFAULTS).clone()


def add_dataset_config(cfg: CN) -> None:
    """Same keys/values as reference glass/config.py:10-17 (training-side; carried only so
    reference YAML dumps merge cleanly)."""
    cfg.DATASETS.merge_from_other_cfg({
        "AUG": False, "RANDOM_CROP_PROB": 0.0, "IGNORE_DIFFICULT": False, "FIX_CROP": False,
        "CROP_SIZE": (512, 512), "MAX_ROTATE_THETA": 30, "FIX_ROTATE": False})


def add_glass_config(cfg: CN) -> None:
    """Same keys/values as reference glass/config.py:20-75."""
    cfg.MODEL.merge_from_other_cfg({
        "ROTATED_BOXES_ON": False, "ORIENTATION_ON": False,
        "ROI_HYBRID_HEAD": {"NAME": "ResBlockHybridHead", "POOLER_RESOLUTION": 64,
                            "NUM_FEATURES": 256, "DEPTH": 3, "NORM_IMG_CROPS": False},
        "FILTERED_RPN": {"IGNORE_TEXT": ["###", ""]},
        "LOCAL_FEATURE_EXTRACTOR": {"NAME": "ResNet_FeatureExtractor", "NUM_FEATURES": 256},
        "HYBRID_FUSION": {"NAME": "MultiAspectGCAttention", "NUM_FEATURES": 256, "RATIO": 0.5,
                          "HEADERS": 8, "FUSION_TYPE": "channel_add"},
        "ROI_ORIENTATION_HEAD": {"LOSS_WEIGHT": 1.0, "APPLY_TO_BOXES": False,
                                 "APPLY_TO_BOXES_DURING_TRAINING": True},
    })
    cfg.MODEL.ROI_MASK_HEAD.LOSS_WEIGHT = 0.005
    cfg.MODEL.ROI_HEADS.CLASS_NAMES = ["word"]
    cfg.INPUT.MIN_SIZE_TEST = 1600
    cfg.INPUT.MAX_SIZE_TEST = 1600
    cfg.INPUT.MAX_UPSCALE_RATIO = 2
    cfg.INPUT.merge_from_other_cfg({"ROTATION": {"ENABLED": False, "ANGLES": [0]}})
    cfg.TEST.IOU_THRESHOLD = 0.5
    cfg.TEST.USE_FILTERED_METRICS = True
    cfg.TEST.DONT_CARE_GT_LABELS = ["###", ""]


def _recognizer_block(name, backbone, encoder, decoder):
    return {
        "SAMPLE_WORDS_STRATEGY": "random", "SAMPLE_WORDS_STRATEGY_PROB": 0.3, "CLASS_IND": 0,
        "IGNORE_EMPTY_TEXT": True, "LABELS_TYPE": "attention", "MAX_WORD_LENGTH": 50,
        "CHARACTER_SET": _CHARSET, "UNK_SYMBOL_PRED": False, "POOLER_RESOLUTION_WIDTH": 32,
        "POOLER_RESOLUTION_HEIGHT": 32, "IN_FEATURES": ["p2", "p3", "p4", "p5", "p6"],
        "PAD_SAMPLER": "", "MAX_BATCH_SIZE": 256, "LOSS_WEIGHT": 2.0, "IGNORE_TEXT": ["###"],
        "SENSITIVE": True,
        "RECOGNIZER_HEAD": {
            "POOLER_PAD": {"NAME": ""},
            "BACKBONE": {"NAME": backbone},
            "ENCODER": {"NAME": encoder, "NUM_OF_LAYERS": 2, "HEIGHT_REDUCTION": "mean",
                        "N_HEAD": 8},
            "DECODER": {"NAME": decoder, "POS_ENC_HEIGHT_WIDTH": None}},
        **({"NAME": name} if name is not None else {}),
    }


def add_e2e_config(cfg: CN) -> None:
    """Same keys/values as reference glass/config.py:78-170."""
    cfg.MODEL.RECOGNIZER_ON = False
    # MI355X build only (not a reference key): "fp32" = the reference's arithmetic; "fp16" = convolutions / linears with
    # operands rounded to fp16 on the fp16 matrix cores, fp32 accumulate and storage (BASELINE.json configs[4])
    cfg.MODEL.CONV_PRECISION = "fp32"
    cfg.MODEL.ROI_MASK_HEAD.merge_from_other_cfg(
        _recognizer_block(None, "CNN_V1", "BiLSTMBlock", "ASTER"))
    cfg.MODEL.ROI_MASK_HEAD.MASK_INFERENCE = False
    # MI355X build only (not a reference key), read with MASK_INFERENCE: True = `pred_masks` is the bool [R, H, W] tensor of the
    # masks pasted over the whole image, as in the reference; False = the instances carry the RoI masks themselves,
    # `pred_mask_rois` float [R, M, M], and `pred_mask_boxes` [R, 5], the boxes they were predicted in (image pixels), which
    # `MaskPolygonizer.from_rois` turns into the same polygons: memory no longer grows with detections x image area, and the
    # two fields pass through GlassRunner.run_batch / run_tiled like any other per-detection row
    cfg.MODEL.ROI_MASK_HEAD.PASTE_MASKS = True
    blk = _recognizer_block("", "CNN_V1_2", "BiLSTMBlockV2", "ASTER_V2")
    blk.update({"POOLER_TYPE": "ROIAlignRotated", "NORM": "BN", "POOLER_SAMPLING_RATIO": 0,
                "CONV_DIM": 256, "SAMPLING_RATIO": 0})
    # MI355X build only (not a reference key): 0 = greedy decoding, the reference's inference path; k >= 1 = beam search of
    # width k on the device (ASTER_V2.beam_decode, glass_beam_search; k <= 16) - `pred_text_prob` then holds the best
    # hypothesis as path rows (one non-zero entry per step: the step's conditional probability at the emitted symbol)
    blk["BEAM_WIDTH"] = 0
    # MI355X build only: with BEAM_WIDTH >= 1 (ValueError otherwise), one forced replay of the best hypothesis
    # (glass_forced_decode) adds its FULL per-step distributions as `pred_text_dist` [Ri,L,C] - what the weighted lexicon
    # protocol reads (`character_probs`); `pred_text_prob` keeps the path rows, bit for bit
    blk["BEAM_DISTRIBUTIONS"] = False
    # MI355X build only: "" = off, nothing changes; a regex (the subset of evaluation/pattern.py) = with BEAM_WIDTH >= 1
    # (ValueError otherwise) the head builds a one-segment, case-sensitive DecodePattern at construction and the search can only
    # spell strings the regex accepts (RecognizerRCNNHeadV3.set_pattern, glass_beam_search_dfa)
    blk["DECODE_PATTERN"] = ""
    # MI355X build only: 0.0 = off, nothing changes; else (with DECODE_PATTERN; ValueError otherwise) a bonus per character, a
    # natural log, on the pattern's transitions: the search ranks by the model score + the bonus times the characters
    # (DecodePattern.weighted(length_bonus=...), glass_beam_search_wdfa); the word score stays the model's probability
    blk["DECODE_LENGTH_BONUS"] = 0.0
    # MI355X build only: False = off, nothing changes; True (with DECODE_PATTERN; ValueError otherwise) = the head builds its
    # pattern with case_insensitive=True and the search merges the two cases of a letter into one candidate per beam
    # (RecognizerRCNNHeadV3.set_pattern(merge_case=True), include/glass_hip_feature_merged.h): k distinct folded strings, and
    # the word score is the probability of the word, not of one casing
    blk["DECODE_MERGE_CASE"] = False
    # MI355X build only: False = off, no launch and no field is added; True = the head replays the emitted symbols once
    # (glass_forced_attention; with BEAM_DISTRIBUTIONS the same replay supplies `pred_text_dist`), turns the decoder's attention
    # rows into spans along the pooled box (glass_char_spans, include/glass_hip_feature_chars.h) and every Instances carries
    # pred_char_spans / pred_char_centres / pred_char_count / pred_char_monotone / pred_char_frames
    # (glass_amd.postprocess.char_quads and chars_of give the quads and the characters)
    blk["CHAR_BOXES"] = False
    cfg.MODEL.merge_from_other_cfg({"ROI_RECOGNIZER_HEAD": blk})


def add_post_process_config(cfg: CN) -> None:
    """Same keys/values as reference glass/config.py:173-214."""
    cfg.merge_from_other_cfg({"POST_PROCESSING": {
        "NAME": "PostProcessorAcademic", "SKIP_ALL": False, "BOX_INFLATE_RATIO": 0.05,
        "BOX_PX_PADDING": [0, 0, 0, 0], "MIN_BOX_DIMENSION": 2, "MAX_OUTSIDE_BOX_MARGIN_PX": 5,
        "MERGE_IOA_THRESH": 0.3, "OVERLAP_WIDTH_PER_HEIGHT_THRESH": 0.3,
        "PAIRS_HEIGHT_RATIO_THRESH": 0.35, "LOW_CONFIDENCE": 0.01, "VALID_CONFIDENCE": 0.15,
        "DETECT_THRESHOLD": 0.25, "TEXT_THRESHOLD": 0.25, "MAX_ANGLE_DIFF": 15,
        # MI355X build only: False = off, nothing changes; True = the surviving words of every image are grouped into text
        # lines in reading order on the device, right after the word kernel (ops.native.group_lines; the thresholds below
        # are those of include/glass_hip_feature_lines.h), and every Instances carries pred_line_ids / pred_line_pos /
        # pred_reading_rank / pred_line_boxes (glass_amd.postprocess.lines_of gives the lines on the host)
        "GROUP_LINES": False, "LINE_MAX_ANGLE_DIFF": 15.0, "LINE_MIN_HEIGHT_RATIO": 0.5, "LINE_MAX_OFFSET": 0.5,
        "LINE_MAX_GAP": 1.0,
        # with GROUP_LINES only (a ValueError without): True = the lines are also ordered column by column and cut into blocks
        # on the device, right behind the line grouping (ops.native.order_lines; the thresholds are those of
        # include/glass_hip_feature_layout.h), and every Instances carries pred_page_rank / pred_block_ids / pred_block_boxes
        # (glass_amd.postprocess.blocks_of and page_text give the blocks and the text on the host)
        "ORDER_LINES": False, "ORDER_MIN_OVERLAP": 0.1, "BLOCK_MAX_GAP": 0.8, "BLOCK_MIN_HEIGHT_RATIO": 0.7,
        # with GROUP_LINES only (a ValueError without; ORDER_LINES is not needed): True = the lines are also aligned into rows,
        # cells, tables and columns on the device, behind the line grouping and the page order (ops.native.row_grid; the
        # thresholds are those of include/glass_hip_feature_grid.h), and every Instances carries pred_row_ids / pred_row_pos /
        # pred_table_ids / pred_col_ids / pred_row_rank / pred_row_boxes / pred_table_boxes (glass_amd.postprocess.rows_of,
        # tables_of and rows_text give the rows, the tables and the text on the host)
        "ALIGN_ROWS": False, "ROW_MIN_OVERLAP": 0.5, "ROW_MIN_HEIGHT_RATIO": 0.5, "COLUMN_MIN_OVERLAP": 0.1,
        "TABLE_MAX_ROW_GAP": 2.0}})


def get_glass_cfg(config_path: str = None, opts=None) -> CN:
    """The reference predictor's cfg set-up (glass/inference/glass_runner.py:31-39) in one call."""
    cfg = get_cfg()
    add_e2e_config(cfg)
    add_glass_config(cfg)
    add_dataset_config(cfg)
    add_post_process_config(cfg)
    if config_path:
        cfg.merge_from_file(config_path)
    cfg.merge_from_list(list(opts or []))
    return cfg
