"""Recognizer head (`RecognizerRCNNHeadV3`): CNN -> BiLSTM encoder -> attention decoder.

Mirrors reference glass/modeling/recognition/recognizer_head_v2.py:291-345 and the eval branch
of `BaseRecognizerRCNNHead.forward` (:150-163): empty input returns the instances untouched,
otherwise `pred_text_prob` [Ri,26,97] is attached per image.
"""
from __future__ import annotations

from typing import List

import torch

from ...ops import native as K
from ...utils.module import InferenceModule

from ...structures.core import Instances
from ...utils.registry import Registry
from .recognizer_backbone import build_recognizer_backbonev2
from .recognizer_decoder import build_recognizer_decoderv2
from .recognizer_encoder import build_recognizer_encoderv2
from .text_encoder import TextEncoder

ROI_RECOGNIZER_HEAD_REGISTRY = Registry("ROI_RECOGNIZER_HEAD")


@ROI_RECOGNIZER_HEAD_REGISTRY.register()
class RecognizerRCNNHeadV3(InferenceModule):
    def __init__(self, cfg, input_shape):
        super().__init__()
        self.backbone = build_recognizer_backbonev2(cfg, input_shape)
        self.encoder = build_recognizer_encoderv2(cfg, input_shape)
        self.decoder = build_recognizer_decoderv2(cfg, input_shape)
        self.max_word_length = cfg.MODEL.ROI_RECOGNIZER_HEAD.MAX_WORD_LENGTH
        self.class_ind = cfg.MODEL.ROI_RECOGNIZER_HEAD.CLASS_IND
        self.text_encoder = TextEncoder(cfg)
        # MI355X build only: 0 = greedy decoding (the reference's path), k >= 1 = beam search of width k on the device
        self.beam_width = int(getattr(cfg.MODEL.ROI_RECOGNIZER_HEAD, "BEAM_WIDTH", 0))
        if not 0 <= self.beam_width <= 16:
            raise ValueError(f"MODEL.ROI_RECOGNIZER_HEAD.BEAM_WIDTH must be in 0..16 (got {self.beam_width})")
        # a hypothesis ends where the word post-processing stops reading: at the text encoder's stop symbol ('[s]'), so the
        # word score the consumers of `pred_text_prob` compute from the path rows is exp(score of the best hypothesis)
        ch = self.text_encoder.character
        self.beam_eos = ch.index("[s]") if "[s]" in ch else 0
        # MI355X build only: with the search, also the best hypothesis's FULL per-step distributions (one forced replay,
        # ASTER_V2.beam_decode(distributions="best")) as `pred_text_dist`, next to the path rows in `pred_text_prob`
        self.beam_distributions = bool(getattr(cfg.MODEL.ROI_RECOGNIZER_HEAD, "BEAM_DISTRIBUTIONS", False))
        if self.beam_distributions and self.beam_width < 1:
            raise ValueError("MODEL.ROI_RECOGNIZER_HEAD.BEAM_DISTRIBUTIONS needs MODEL.ROI_RECOGNIZER_HEAD.BEAM_WIDTH >= 1 "
                             f"(got BEAM_WIDTH {self.beam_width}): the greedy decoder's pred_text_prob already holds full rows")
        # MI355X build only: a non-empty regex constrains the search to it from construction on (set_pattern with a
        # one-segment evaluation.pattern.DecodePattern, case-sensitive unless DECODE_MERGE_CASE)
        regex = str(getattr(cfg.MODEL.ROI_RECOGNIZER_HEAD, "DECODE_PATTERN", "") or "")
        # MI355X build only: with DECODE_PATTERN, the pattern is built case-insensitive and the search merges the two cases of
        # a letter into one candidate (set_pattern(merge_case=True), include/glass_hip_feature_merged.h): the word score is the
        # probability of the word, not of one casing
        merge = bool(getattr(cfg.MODEL.ROI_RECOGNIZER_HEAD, "DECODE_MERGE_CASE", False))
        if merge and not regex:
            raise ValueError("MODEL.ROI_RECOGNIZER_HEAD.DECODE_MERGE_CASE needs MODEL.ROI_RECOGNIZER_HEAD.DECODE_PATTERN "
                             "(the merged search runs on a pattern)")
        if regex:
            if self.beam_width < 1:
                raise ValueError("MODEL.ROI_RECOGNIZER_HEAD.DECODE_PATTERN needs MODEL.ROI_RECOGNIZER_HEAD.BEAM_WIDTH >= 1 "
                                 f"(got BEAM_WIDTH {self.beam_width}): the greedy decoder does not search")
            from ...evaluation.pattern import DecodePattern
            self.set_pattern(DecodePattern(regex, self.text_encoder, self.decoder.max_word_len, self.beam_eos,
                                           case_insensitive=merge, device=cfg.MODEL.DEVICE), merge_case=merge)
        # MI355X build only: with DECODE_PATTERN, a non-zero bonus per character (a natural log) makes the pattern a
        # WeightedPattern: the search ranks by the model score + the bonus times the characters (glass_beam_search_wdfa)
        bonus = float(getattr(cfg.MODEL.ROI_RECOGNIZER_HEAD, "DECODE_LENGTH_BONUS", 0.0) or 0.0)
        if bonus != 0.0:
            if not regex:
                raise ValueError("MODEL.ROI_RECOGNIZER_HEAD.DECODE_LENGTH_BONUS needs MODEL.ROI_RECOGNIZER_HEAD.DECODE_PATTERN "
                                 "(the bonus is a weight on the pattern's transitions)")
            self.set_pattern(self.pattern.weighted(length_bonus=bonus), merge_case=merge)

        # MI355X build only: one forced replay of the emitted symbols (glass_forced_attention) and glass_char_spans add where
        # inside the pooled box every character lies (postprocess/char_boxes.py); off: no launch and no field is added
        self.char_boxes = bool(getattr(cfg.MODEL.ROI_RECOGNIZER_HEAD, "CHAR_BOXES", False))

    def import_weights(self, sd, device, prefix: str) -> None:
        self.backbone.import_weights(sd, device, prefix + "backbone.")
        self.encoder.import_weights(sd, device, prefix + "encoder.")
        self.decoder.import_weights(sd, device, prefix + "decoder.")

    lexicon = None            # set_lexicon: the LexiconTrie the search is constrained to
    image_segments = None     # set_lexicon: int32 [num_images] on the device, the lexicon segment of every image of a call

    def set_lexicon(self, trie, image_segments=None, merge_case: bool = False) -> None:
        """Constrain the decoding to a lexicon (evaluation.lexicon.LexiconTrie; None switches it off): every RoI decodes to
        the most likely word of its image's segment (glass_beam_search_lexicon), handed on as path rows exactly as the
        unconstrained search's - a RoI for which no word completes gets all-zero rows (an empty text with score 0).
        `image_segments`: int32 [num_images] on the device (default: segment 0 for every image); it is gathered by the
        RoIs' image ids on the device.  `merge_case`: the fold-merged search (set_pattern has the meaning) - it runs on the
        pattern tables, so the head goes through `set_pattern(DecodePattern.from_trie(trie), merge_case=True)`: `pattern` is
        set, `lexicon` stays None.  ValueError unless BEAM_WIDTH >= 1, and if the trie does not fit the decoder."""
        if trie is not None and merge_case:
            if self.lexicon is not None:
                raise ValueError("set_lexicon(merge_case=True): a lexicon is set (set_lexicon(None) first)")
            from ...evaluation.pattern import DecodePattern
            self.set_pattern(None)
            self.set_pattern(DecodePattern.from_trie(trie), image_segments, merge_case=True)
            return
        if trie is None:
            self.lexicon = None
            if self.pattern is None:            # (a pattern's segments are its own)
                self.image_segments = None
            return
        if self.pattern is not None:
            raise ValueError("set_lexicon: a pattern is set (set_pattern(None) first; DecodePattern.from_trie turns a lexicon "
                             "into a pattern)")
        if self.beam_width < 1:
            raise ValueError(f"set_lexicon needs MODEL.ROI_RECOGNIZER_HEAD.BEAM_WIDTH >= 1 (got {self.beam_width}): the greedy "
                             "decoder does not search")
        for name, have, want in (("classes", trie.num_classes, self.decoder.num_classes), ("max_len", trie.max_len, self.decoder.max_word_len),
                                 ("eos", trie.eos, self.beam_eos)):
            if have != want:
                raise ValueError(f"set_lexicon: the lexicon trie was built for {name} = {have}, the head has {want}")
        if image_segments is not None:
            if (not torch.is_tensor(image_segments) or image_segments.device.type == "cpu" or image_segments.dtype != torch.int32
                    or image_segments.dim() != 1):
                raise ValueError("set_lexicon: image_segments must be an int32 [num_images] tensor on the device")
        self.lexicon, self.image_segments = trie, image_segments

    pattern = None            # set_pattern: the DecodePattern the search is constrained to (image_segments: its segments)
    weight_scale = 1.0        # set_pattern: the factor of a WeightedPattern's weights in the score the search ranks by
    merge_case = False        # set_pattern: the search merges the classes of a fold symbol (a letter's two cases)

    def set_pattern(self, pattern, image_segments=None, weight_scale: float = 1.0, merge_case: bool = False) -> None:
        """Constrain the decoding to a pattern (evaluation.pattern.DecodePattern; None switches it off): every RoI decodes to
        the most likely string its image's segment accepts (glass_beam_search_dfa), handed on as path rows exactly as the
        unconstrained search's - a RoI with no hypothesis gets all-zero rows.  `image_segments` as in set_lexicon.
        With a `WeightedPattern` (glass_beam_search_wdfa) the best string is the one with the highest model score +
        `weight_scale` * weights; its path rows are still the model's conditional probabilities, so the word score read from
        them stays a probability.
        `merge_case` (ASTER_V2.beam_decode(merge_case=True), include/glass_hip_feature_merged.h): the classes of a fold symbol
        are one candidate per beam - with a case-insensitive pattern the path rows hold, at the likelier casing of every
        position, the summed conditional probability of both, and the word score is the probability of the word.
        ValueError unless BEAM_WIDTH >= 1, if the pattern does not fit the decoder, and while a lexicon is set."""
        if pattern is None:
            self.pattern = self.image_segments = None
            self.weight_scale = 1.0
            self.merge_case = False
            return
        if self.lexicon is not None:
            raise ValueError("set_pattern: a lexicon is set (set_lexicon(None) first)")
        if self.beam_width < 1:
            raise ValueError(f"set_pattern needs MODEL.ROI_RECOGNIZER_HEAD.BEAM_WIDTH >= 1 (got {self.beam_width}): the greedy "
                             "decoder does not search")
        for name, have, want in (("classes", pattern.num_classes, self.decoder.num_classes),
                                 ("max_len", pattern.max_len, self.decoder.max_word_len), ("eos", pattern.eos, self.beam_eos)):
            if have != want:
                raise ValueError(f"set_pattern: the pattern was built for {name} = {have}, the head has {want}")
        if image_segments is not None:
            if (not torch.is_tensor(image_segments) or image_segments.device.type == "cpu" or image_segments.dtype != torch.int32
                    or image_segments.dim() != 1):
                raise ValueError("set_pattern: image_segments must be an int32 [num_images] tensor on the device")
        self.pattern, self.image_segments, self.weight_scale = pattern, image_segments, float(weight_scale)
        self.merge_case = bool(merge_case)

    def _roi_segments(self, roi_image: torch.Tensor, num_images: int) -> torch.Tensor:
        if self.image_segments is None:
            return torch.zeros_like(roi_image)
        if self.image_segments.shape[0] < num_images:
            raise ValueError(f"image_segments of {self.image_segments.shape[0]} images for a call of {num_images}")
        return self.image_segments.index_select(0, roi_image.long()).contiguous()

    rnn_override = None       # "steps" once K.HandoffGuard.STICKY_AFTER hand-off give-ups were seen by this head
    rnn_giveups = 0

    def forward_nhwc(self, x: torch.Tensor, roi_image: torch.Tensor, num_images: int, guard=None):
        """x [R,8,32,256] fused features -> probabilities [R,26,97] (BEAM_WIDTH >= 1: the best hypothesis's path rows; with
        BEAM_DISTRIBUTIONS the pair (path rows, full distributions [R,26,97] of the best hypothesis) - `split_text_rows`; with
        CHAR_BOXES the triple (rows, distributions | None, the packed character rows [R,27,3] of postprocess.char_boxes.pack_chars)).
        `guard` (ops.native.HandoffGuard): the one-launch BiLSTM / decoder kernels report a hand-off that gave up into
        `guard.status`, and `guard.retry` re-runs encoder + decoder of THIS call on the step kernels - the caller resolves the
        guard at its next host read-back (GeneralizedRCNN._postprocess_batched_g: the surviving-count read).  Without a guard
        the status is read here (one small synchronising copy): no path returns text from a dead hand-off."""
        f = self.backbone.forward_nhwc(x)
        own = guard is None
        if own:
            guard = K.HandoffGuard(x.device, owner=self)
        elif guard.owner is None:
            guard.owner = self

        def run(rnn, status):
            enc = self.encoder.forward_nhwc(f, rnn=rnn, status=status)
            if self.beam_width > 0:         # the search has no in-kernel hand-off: only the encoder is guarded
                lex = {} if self.lexicon is None else {"lexicon": self.lexicon, "segments": self._roi_segments(roi_image, num_images)}
                if self.pattern is not None:
                    lex = {"pattern": self.pattern, "segments": self._roi_segments(roi_image, num_images),
                           "weight_scale": self.weight_scale}
                    if self.merge_case:
                        lex["merge_case"] = True
                if self.char_boxes:
                    # ONE replay of the best hypothesis (the search's own symbols and lengths, which the arg-max of its path
                    # rows up to the first stop spells): its attention rows and, with BEAM_DISTRIBUTIONS, its distributions
                    r = self.decoder.beam_decode(enc, self.beam_width, self.beam_eos, path_probs=True, attention=True,
                                                 distributions="best" if self.beam_distributions else None, **lex)
                    ln = torch.where(torch.isneginf(r.scores[:, 0]), torch.zeros_like(r.lengths[:, 0]), r.lengths[:, 0])
                    return r.path_probs, r.distributions, self._char_rows(r.attention, r.symbols[:, 0], ln)
                if self.beam_distributions:
                    r = self.decoder.beam_decode(enc, self.beam_width, self.beam_eos, path_probs=True, distributions="best", **lex)
                    return r.path_probs, r.distributions
                return self.decoder.beam_decode(enc, self.beam_width, self.beam_eos, path_probs=True, **lex).path_probs
            rows = self.decoder(enc, roi_image=roi_image, num_images=num_images, rnn=rnn, status=status)
            if self.char_boxes:
                # the emitted symbols = the arg-max of the greedy rows, replayed once up to the first stop symbol
                sym = rows.argmax(dim=-1).to(torch.int32)
                replay = self.decoder.score(enc, sym, None, eos=self.beam_eos, attention=True)
                return rows, None, self._char_rows(replay.attention, sym, replay.lengths)
            return rows
        if self.rnn_override == "steps":
            return run("steps", None)
        out = run(None, guard.status)
        guard.retry = lambda: run("steps", None)
        if own:
            again = guard.resolve(guard.status.item())
            return out if again is None else again
        return out

    def _char_rows(self, attention: torch.Tensor, symbols: torch.Tensor, lengths: torch.Tensor) -> torch.Tensor:
        """attention rows [R,L,T] of the replay, its symbols [R,L] and lengths [R] -> the packed character rows [R,L+1,3]"""
        from ...postprocess.char_boxes import pack_chars
        return pack_chars(K.char_spans(attention.contiguous(), symbols.contiguous(), lengths.contiguous(), self.beam_eos))

    def forward(self, x: torch.Tensor, instances: List[Instances]):
        assert not self.training, "inference only"
        if x.shape[0] == 0:
            return instances
        if self.char_boxes:
            raise NotImplementedError("MODEL.ROI_RECOGNIZER_HEAD.CHAR_BOXES: the list-wise forward(x, instances) does not know the "
                                      "boxes that were pooled; the batched path (GeneralizedRCNN.inference) carries the fields")
        from ..backbone.resnet_fpn import as_nhwc
        counts = [len(i) for i in instances]
        roi_image = K.upload(torch.repeat_interleave(torch.arange(len(counts), dtype=torch.int32), torch.tensor(counts)),
                             torch.int32, x.device)
        preds, dist = split_text_rows(self.forward_nhwc(as_nhwc(x), roi_image, len(counts)))
        for p, inst in zip(preds.split(counts, dim=0), instances):
            inst.pred_text_prob = p
        if dist is not None:
            for d, inst in zip(dist.split(counts, dim=0), instances):
                inst.pred_text_dist = d
        return instances


def split_text_rows(out, chars: bool = False):
    """what `RecognizerRCNNHeadV3.forward_nhwc` returned -> (pred_text_prob rows, pred_text_dist rows | None); with `chars` a third
    member: the packed character rows of CHAR_BOXES (postprocess.char_boxes.pack_chars) | None"""
    rows = tuple(out) if isinstance(out, tuple) else (out,)
    rows = rows + (None,) * (3 - len(rows))
    return rows if chars else rows[:2]


def build_recognizer_head(cfg, input_shape):
    return ROI_RECOGNIZER_HEAD_REGISTRY.get(cfg.MODEL.ROI_RECOGNIZER_HEAD.NAME)(cfg, input_shape)
