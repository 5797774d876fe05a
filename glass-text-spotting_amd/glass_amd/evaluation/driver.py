"""`inference_on_dataset`: the loop of the evaluation protocol (detectron2 evaluation/evaluator.py inference_on_dataset
[d2-recall], as tools/eval_glass.py drives it) without a data loader: map, batch, run, hand to the writer."""
from __future__ import annotations

from typing import Callable, Dict, List, Optional, Sequence


def inference_on_dataset(model, dataset_dicts: Sequence[Dict], mapper: Callable[[Dict], Dict], writer=None,
                         batch_size: int = 8, lexicon=None, lexicon_key: Optional[Callable[[Dict], object]] = None, pattern=None,
                         pattern_key: Optional[Callable[[Dict], object]] = None, merge_case: bool = False) -> List[Dict]:
    """Run `model` over `dataset_dicts` and return its per-image outputs in input order.

    The reference evaluates one image per call.  Here up to `batch_size` images share a call, grouped by their own padded
    shape (multiple of the backbone's size divisibility) as GlassRunner.run_batch groups them: detectron2 pads a batch to
    its largest image and the pad region is visible to the backbone and the RPN, so only images of one padded shape give
    per-image results that do not depend on the batch.  `writer` (evaluation.TextResultWriter, or anything with
    `process(inputs, outputs)`) sees every call's inputs and outputs.

    `lexicon` (evaluation.lexicon.LexiconTrie): lexicon-constrained decoding - the recognizer head is switched to the trie
    (`RecognizerRCNNHeadV3.set_lexicon`, which needs BEAM_WIDTH >= 1) for the run and back to what it had afterwards; every
    word the model emits is then a word of the lexicon.  `lexicon_key` (mapped input -> key of a dict lexicon, e.g. the
    image id of the per-image strong lexicons): the segments of a call's images are set right before the call; without it
    every image decodes against segment 0.

    `pattern` (evaluation.pattern.DecodePattern) / `pattern_key`: the same for pattern-constrained decoding
    (`RecognizerRCNNHeadV3.set_pattern`); a pattern the head had before (MODEL.ROI_RECOGNIZER_HEAD.DECODE_PATTERN) is put back
    afterwards.  Not together with `lexicon`.  A `WeightedPattern` (evaluation.weighted_pattern) is taken as it is, with
    weight_scale 1; the head's own scale is put back with its pattern.

    `merge_case` (with `lexicon` or `pattern`; ValueError otherwise): the fold-merged search
    (`set_pattern(..., merge_case=True)` / `set_lexicon(..., merge_case=True)`, which goes through `DecodePattern.from_trie`) -
    with a case-insensitive table a word's casings are one hypothesis and the word score is the probability of the word."""
    assert batch_size >= 1
    if merge_case and lexicon is None and pattern is None:
        raise ValueError("merge_case without a lexicon or a pattern")
    if lexicon is None and lexicon_key is not None:
        raise ValueError("lexicon_key without a lexicon")
    if pattern is None and pattern_key is not None:
        raise ValueError("pattern_key without a pattern")
    if lexicon is not None and pattern is not None:
        raise ValueError("lexicon and pattern together")
    head = None
    if lexicon is not None or pattern is not None:
        import torch
        from ..ops import native
        head = model.roi_heads.recognizer_head
        before = (head.lexicon, head.pattern, head.image_segments, head.weight_scale, head.merge_case)
        head.lexicon = head.pattern = head.image_segments = None
        try:
            if lexicon is not None:
                head.set_lexicon(lexicon, merge_case=bool(merge_case))
            else:
                head.set_pattern(pattern, merge_case=bool(merge_case))
        except Exception:
            head.lexicon, head.pattern, head.image_segments, head.weight_scale, head.merge_case = before
            raise
    table, table_key = (lexicon, lexicon_key) if lexicon is not None else (pattern, pattern_key)
    d = model.backbone.size_divisibility
    outputs: List[Optional[Dict]] = [None] * len(dataset_dicts)
    pending: Dict[tuple, List[tuple]] = {}

    def run(group: List[tuple]) -> None:
        inputs = [inp for _, inp in group]
        if table_key is not None:
            segments = [table.segment(table_key(inp)) for inp in inputs]
            head.image_segments = native.upload(segments, torch.int32, table.device)
        outs = list(model(inputs))
        assert len(outs) == len(inputs)
        if writer is not None:
            writer.process(inputs, outs)
        for (i, _), o in zip(group, outs):
            outputs[i] = o

    try:
        for i, dd in enumerate(dataset_dicts):
            inp = mapper(dd)
            h, w = model.input_size(inp)
            key = ((h + d - 1) // d * d, (w + d - 1) // d * d)
            group = pending.setdefault(key, [])
            group.append((i, inp))
            if len(group) >= batch_size:      # run as soon as a group is full: at most batch_size images per shape are held
                run(pending.pop(key))
        for group in pending.values():
            run(group)
    finally:
        if head is not None:
            head.lexicon, head.pattern, head.image_segments, head.weight_scale, head.merge_case = before
    return outputs
