"""`inference_on_dataset`: the loop of the evaluation protocol (detectron2 evaluation/evaluator.py inference_on_dataset
[d2-recall], as tools/eval_glass.py drives it) without a data loader: map, batch, run, hand to the writer."""
from __future__ import annotations

from typing import Callable, Dict, List, Optional, Sequence


def inference_on_dataset(model, dataset_dicts: Sequence[Dict], mapper: Callable[[Dict], Dict], writer=None,
                         batch_size: int = 8) -> List[Dict]:
    """Run `model` over `dataset_dicts` and return its per-image outputs in input order.

    The reference evaluates one image per call.  Here up to `batch_size` images share a call, grouped by their own padded
    shape (multiple of the backbone's size divisibility) as GlassRunner.run_batch groups them: detectron2 pads a batch to
    its largest image and the pad region is visible to the backbone and the RPN, so only images of one padded shape give
    per-image results that do not depend on the batch.  `writer` (evaluation.TextResultWriter, or anything with
    `process(inputs, outputs)`) sees every call's inputs and outputs."""
    assert batch_size >= 1
    d = model.backbone.size_divisibility
    outputs: List[Optional[Dict]] = [None] * len(dataset_dicts)
    pending: Dict[tuple, List[tuple]] = {}

    def run(group: List[tuple]) -> None:
        inputs = [inp for _, inp in group]
        outs = list(model(inputs))
        assert len(outs) == len(inputs)
        if writer is not None:
            writer.process(inputs, outs)
        for (i, _), o in zip(group, outs):
            outputs[i] = o

    for i, dd in enumerate(dataset_dicts):
        inp = mapper(dd)
        h, w = model.input_size(inp)
        key = ((h + d - 1) // d * d, (w + d - 1) // d * d)
        group = pending.setdefault(key, [])
        group.append((i, inp))
        if len(group) >= batch_size:          # run as soon as a group is full: at most batch_size images per shape are held
            run(pending.pop(key))
    for group in pending.values():
        run(group)
    return outputs
