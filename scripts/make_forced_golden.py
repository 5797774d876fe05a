"""Generate tests/golden/forced_decode.npz by RUNNING THE REFERENCE's own teacher-forced forward,
`AttentionRecognitionHead.forward((x, targets, lengths))` (reference glass/modeling/recognition/prediction_aster.py:33-60).

Needs a checkout of the reference (REFERENCE_ROOT, default: where oracle/make_golden.py looks); the file is loaded by path behind the
detectron2 / fvcore shim of oracle/make_golden.py, nothing of it is copied.  Weights are not stored: the fixture records the
seed and the two edits of the beam-search golden (a sharper output layer, a boosted <eos> bias), and the tests regenerate them
with tests/beam_cases.decoder_sd.  Data only: x [3,32,256], labels [3,27] (slot 0 = [GO], the word from slot 1, as
TextEncoder.encode lays them out), logits [3,26,97].

    python scripts/make_forced_golden.py
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "glass-text-spotting_amd"))

SEED, FC_SCALE, BIAS0 = 1234, 6.0, 2.0


def main():
    from glass_amd.utils.synth import make_state_dict
    from oracle import make_golden as MG
    MG.REF = os.environ.get("REFERENCE_ROOT", MG.REF)
    MG._install_shims()
    pa = MG._load("ref_pa_forced", "glass/modeling/recognition/prediction_aster.py")
    pa.device = torch.device("cpu")
    sd = make_state_dict(SEED, parts=("recog",))
    dec = pa.AttentionRecognitionHead(num_classes=97, in_planes=256, sDim=256, attDim=256, max_len_labels=26).eval()
    dsd = {k: v.clone() for k, v in MG._sub(sd, "roi_heads.recognizer_head.decoder.recognizer.").items()}
    dsd["decoder.fc.weight"] = dsd["decoder.fc.weight"] * FC_SCALE
    dsd["decoder.fc.bias"][0] += BIAS0
    dec.load_state_dict(dsd, strict=True)
    x = MG._rand((3, 32, 256), 51)
    g = torch.Generator().manual_seed(52)
    labels = torch.randint(0, 97, (3, 27), generator=g)
    labels[:, 0] = 0
    with torch.no_grad():
        logits = dec((x, labels, 26))
    assert tuple(logits.shape) == (3, 26, 97)
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "forced_decode.npz"), seed=SEED, fc_scale=FC_SCALE, bias0=BIAS0,
                        x=x.numpy(), labels=labels.numpy().astype(np.int64), logits=logits.numpy().astype(np.float32))
    print("forced_decode.npz: logits", tuple(logits.shape), "max |logit|", float(logits.abs().max()))


if __name__ == "__main__":
    main()
