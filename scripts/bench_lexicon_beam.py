"""Lexicon-constrained beam search on one device: ASTER_V2.beam_decode(lexicon=LexiconTrie) (glass_beam_search_lexicon)
against the unconstrained ASTER_V2.beam_decode (glass_beam_search) of the same build on the same inputs, in the same process,
alternating.

The shipped decoder shape: T = 32 encoder steps, D = 256, 97 classes, 26 decoding steps; seeded random encoder outputs and
synthetic decoder weights.  Two synthetic lexicons, generated with a seed: "strong" - one segment of 100 words per image, 8
RoIs per image; "generic" - a single segment of 90,000 words.  For every (lexicon, RoIs, width):
  lexicon / free   - wall time of one call ending in a device synchronise, median and min of --reps after --warmup;
  peak extra MiB   - torch.cuda.max_memory_allocated over one call minus what was allocated before it (inputs and trie excluded);
  completed        - RoIs whose best hypothesis is a lexicon word (all of them, unless a segment is empty).
Per lexicon: the trie's nodes and bytes on the device, and its host build time.

  python scripts/bench_lexicon_beam.py [--reps 20] [--warmup 2] [--out profiles/lexicon_beam.txt]
"""
import argparse
import json
import os
import statistics
import sys
import time
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "glass-text-spotting_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np
import torch

from glass_amd.config import get_glass_cfg
from glass_amd.evaluation.lexicon import LexiconTrie
from glass_amd.modeling.recognition.recognizer_decoder import ASTER_V2
from glass_amd.modeling.recognition.text_encoder import TextEncoder
from glass_amd.structures.core import ShapeSpec
from glass_amd.utils.synth import make_state_dict

PRE = "roi_heads.recognizer_head.decoder."
C, L, T, D = 97, 26, 32, 256
ROIS_PER_IMAGE = 8


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def peak_extra_mib(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    del out
    return (peak - base) / 2 ** 20


def words(rng, n):
    """n seeded words of 2..12 letters and digits, lengths roughly as in a scene-text vocabulary"""
    al = np.array(list("abcdefghijklmnopqrstuvwxyz0123456789"))
    lens = np.clip(rng.poisson(6.0, n), 2, 12)
    return ["".join(al[rng.integers(0, len(al), int(m))]) for m in lens]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_lexicon_beam.py measures on a HIP device; none found")
    dev = torch.device("cuda:0")
    cfg = get_glass_cfg(os.path.join(ROOT, "configs", "glass_icdar15_mi355x.yaml"), ["MODEL.DEVICE", "cuda:0"])
    enc = TextEncoder(cfg)
    eos = enc.character.index("[s]")
    assert len(enc.character) == C
    rc = SimpleNamespace(CHARACTER_SET=list(enc.character[2:]), MAX_WORD_LENGTH=L - 1)
    dec = ASTER_V2(SimpleNamespace(MODEL=SimpleNamespace(ROI_RECOGNIZER_HEAD=rc)), ShapeSpec(channels=D))
    dec.import_weights(dict(make_state_dict(1234, parts=("recog",))), dev, PRE)
    rng = np.random.default_rng(2024)
    lexicons = {"strong (100 words per image)": {i: words(rng, 100) for i in range(1024 // ROIS_PER_IMAGE)},
                "generic (one segment of 90000 words)": words(rng, 90000)}
    lines = [f"lexicon-constrained beam search: T={T} D={D} classes={C} steps={L}, device {torch.cuda.get_device_name(0)}, "
             f"median (min) of {args.reps} alternating reps after {args.warmup} warm-up calls, times in ms"]
    records = []
    for name, lex in lexicons.items():
        trie = LexiconTrie(lex, enc, L, eos, device=dev)
        lines.append(f" {name}: {len(trie)} words, {trie.num_nodes} nodes, F {trie.num_fold}, {trie.mask_words} mask words per node, "
                     f"{trie.nbytes / 2 ** 20:.2f} MiB on the device, built on the host in {trie.build_seconds * 1e3:.0f} ms, "
                     f"left out {trie.skipped}")
        print(lines[-1], flush=True)
        for R in (256, 1024):
            g = torch.Generator(device="cpu")
            g.manual_seed(R)
            x = torch.randn((R, T, D), generator=g).to(dev)
            per_image = isinstance(lex, dict)
            seg = (torch.arange(R, dtype=torch.int32) // ROIS_PER_IMAGE if per_image else torch.zeros(R, dtype=torch.int32)).to(dev)
            for k in (1, 5, 8):
                lexi = lambda: dec.beam_decode(x, k, eos, path_probs=True, lexicon=trie, segments=seg)
                free = lambda: dec.beam_decode(x, k, eos, path_probs=True)
                for _ in range(args.warmup):
                    lexi(); free()
                tl, tf = [], []
                for _ in range(args.reps):
                    ms, rl = timed(lexi); tl.append(ms)
                    ms, _ = timed(free); tf.append(ms)
                done = int(torch.isfinite(rl.scores[:, 0]).sum())
                ml, mf = peak_extra_mib(lexi), peak_extra_mib(free)
                med = statistics.median
                records.append({"lexicon": name, "rois": R, "width": k, "lexicon_ms": round(med(tl), 3), "lexicon_ms_min": round(min(tl), 3),
                                "free_ms": round(med(tf), 3), "free_ms_min": round(min(tf), 3), "lexicon_peak_mib": round(ml, 1),
                                "free_peak_mib": round(mf, 1), "completed": done, "trie_nodes": trie.num_nodes,
                                "trie_bytes": trie.nbytes, "trie_build_ms": round(trie.build_seconds * 1e3, 1)})
                lines.append(f"  RoIs {R:5d} width {k}: lexicon {med(tl):8.3f} ({min(tl):8.3f})  free {med(tf):8.3f} ({min(tf):8.3f})  "
                             f"lexicon/free {med(tl) / med(tf):5.2f}x  peak extra MiB lexicon {ml:6.1f} free {mf:6.1f}  "
                             f"best hypothesis is a lexicon word for {done} of {R} RoIs")
                print(lines[-1], flush=True)
    lines.append("not measured: per-kernel times, the end-to-end step with set_lexicon, real lexicon files")
    lines.append(json.dumps({"metric": "lexicon_beam", "device": torch.cuda.get_device_name(0), "reps": args.reps, "results": records}))
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
