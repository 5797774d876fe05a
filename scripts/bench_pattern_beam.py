"""Pattern-constrained beam search on one device: ASTER_V2.beam_decode(pattern=DecodePattern) (glass_beam_search_dfa) against
the lexicon-constrained search (glass_beam_search_lexicon, on a 90,000-word trie) and the unconstrained one (glass_beam_search)
of the same build on the same inputs, in the same process, alternating.

The shipped decoder shape: T = 32 encoder steps, D = 256, 97 classes, 26 decoding steps; seeded random encoder outputs and
synthetic decoder weights.  Patterns: the regexes [0-9]+ and [A-Za-z0-9]+ (case-sensitive), and the 90,000-word synthetic
lexicon of scripts/bench_lexicon_beam.py turned into a DFA with DecodePattern.from_trie (a dense table of nodes x F entries).
For every (pattern, RoIs, width):
  pattern / lexicon / free - wall time of one call ending in a device synchronise, median and min of --reps after --warmup;
  completed                - RoIs whose best hypothesis exists.
Per pattern: states, fold symbols, bytes on the device and the host build time (for from_trie: of the table, the trie aside).

  python scripts/bench_pattern_beam.py [--reps 20] [--warmup 2] [--out profiles/pattern_beam.txt]
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
from glass_amd.evaluation.pattern import DecodePattern
from glass_amd.modeling.recognition.recognizer_decoder import ASTER_V2
from glass_amd.modeling.recognition.text_encoder import TextEncoder
from glass_amd.structures.core import ShapeSpec
from glass_amd.utils.synth import make_state_dict

PRE = "roi_heads.recognizer_head.decoder."
C, L, T, D = 97, 26, 32, 256


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def words(rng, n):
    """n seeded words of 2..12 letters and digits (scripts/bench_lexicon_beam.py)"""
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
        raise SystemExit("bench_pattern_beam.py measures on a HIP device; none found")
    dev = torch.device("cuda:0")
    cfg = get_glass_cfg(os.path.join(ROOT, "configs", "glass_icdar15_mi355x.yaml"), ["MODEL.DEVICE", "cuda:0"])
    enc = TextEncoder(cfg)
    eos = enc.character.index("[s]")
    assert len(enc.character) == C
    rc = SimpleNamespace(CHARACTER_SET=list(enc.character[2:]), MAX_WORD_LENGTH=L - 1)
    dec = ASTER_V2(SimpleNamespace(MODEL=SimpleNamespace(ROI_RECOGNIZER_HEAD=rc)), ShapeSpec(channels=D))
    dec.import_weights(dict(make_state_dict(1234, parts=("recog",))), dev, PRE)
    trie = LexiconTrie(words(np.random.default_rng(2024), 90000), enc, L, eos, device=dev)
    patterns = {"[0-9]+": DecodePattern(r"[0-9]+", enc, L, eos, device=dev),
                "[A-Za-z0-9]+": DecodePattern(r"[A-Za-z0-9]+", enc, L, eos, device=dev),
                "from_trie (90000 words)": DecodePattern.from_trie(trie)}
    lines = [f"pattern-constrained beam search: T={T} D={D} classes={C} steps={L}, device {torch.cuda.get_device_name(0)}, "
             f"median (min) of {args.reps} alternating reps after {args.warmup} warm-up calls, times in ms",
             f" the lexicon search's trie: {len(trie)} words, {trie.num_nodes} nodes, F {trie.num_fold}, {trie.nbytes / 2 ** 20:.2f} MiB "
             f"on the device, built on the host in {trie.build_seconds * 1e3:.0f} ms"]
    records = []
    for name, pat in patterns.items():
        lines.append(f" {name}: {pat.num_states} states, F {pat.num_fold}, {pat.nbytes / 2 ** 20:.3f} MiB on the device "
                     f"({pat.next.nbytes} bytes of transitions), built on the host in {pat.build_seconds * 1e3:.1f} ms")
        print(lines[-1], flush=True)
        for R in (256, 1024):
            g = torch.Generator(device="cpu")
            g.manual_seed(R)
            x = torch.randn((R, T, D), generator=g).to(dev)
            seg = torch.zeros(R, dtype=torch.int32).to(dev)
            for k in (1, 5, 8):
                dfa = lambda: dec.beam_decode(x, k, eos, path_probs=True, pattern=pat, segments=seg)
                lexi = lambda: dec.beam_decode(x, k, eos, path_probs=True, lexicon=trie, segments=seg)
                free = lambda: dec.beam_decode(x, k, eos, path_probs=True)
                for _ in range(args.warmup):
                    dfa(); lexi(); free()
                td, tl, tf = [], [], []
                for _ in range(args.reps):
                    ms, rd = timed(dfa); td.append(ms)
                    ms, _ = timed(lexi); tl.append(ms)
                    ms, _ = timed(free); tf.append(ms)
                done = int(torch.isfinite(rd.scores[:, 0]).sum())
                med = statistics.median
                records.append({"pattern": name, "rois": R, "width": k, "pattern_ms": round(med(td), 3), "pattern_ms_min": round(min(td), 3),
                                "lexicon_ms": round(med(tl), 3), "lexicon_ms_min": round(min(tl), 3), "free_ms": round(med(tf), 3),
                                "free_ms_min": round(min(tf), 3), "completed": done, "states": pat.num_states, "fold": pat.num_fold,
                                "bytes": pat.nbytes, "build_ms": round(pat.build_seconds * 1e3, 2)})
                lines.append(f"  RoIs {R:5d} width {k}: pattern {med(td):8.3f} ({min(td):8.3f})  lexicon {med(tl):8.3f} ({min(tl):8.3f})  "
                             f"free {med(tf):8.3f} ({min(tf):8.3f})  pattern/lexicon {med(td) / med(tl):5.2f}x  pattern/free "
                             f"{med(td) / med(tf):5.2f}x  best hypothesis exists for {done} of {R} RoIs")
                print(lines[-1], flush=True)
    lines.append("not measured: per-kernel times, the end-to-end step with set_pattern / DECODE_PATTERN, automata whose live states "
                 "are spread over a table larger than the caches (from_trie's beams sit in neighbouring nodes), real lexicon files")
    lines.append(json.dumps({"metric": "pattern_beam", "device": torch.cuda.get_device_name(0), "reps": args.reps, "results": records}))
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
