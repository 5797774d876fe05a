"""Fold-merged constrained beam search on one device: ASTER_V2.beam_decode(pattern=..., merge_case=True)
(glass_beam_search_merged_dfa / glass_beam_search_merged_wdfa) against the unmerged search on the SAME case-insensitive pattern
(glass_beam_search_dfa / glass_beam_search_wdfa), from the same build on the same inputs, in the same process, alternating.  The
unmerged lines can be set against profiles/weighted_beam.txt: the step kernel the searches share did not slow.

The shipped decoder shape: T = 32 encoder steps, D = 256, 97 classes, 26 decoding steps; seeded random encoder outputs and
synthetic decoder weights (scripts/bench_weighted_beam.py).  Automata, all case-insensitive (a letter's two cases are one fold
symbol, so the merge has 26 groups of two):
  [A-Za-z0-9]+;
  the 90,000-word synthetic lexicon as a DFA (DecodePattern.from_trie);
  [A-Za-z0-9]+ crossed with a character trigram model estimated on upper-cased words (weighted, weight_scale 1).
For every (automaton, RoIs, width):
  merged / unmerged - wall time of one call ending in a device synchronise, median and min of --reps after --warmup;
  twins             - the share of the unmerged run's finite result slots whose folded string an earlier slot of the same RoI
                      already holds: what the merge frees; the same count on the merged run (the invariant: always 0).

  python scripts/bench_merged_beam.py [--reps 20] [--warmup 2] [--out profiles/merged_beam.txt]
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
from glass_amd.evaluation.weighted_pattern import CharNgramLM
from glass_amd.modeling.recognition.recognizer_decoder import ASTER_V2
from glass_amd.modeling.recognition.text_encoder import TextEncoder
from glass_amd.structures.core import ShapeSpec
from glass_amd.utils.synth import make_state_dict

PRE = "roi_heads.recognizer_head.decoder."
C, L, T, D = 97, 26, 32, 256

# what hipcc -Rpass-analysis=kernel-resource-usage reports for con_step_kernel<KB, CP, MERGE> at --offload-arch=gfx950 (a
# compile-time figure: re-derive it when csrc/decoder_search.hip or csrc/decoder_common.h change).  Per KB = 1 / 2 / 4 / 8 / 16.
RESOURCES = """step kernel resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950), KB = 1 / 2 / 4 / 8 / 16:
  merged DFA   (new): VGPRs 175 / 184 / 152 / 162 / 165, waves per SIMD 2 / 2 / 3 / 3 / 3, LDS 3412 / 6760 / 13456 / 26848 / 53632 bytes, scratch 0
  unmerged DFA      : VGPRs 175 / 184 / 152 / 162 / 165, waves per SIMD 2 / 2 / 3 / 3 / 3, LDS 3412 / 6760 / 13456 / 26848 / 53632 bytes, scratch 0
  merged WDFA  (new): VGPRs 175 / 184 / 154 / 163 / 162, waves per SIMD 2 / 2 / 3 / 3 / 3, LDS 3416 / 6768 / 13472 / 26880 / 53696 bytes, scratch 0
  unmerged WDFA     : VGPRs 175 / 184 / 153 / 163 / 162, waves per SIMD 2 / 2 / 3 / 3 / 3, LDS 3416 / 6768 / 13472 / 26880 / 53696 bytes, scratch 0
  (the unmerged and the trie instantiations: every figure, and every instruction, as before the merge stage was added.  The merge
   parks its results in the idle sproj array and needs ONE barrier; the row-by-row form with a barrier per beam row and the group
   re-read from memory in every row had 166 / 163 VGPRs at KB = 16 and measured 1.03 - 1.06x of the unmerged search where this
   one measures 1.02 - 1.04x: 9.99 against 9.59 ms instead of 9.87 against 9.61 ms for [A-Za-z0-9]+, 1024 RoIs, width 8)"""


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


def folded_rows(result, fold):
    """[R, k, L] int64: the fold symbol at every position before the stop, -1 from there on; and the finite mask [R, k]"""
    sym = result.symbols.cpu().numpy().astype(np.int64)
    ln = result.lengths.cpu().numpy().astype(np.int64)
    f = fold[sym]
    pos = np.arange(sym.shape[2])[None, None, :]
    f[pos >= np.maximum(ln - 1, 0)[:, :, None]] = -1
    return f, np.isfinite(result.scores.cpu().numpy())


def repeats(result, fold):
    """(finite result slots, those whose folded string an earlier finite slot of the same RoI holds)"""
    f, fin = folded_rows(result, fold)
    total = again = 0
    for rows, ok in zip(f, fin):
        seen = set()
        for row, good in zip(rows, ok):
            if good:
                key = row.tobytes()
                total += 1
                again += key in seen
                seen.add(key)
    return total, again


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_merged_beam.py measures on a HIP device; none found")
    dev = torch.device("cuda:0")
    cfg = get_glass_cfg(os.path.join(ROOT, "configs", "glass_icdar15_mi355x.yaml"), ["MODEL.DEVICE", "cuda:0"])
    enc = TextEncoder(cfg)
    eos = enc.character.index("[s]")
    assert len(enc.character) == C
    rc = SimpleNamespace(CHARACTER_SET=list(enc.character[2:]), MAX_WORD_LENGTH=L - 1)
    dec = ASTER_V2(SimpleNamespace(MODEL=SimpleNamespace(ROI_RECOGNIZER_HEAD=rc)), ShapeSpec(channels=D))
    dec.import_weights(dict(make_state_dict(1234, parts=("recog",))), dev, PRE)
    lexicon = words(np.random.default_rng(2024), 90000)
    trie = LexiconTrie(lexicon, enc, L, eos, case_insensitive=True, device=dev)
    lm = CharNgramLM.estimate([w.upper() for w in words(np.random.default_rng(11), 20000)], order=3)
    alnum = DecodePattern(r"[A-Za-z0-9]+", enc, L, eos, case_insensitive=True, device=dev)
    automata = {"[A-Za-z0-9]+": alnum, "from_trie (90000 words)": DecodePattern.from_trie(trie),
                "[A-Za-z0-9]+ x trigram": alnum.weighted(lm=lm)}
    lines = [f"fold-merged beam search: T={T} D={D} classes={C} steps={L}, device {torch.cuda.get_device_name(0)}, median (min) of "
             f"{args.reps} alternating reps after {args.warmup} warm-up calls, times in ms, case-insensitive patterns, weight_scale 1"]
    lines += RESOURCES.split("\n")
    records = []
    for name, pat in automata.items():
        sizes = np.diff(pat.fold_groups()[0])
        lines.append(f" {name}: {pat.num_states} states, F {pat.num_fold}, {int((sizes == 2).sum())} groups of two and "
                     f"{int((sizes == 1).sum())} of one, {pat.nbytes / 2 ** 20:.3f} MiB on the device")
        print(lines[-1], flush=True)
        for R in (256, 1024):
            g = torch.Generator(device="cpu")
            g.manual_seed(R)
            x = torch.randn((R, T, D), generator=g).to(dev)
            seg = torch.zeros(R, dtype=torch.int32).to(dev)
            for k in (1, 5, 8):
                merged = lambda: dec.beam_decode(x, k, eos, path_probs=True, pattern=pat, segments=seg, merge_case=True)
                plain = lambda: dec.beam_decode(x, k, eos, path_probs=True, pattern=pat, segments=seg)
                for _ in range(args.warmup):
                    merged(); plain()
                tm, tp = [], []
                for _ in range(args.reps):
                    ms, rm = timed(merged); tm.append(ms)
                    ms, rp = timed(plain); tp.append(ms)
                slots, twins = repeats(rp, pat.fold)
                mslots, mtwins = repeats(rm, pat.fold)
                med = statistics.median
                records.append({"automaton": name, "rois": R, "width": k, "merged_ms": round(med(tm), 3), "merged_ms_min": round(min(tm), 3),
                                "unmerged_ms": round(med(tp), 3), "unmerged_ms_min": round(min(tp), 3), "unmerged_slots": slots,
                                "unmerged_twin_slots": twins, "merged_slots": mslots, "merged_twin_slots": mtwins})
                lines.append(f"  RoIs {R:5d} width {k}: merged {med(tm):8.3f} ({min(tm):8.3f})  unmerged {med(tp):8.3f} ({min(tp):8.3f})  "
                             f"merged/unmerged {med(tm) / med(tp):5.2f}x  case twins in the unmerged result: {twins} of {slots} slots "
                             f"({100.0 * twins / max(slots, 1):.1f}%); in the merged: {mtwins} of {mslots}")
                print(lines[-1], flush=True)
    lines.append("not measured: per-kernel times, the end-to-end step with set_pattern(merge_case=True) / DECODE_MERGE_CASE, real "
                 "lexicon files, accuracy on real text (the synthetic decoder weights are near uniform over the classes, so the twin "
                 "share here says how the unmerged beam fills, not how a trained model's would)")
    lines.append(json.dumps({"metric": "merged_beam", "device": torch.cuda.get_device_name(0), "reps": args.reps, "results": records}))
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
