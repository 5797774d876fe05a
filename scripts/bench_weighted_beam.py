"""Weighted-pattern beam search on one device: ASTER_V2.beam_decode(pattern=WeightedPattern) (glass_beam_search_wdfa) against
the unweighted search on the same automaton's base pattern (glass_beam_search_dfa), from the same build on the same inputs, in
the same process, alternating.  The same run repeats the lexicon-constrained (glass_beam_search_lexicon, the 90,000-word trie)
and the unconstrained search (glass_beam_search), so that their lines can be set against profiles/pattern_beam.txt: the step
kernel the four searches share did not slow.

The shipped decoder shape: T = 32 encoder steps, D = 256, 97 classes, 26 decoding steps; seeded random encoder outputs and
synthetic decoder weights.  Automata:
  [A-Za-z0-9]+ crossed with a character trigram model (CharNgramLM.estimate on a seeded synthetic word list, mixed case);
  the 90,000-word synthetic lexicon of scripts/bench_lexicon_beam.py as a DFA (DecodePattern.from_trie) with seeded word priors
    pushed toward the root.
For every (automaton, RoIs, width):
  weighted / pattern / lexicon / free - wall time of one call ending in a device synchronise, median and min of --reps after
                                        --warmup;
  completed                           - RoIs whose best hypothesis exists;  changed - RoIs whose best string differs from the
                                        unweighted search's.
Per automaton: states, fold symbols, bytes on the device and the host build time of the weighted tables (the base aside).

  python scripts/bench_weighted_beam.py [--reps 20] [--warmup 2] [--out profiles/weighted_beam.txt]
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


def mixed_case(rng, ws):
    """every word as it is, capitalised or in capitals, a third each"""
    how = rng.integers(0, 3, len(ws))
    return [w if h == 0 else w.capitalize() if h == 1 else w.upper() for w, h in zip(ws, how)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_weighted_beam.py measures on a HIP device; none found")
    dev = torch.device("cuda:0")
    cfg = get_glass_cfg(os.path.join(ROOT, "configs", "glass_icdar15_mi355x.yaml"), ["MODEL.DEVICE", "cuda:0"])
    enc = TextEncoder(cfg)
    eos = enc.character.index("[s]")
    assert len(enc.character) == C
    rc = SimpleNamespace(CHARACTER_SET=list(enc.character[2:]), MAX_WORD_LENGTH=L - 1)
    dec = ASTER_V2(SimpleNamespace(MODEL=SimpleNamespace(ROI_RECOGNIZER_HEAD=rc)), ShapeSpec(channels=D))
    dec.import_weights(dict(make_state_dict(1234, parts=("recog",))), dev, PRE)
    lexicon = words(np.random.default_rng(2024), 90000)
    trie = LexiconTrie(lexicon, enc, L, eos, device=dev)
    t0 = time.perf_counter()
    lm = CharNgramLM.estimate(mixed_case(np.random.default_rng(7), words(np.random.default_rng(11), 20000)), order=3)
    lm_seconds = time.perf_counter() - t0
    logprior = np.log(np.random.default_rng(5).zipf(1.3, len(lexicon)).astype(np.float64))
    logprior -= np.log(np.exp(logprior).sum())                                     # log of a distribution over the words
    alnum = DecodePattern(r"[A-Za-z0-9]+", enc, L, eos, device=dev)
    as_dfa = DecodePattern.from_trie(trie)
    automata = {"[A-Za-z0-9]+ x trigram": (alnum, alnum.weighted(lm=lm)),
                "from_trie (90000 words) + priors": (as_dfa, as_dfa.weighted(word_logprior=logprior))}
    lines = [f"weighted-pattern beam search: T={T} D={D} classes={C} steps={L}, device {torch.cuda.get_device_name(0)}, "
             f"median (min) of {args.reps} alternating reps after {args.warmup} warm-up calls, times in ms, weight_scale 1",
             f" the lexicon search's trie: {len(trie)} words, {trie.num_nodes} nodes, F {trie.num_fold}, {trie.nbytes / 2 ** 20:.2f} MiB "
             f"on the device, built on the host in {trie.build_seconds * 1e3:.0f} ms",
             f" the trigram model: {len(lm.logp)} n-grams, {len(lm.backoff)} back-off weights, estimated from 20000 words in "
             f"{lm_seconds * 1e3:.0f} ms"]
    records = []
    for name, (base, pat) in automata.items():
        lines.append(f" {name}: {pat.num_states} states ({base.num_states} unweighted), F {pat.num_fold}, {pat.nbytes / 2 ** 20:.3f} MiB on the "
                     f"device ({pat.trans.nbytes} bytes of transitions; unweighted {base.next.nbytes}), weighted tables built on the host "
                     f"in {pat.build_seconds * 1e3:.1f} ms (the base in {base.build_seconds * 1e3:.1f} ms)")
        print(lines[-1], flush=True)
        for R in (256, 1024):
            g = torch.Generator(device="cpu")
            g.manual_seed(R)
            x = torch.randn((R, T, D), generator=g).to(dev)
            seg = torch.zeros(R, dtype=torch.int32).to(dev)
            for k in (1, 5, 8):
                wdfa = lambda: dec.beam_decode(x, k, eos, path_probs=True, pattern=pat, segments=seg)
                dfa = lambda: dec.beam_decode(x, k, eos, path_probs=True, pattern=base, segments=seg)
                lexi = lambda: dec.beam_decode(x, k, eos, path_probs=True, lexicon=trie, segments=seg)
                free = lambda: dec.beam_decode(x, k, eos, path_probs=True)
                for _ in range(args.warmup):
                    wdfa(); dfa(); lexi(); free()
                tw, td, tl, tf = [], [], [], []
                for _ in range(args.reps):
                    ms, rw = timed(wdfa); tw.append(ms)
                    ms, rd = timed(dfa); td.append(ms)
                    ms, _ = timed(lexi); tl.append(ms)
                    ms, _ = timed(free); tf.append(ms)
                done = int(torch.isfinite(rw.scores[:, 0]).sum())
                changed = int((rw.symbols[:, 0] != rd.symbols[:, 0]).any(dim=1).sum())
                med = statistics.median
                records.append({"automaton": name, "rois": R, "width": k, "weighted_ms": round(med(tw), 3), "weighted_ms_min": round(min(tw), 3),
                                "pattern_ms": round(med(td), 3), "pattern_ms_min": round(min(td), 3), "lexicon_ms": round(med(tl), 3),
                                "lexicon_ms_min": round(min(tl), 3), "free_ms": round(med(tf), 3), "free_ms_min": round(min(tf), 3),
                                "completed": done, "changed": changed, "states": pat.num_states, "fold": pat.num_fold, "bytes": pat.nbytes,
                                "build_ms": round(pat.build_seconds * 1e3, 2)})
                lines.append(f"  RoIs {R:5d} width {k}: weighted {med(tw):8.3f} ({min(tw):8.3f})  pattern {med(td):8.3f} ({min(td):8.3f})  "
                             f"lexicon {med(tl):8.3f} ({min(tl):8.3f})  free {med(tf):8.3f} ({min(tf):8.3f})  weighted/pattern "
                             f"{med(tw) / med(td):5.2f}x  best hypothesis exists for {done} of {R} RoIs, differs from the unweighted for {changed}")
                print(lines[-1], flush=True)
    lines.append("not measured: per-kernel times, the end-to-end step with set_pattern / DECODE_LENGTH_BONUS, a product automaton larger "
                 "than the caches (this one has a few thousand states), real lexicon files and priors, accuracy on real text")
    lines.append(json.dumps({"metric": "weighted_beam", "device": torch.cuda.get_device_name(0), "reps": args.reps, "results": records}))
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
