"""Lexicon matching (glass_lexicon_match, csrc/lexicon.hip) on one device against the host find_match_word loop.

Cases, on seeded synthetic lexicons of English-like word lengths:
  generic - every query against one 90,000-word lexicon (the IC15 generic-vocabulary scale; 15,000 queries = 500
            images x 30 words),
  strong  - 500 images x 30 words, each against its own 100-word lexicon (the IC15 per-image strong lexicons).
Device times are HIP-event times of the lexicon_match call (query upload + its three launches) after a warm-up, the
median of --reps; `match` is the whole LexiconMatcher.match wall time (host encoding and pair lookup included).  The
host path runs find_match_word for --host-queries queries of each case; their answers are checked against the device.

  python scripts/bench_lexicon.py [--reps 5] [--host-queries 2]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "glass-text-spotting_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np
import torch

from glass_amd.evaluation import LexiconMatcher, encode_query, find_match_word
from glass_amd.ops import native as K

_LETTERS = np.frombuffer(b"etaoinshrdlcumwfgypbvkjxqz", dtype=np.uint8)
_FREQ = np.array([12.7, 9.1, 8.2, 7.5, 7.0, 6.7, 6.3, 6.1, 6.0, 4.3, 4.0, 2.8, 2.8, 2.4, 2.4, 2.2, 2.0, 2.0, 1.9, 1.5,
                  1.0, 0.8, 0.15, 0.15, 0.1, 0.07])


def words(rng, n, mean_len=8.0):
    lens = np.clip(rng.poisson(mean_len - 2, n) + 2, 1, 24)
    sym = rng.choice(_LETTERS, size=int(lens.sum()), p=_FREQ / _FREQ.sum()).tobytes().decode()
    out, o = [], 0
    for k in lens:
        out.append(sym[o:o + k].capitalize())
        o += k
    return out


def noisy(rng, w):
    """a recognised word: the lexicon word with 0-2 random substitutions"""
    w = list(w.upper())
    for _ in range(rng.integers(0, 3)):
        w[rng.integers(0, len(w))] = chr(int(rng.choice(_LETTERS))).upper()
    return "".join(w)


def device_time(m, queries, segments, reps):
    q = [encode_query(s) for s in queries]
    seg = [m.lexicon.segment(k) for k in segments]
    t = m.lexicon.tensors
    call = lambda: K.lexicon_match(q, seg, t["word_off"], t["word_len"], t["word_sym"], t["word_index"], t["seg_off"],
                                   m.lexicon.max_segment_words)
    call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    t0 = time.perf_counter()
    res = m.match(queries, segments)
    wall = (time.perf_counter() - t0) * 1e3
    return statistics.median(ms), min(ms), wall, res


def run_case(name, lexicon, pairs, queries, segments, pairs_per_query, reps, host_queries, dev):
    t0 = time.perf_counter()
    m = LexiconMatcher(lexicon, pairs, device=dev)
    torch.cuda.synchronize()
    load_ms = (time.perf_counter() - t0) * 1e3
    med, best, wall, res = device_time(m, queries, segments, reps)
    total_pairs = sum(pairs_per_query)
    t0 = time.perf_counter()
    for i in range(host_queries):
        lex, pr = (lexicon, pairs) if segments[i] is None else (lexicon[segments[i]], pairs[segments[i]])
        assert find_match_word(queries[i], lex, pr) == res[i], (name, i)
    host_s = (time.perf_counter() - t0) / max(host_queries, 1)
    host_total_h = host_s * len(queries) / 3600
    print(f"{name}: {len(queries)} queries, {total_pairs:.3e} (query, word) pairs")
    print(f"  device lexicon_match: median {med:.3f} ms, min {best:.3f} ms over {reps} reps -> {total_pairs / (med * 1e-3):.3e} pairs/s")
    print(f"  LexiconMatcher.match wall (host encode + launch + lookup): {wall:.1f} ms;  lexicon encode + upload {load_ms:.1f} ms")
    print(f"  host find_match_word: {host_s:.3f} s per query ({host_queries} queries, answers equal) -> {host_total_h:.2f} h for all")
    return {"case": name, "queries": len(queries), "pairs": total_pairs, "device_ms_median": round(med, 3), "device_ms_min": round(best, 3),
            "pairs_per_s": total_pairs / (med * 1e-3), "match_wall_ms": round(wall, 1), "host_s_per_query": round(host_s, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-queries", type=int, default=2)
    ap.add_argument("--generic-words", type=int, default=90_000)
    ap.add_argument("--images", type=int, default=500)
    ap.add_argument("--words-per-image", type=int, default=30)
    ap.add_argument("--strong-words", type=int, default=100)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(2026)
    n_q = a.images * a.words_per_image
    out = []

    generic = words(rng, a.generic_words)
    gpairs = {w.upper(): w for w in generic}
    gq = [noisy(rng, generic[i]) for i in rng.integers(0, len(generic), n_q)]
    out.append(run_case("generic", generic, gpairs, gq, [None] * n_q, [len(generic)] * n_q, a.reps, a.host_queries, dev))

    strong = {i: words(rng, a.strong_words) for i in range(1, a.images + 1)}
    spairs = {i: {w.upper(): w for w in ws} for i, ws in strong.items()}
    sseg = [1 + k // a.words_per_image for k in range(n_q)]
    sq = [noisy(rng, strong[s][int(rng.integers(0, a.strong_words))]) for s in sseg]
    out.append(run_case("strong", strong, spairs, sq, sseg, [a.strong_words] * n_q, a.reps, a.host_queries, dev))
    print(json.dumps({"metric": "lexicon_match", "device": torch.cuda.get_device_name(0), "cases": out}))


if __name__ == "__main__":
    main()
