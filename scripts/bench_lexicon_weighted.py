"""Weighted lexicon matching (glass_lexicon_match_weighted, csrc/lexicon_weighted.hip) on one device against the host
find_match_word_weighted loop, on the input of scripts/bench_lexicon.py's generic case: 15,000 queries (500 images x 30
words) against one 90,000-word lexicon, with a 26 x 97 character-probability table per query.

Prints
  kernel  - HIP-event time of the glass_lexicon_match_weighted call alone (its four launches; queries and cost tables
            already on the device), median of --reps after a warm-up,
  match   - wall time of one whole WeightedLexiconMatcher.match call: cost-table build on the host, upload, launches,
            download and pair lookup (the table build is also shown on its own),
  host    - find_match_word_weighted per query on --host-queries queries (answers checked against the device), SCALED to
            all queries,
and, beside them, the un-weighted glass_lexicon_match time on the same queries and lexicon.

  python scripts/bench_lexicon_weighted.py [--reps 5] [--host-queries 20]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "glass-text-spotting_amd"), os.path.join(ROOT, "scripts")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np
import torch

from bench_lexicon import noisy, words
from glass_amd.config import get_glass_cfg
from glass_amd.evaluation import (LexiconMatcher, WeightedLexiconMatcher, encode_query, find_match_word_weighted,
                                  weighted_cost_tables)
from glass_amd.modeling.recognition.text_encoder import TextEncoder
from glass_amd.ops import native as K


def make_scores(rng, queries, enc, rows=26):
    """[Q][rows][classes] float32: a peaked distribution per step, the query's own character on top"""
    C = len(enc.character)
    s = rng.random((len(queries), rows, C), dtype=np.float32) ** 12
    for i, q in enumerate(queries):
        s[i, np.arange(len(q)), [enc.char_encode(c) for c in q]] = rng.uniform(0.5, 3.0, len(q))
    return s / s.sum(axis=2, keepdims=True)


def events_ms(call, reps):
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
    return statistics.median(ms), min(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-queries", type=int, default=20)
    ap.add_argument("--generic-words", type=int, default=90_000)
    ap.add_argument("--images", type=int, default=500)
    ap.add_argument("--words-per-image", type=int, default=30)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(2026)
    n_q = a.images * a.words_per_image
    enc = TextEncoder(get_glass_cfg(os.path.join(ROOT, "configs", "glass_icdar15_mi355x.yaml"), []))
    lexicon = words(rng, a.generic_words)
    pairs = {w.upper(): w for w in lexicon}
    queries = [noisy(rng, lexicon[i]) for i in rng.integers(0, len(lexicon), n_q)]
    scores = make_scores(rng, queries, enc)
    m = WeightedLexiconMatcher(lexicon, pairs, enc, device=dev)
    A = len(m.classes)

    # the whole call, and its host part alone
    m.match(queries[:64], scores=scores[:64])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = m.match(queries, scores=scores)
    match_ms = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    tables = [np.concatenate([x.reshape(-1) for x in weighted_cost_tables(q, s, enc, m.classes)]) for q, s in zip(queries, scores)]
    build_ms = (time.perf_counter() - t0) * 1e3
    sizes = np.fromiter((x.size for x in tables), dtype=np.int64, count=n_q)
    cost = np.concatenate(tables)

    # the kernel alone: everything on the device already
    t = m.lexicon.tensors
    q_np, lens = K._lexicon_queries([encode_query(s) for s in queries])
    d = dict(q_sym=torch.from_numpy(q_np).to(dev), q_len=torch.from_numpy(lens).to(dev), q_seg=torch.zeros(n_q, dtype=torch.int32, device=dev),
             cost=torch.from_numpy(cost).to(dev), off=torch.from_numpy(np.cumsum(sizes) - sizes).to(dev))
    index = torch.empty(n_q, dtype=torch.int32, device=dev)
    dist = torch.empty(n_q, dtype=torch.float64, device=dev)
    status = torch.empty(n_q, dtype=torch.int32, device=dev)
    kernel = lambda: K.lexicon_match_weighted_launch(d["q_sym"], d["q_len"], d["q_seg"], d["cost"], cost.size, d["off"], m.sym_class, A,
                                                     int(lens.max()), t["word_off"], t["word_len"], t["word_sym"], t["word_index"],
                                                     t["seg_off"], m.lexicon.max_segment_words, index, dist, status)
    k_med, k_min = events_ms(kernel, a.reps)
    assert int(status.max()) == 0
    up = m.lexicon.upper
    again = [(pairs[up[i]], x) if i >= 0 else ("", 100) for i, x in zip(index.cpu().tolist(), dist.cpu().tolist())]
    assert again == res, "the timed launch and match() disagree"

    # the un-weighted matcher on the same input
    u = LexiconMatcher(m.lexicon, pairs)
    enc_q = [encode_query(s) for s in queries]
    seg = [0] * n_q
    u_med, u_min = events_ms(lambda: K.lexicon_match(enc_q, seg, t["word_off"], t["word_len"], t["word_sym"], t["word_index"], t["seg_off"],
                                                     m.lexicon.max_segment_words), a.reps)
    unit = u.match(queries)
    moved = sum(r[0] != v[0] for r, v in zip(res, unit))

    # the host path on a sample
    t0 = time.perf_counter()
    for i in range(a.host_queries):
        got = find_match_word_weighted(queries[i], lexicon, pairs, scores[i].astype(np.float64).tolist(), enc)
        assert (got[0], float(got[1]).hex()) == (res[i][0], float(res[i][1]).hex()), (i, got, res[i])
    host_s = (time.perf_counter() - t0) / max(a.host_queries, 1)

    print(f"weighted lexicon match: {n_q} queries x {len(lexicon)} words, scores {scores.shape[1]} x {scores.shape[2]}, {A} symbol classes, "
          f"{cost.nbytes / 2**20:.1f} MiB of cost tables")
    print(f"  kernel  glass_lexicon_match_weighted (4 launches, inputs on the device): median {k_med:.3f} ms, min {k_min:.3f} ms over {a.reps} reps")
    print(f"  match   WeightedLexiconMatcher.match wall (table build + upload + launches + lookup): {match_ms:.1f} ms; "
          f"the host table build alone: {build_ms:.1f} ms")
    print(f"  host    find_match_word_weighted: {host_s:.3f} s per query on {a.host_queries} queries (answers equal, distances bit for bit) "
          f"-> SCALED to {n_q} queries: {host_s * n_q / 3600:.2f} h")
    print(f"  beside  un-weighted glass_lexicon_match on the same input (query upload + 3 launches): median {u_med:.3f} ms, min {u_min:.3f} ms; "
          f"the weighted rule picks another word for {moved} of {n_q} queries")
    print(json.dumps({"metric": "lexicon_match_weighted", "device": torch.cuda.get_device_name(0), "queries": n_q, "words": len(lexicon),
                      "kernel_ms_median": round(k_med, 3), "kernel_ms_min": round(k_min, 3), "match_wall_ms": round(match_ms, 1),
                      "table_build_ms": round(build_ms, 1), "host_s_per_query": round(host_s, 4),
                      "host_h_scaled": round(host_s * n_q / 3600, 3), "unweighted_ms_median": round(u_med, 3)}))


if __name__ == "__main__":
    main()
