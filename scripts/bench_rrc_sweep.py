"""Threshold sweep of the RRC scorer (glass_rrc_sweep, csrc/rrc_sweep.hip; RRCScorer.sweep) on one device.

The seeded 2000-image synthetic of scripts/bench_rrc_score.py with seeded three-digit scores on every detection and a
--grid x --grid grid of (text, detection) thresholds (101 x 101: 0.00, 0.01, ..., 1.00).
Times: HIP events around the native `rrc_sweep` call (bit matrices + sweep kernel; areas and don't-care marks already on
the device) after a warm-up, median and min of --reps, summed over the chunks; `sweep()` is the host wall time of the whole
call on the {name: [(line, score_text, score_detection)]} dictionary, ended by the download of the counts, and `encode` its
parsing + upload part alone, measured by itself.  For comparison, the path a grid search used before: one
`RRCScorer.score` call per cell on that cell's thresholded lines (what `TextResultWriter.evaluate` runs after
`to_eval_format`; its record formatting and self-intersection test come on top and are not timed here), on the 3 x 3
sub-grid of --compare-at.  Every compared cell must give the sweep's numbers.

  python scripts/bench_rrc_sweep.py [--images 2000] [--grid 101] [--reps 5]
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

from bench_rrc_score import make_case, timed
from glass_amd.evaluation import RRCScorer
from glass_amd.evaluation.rrc_score import parse_method_string, transcription_ids
from glass_amd.ops import native as K


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=2000)
    ap.add_argument("--max-dets", type=int, default=300)
    ap.add_argument("--ring-share", type=float, default=0.3)
    ap.add_argument("--grid", type=int, default=101)
    ap.add_argument("--compare-at", type=float, nargs=3, default=[0.2, 0.5, 0.8])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=2026)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the benchmark needs a HIP device"
    dev = torch.device("cuda:0")
    gt, files = make_case(a.images, a.max_dets, a.ring_share, a.seed)
    rng = np.random.default_rng(a.seed + 1)
    scored = {name: [(l, round(float(rng.random()), 3), round(float(rng.random()), 3)) for l in lines] for name, lines in files.items()}
    grid = [round(k / (a.grid - 1), 6) for k in range(a.grid)] if a.grid > 1 else [0.5]
    scorer = RRCScorer(gt, False, dev)

    t0 = time.perf_counter()
    enc = scorer.encode_submission(files, validate=False)
    torch.cuda.synchronize()
    enc_ms = (time.perf_counter() - t0) * 1e3
    G, D = enc.n_gt_per_image, enc.n_det_per_image
    print(f"case: {a.images} images, {int(G.sum())} GT polygons, {int(D.sum())} detections ({int(D.max())} in one image at most), "
          f"{int((G * D).sum()):.3e} pairs; grid {a.grid} x {a.grid} = {a.grid ** 2} combinations")

    # the native call alone, chunk by chunk as sweep() runs it
    up = lambda v, t: K.upload(np.ascontiguousarray(v), t, dev)
    gt_accept, det_word = transcription_ids(scorer.samples, enc.det_transcriptions, False)
    gt_accept, det_word = up(gt_accept, torch.int32).reshape(-1, 4), up(det_word, torch.int32)
    flat = np.array([(st, sd) for key in scorer.keys for _, st, sd in scored.get(key + ".txt", [])], dtype=np.float64).reshape(-1, 2)
    score_text, score_det = up(flat[:, 0], torch.float64), up(flat[:, 1], torch.float64)
    text_th, det_th = up(np.repeat(grid, len(grid)), torch.float64), up(np.tile(grid, len(grid)), torch.float64)
    counts = torch.zeros((len(grid) ** 2, 6), dtype=torch.int64, device=dev)
    d_off = np.concatenate([[0], np.cumsum(D)])
    k_med = k_min = 0.0
    for ca, cb in scorer.chunks(D):
        pair_off = K.upload(np.concatenate([[0], np.cumsum(G[ca:cb] * D[ca:cb])]).astype(np.int64), torch.int64, dev)
        gt_off, det_off = enc.gt_off[ca:cb + 1], enc.det_off[ca:cb + 1]
        area, inter = K.rrc_pair_areas(enc.pts, enc.poly_off, gt_off, det_off, pair_off, int((G[ca:cb] * D[ca:cb]).sum()))
        g0, g1, d0, d1 = int(scorer._gt_off_host[ca]), int(scorer._gt_off_host[cb]), int(d_off[ca]), int(d_off[cb])
        dc_e, dc_d, _, _ = K.rrc_match(area, inter, pair_off, gt_off, det_off, scorer._gt_dc_e2e[g0:g1], scorer._gt_dc_det[g0:g1], d1 - d0)
        med, best, _ = timed(lambda: K.rrc_sweep(area, inter, pair_off, gt_off, det_off, scorer._gt_dc_e2e[g0:g1], scorer._gt_dc_det[g0:g1],
                                                 dc_e, dc_d, score_text[d0:d1], score_det[d0:d1], gt_accept[g0:g1], det_word[d0:d1],
                                                 text_th, det_th, counts, max_dets=int(D[ca:cb].max())), a.reps)
        k_med, k_min = k_med + med, k_min + best

    walls = []
    for _ in range(max(a.reps // 2, 2)):
        t0 = time.perf_counter()
        sw = scorer.sweep(scored, grid, grid, validate=False)
        walls.append((time.perf_counter() - t0) * 1e3)
    wall = statistics.median(walls)

    # the earlier method on a 3 x 3 sub-grid: one score() per cell
    cells = []
    sub = scorer.sweep(scored, a.compare_at, a.compare_at, validate=False)
    for i, t in enumerate(a.compare_at):
        for j, d in enumerate(a.compare_at):
            cell = {name: [l for l, st, sd in ls if not (st < t or sd < d)] for name, ls in scored.items()}
            t0 = time.perf_counter()
            res = scorer.score(cell, validate=False)
            cells.append((time.perf_counter() - t0) * 1e3)
            one = sub.results(i, j)
            assert one == dict(parse_method_string(res[k]) for k in ("e2e_method", "det_only_method")), (t, d)
            if t in grid and d in grid:
                assert sw.results(grid.index(t), grid.index(d)) == one, (t, d)
    cell_ms = statistics.median(cells)

    bt, bd, best = sw.best()
    print(f"  rrc_sweep (bit matrices + sweep kernel, {a.grid ** 2} combinations): median {k_med:.3f} ms, min {k_min:.3f} ms over {a.reps} reps "
          f"-> {a.images * a.grid ** 2 / (k_med * 1e-3):.3e} (image, combination) problems/s")
    print(f"  RRCScorer.sweep wall: median {wall:.0f} ms, min {min(walls):.0f} ms; parsing + upload of the submission alone: {enc_ms:.0f} ms, "
          f"so about {wall - enc_ms:.0f} ms for ids, uploads, kernels and the download")
    print(f"  one RRCScorer.score call per cell ({len(cells)} cells at {a.compare_at}): median {cell_ms:.0f} ms, min {min(cells):.0f} ms, "
          f"max {max(cells):.0f} ms per call; every cell equals the sweep's")
    print(f"  one sweep of {a.grid ** 2} cells costs {wall / cell_ms:.2f} such calls")
    print(f"  best E2E hmean {best['E2E_RESULTS']['hmean']:.6f} at text >= {bt}, detection >= {bd}")
    print(json.dumps({"metric": "rrc_sweep", "device": torch.cuda.get_device_name(0), "images": a.images, "combinations": a.grid ** 2,
                      "detections": int(D.sum()), "sweep_kernels_ms_median": round(k_med, 3), "sweep_kernels_ms_min": round(k_min, 3),
                      "sweep_wall_ms_median": round(wall, 1), "encode_ms": round(enc_ms, 1), "score_per_cell_ms_median": round(cell_ms, 1)}))


if __name__ == "__main__":
    main()
