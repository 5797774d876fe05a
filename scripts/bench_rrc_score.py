"""RRC scorer (glass_rrc_pair_areas / glass_rrc_match, csrc/rrc_score.hip; RRCScorer.score) on one device.

A seeded TextOCR-scale synthetic: --images images, 10-60 ground-truth words and up to --max-dets detections per image;
ground truths are quads or 8-20 point rings, detections are quads or (--ring-share of them) pixel-staircase rings of up
to a few hundred points, as `masks_to_polygons` emits; most detections sit on a ground-truth word, so most pairs of an
image are disjoint and a few overlap, as in real submissions.
Times: HIP events around each of the two native calls (layout already on the device) after a warm-up, median and min of
--reps; `score()` is the host wall time of the whole call on the {name: lines} dictionary (parsing, upload, kernels,
download, tallies), ended by the download's synchronisation; `encode` is its parsing + upload part alone.

  python scripts/bench_rrc_score.py [--images 2000] [--reps 5]
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

from glass_amd.evaluation import RRCScorer
from glass_amd.ops import native as K


def quad(rng, cx, cy, w, h):
    t = np.deg2rad(rng.uniform(-25, 25))
    c, s = np.cos(t), np.sin(t)
    return [(int(round(cx + (a * w * c - b * h * s) / 2)), int(round(cy + (a * w * s + b * h * c) / 2))) for a, b in ((-1, 1), (1, 1), (1, -1), (-1, -1))]


def ellipse_ring(rng, cx, cy, w, h, n):
    ang = np.sort(rng.uniform(0, 2 * np.pi, n))[::-1]                      # negative shoelace: the detection files' orientation
    return [(int(round(cx + w / 2 * np.cos(a))), int(round(cy + h / 2 * np.sin(a)))) for a in ang]


def staircase_ring(cx, cy, w, h, steps):
    """a pixel-edge ring like masks_to_polygons': flat top, staircase bottom; 2 * steps + 2 points, x-monotone, simple"""
    x0, y0 = cx - w // 2, cy - h // 2
    sw = max(w // steps, 1)
    pts = [(x0, y0)]
    for k in range(steps):                                                 # along the bottom, left to right, going down then up
        y = y0 + h + (k % 3)
        pts += [(x0 + k * sw, y), (x0 + (k + 1) * sw, y)]
    pts.append((x0 + steps * sw, y0))
    return pts if _shoelace(pts) < 0 else pts[::-1]


def _shoelace(P):
    return sum(P[i][0] * P[(i + 1) % len(P)][1] - P[(i + 1) % len(P)][0] * P[i][1] for i in range(len(P)))


def line(P, text):
    P = P if _shoelace(P) < 0 else P[::-1]
    return ",".join(f"{x},{y}" for x, y in P) + ",####" + text


def make_case(images, max_dets, ring_share, seed):
    rng = np.random.default_rng(seed)
    words = ["word", "Text", "SALE", "exit!", "John's", "ab", "###", "street", "market", "OPEN"]
    gt, files = {}, {}
    for i in range(images):
        G = int(rng.integers(10, 61))
        boxes = [(int(rng.integers(100, 1900)), int(rng.integers(60, 1000)), int(rng.integers(30, 220)), int(rng.integers(12, 60))) for _ in range(G)]
        rings, texts = [], []
        for cx, cy, w, h in boxes:
            P = quad(rng, cx, cy, w, h) if rng.random() < 0.5 else ellipse_ring(rng, cx, cy, w, h, int(rng.integers(8, 21)))
            if len(set(P)) < 3 or _shoelace(P) == 0:
                P = [(cx, cy), (cx + w, cy), (cx + w, cy + h), (cx, cy + h)]
            rings.append([v for p in P for v in p])
            texts.append(str(rng.choice(words)))
        key = f"{i:07d}"
        gt[key] = (rings, texts)
        D = int(rng.integers(max_dets // 8, max_dets + 1))
        lines = []
        for d in range(D):
            if rng.random() < 0.8:
                cx, cy, w, h = boxes[int(rng.integers(0, G))]
                cx, cy = cx + int(rng.integers(-5, 6)), cy + int(rng.integers(-4, 5))
            else:
                cx, cy, w, h = int(rng.integers(100, 1900)), int(rng.integers(60, 1000)), int(rng.integers(30, 220)), int(rng.integers(12, 60))
            if rng.random() < ring_share:
                P = staircase_ring(cx, cy, w, h, int(rng.integers(8, min(max(w // 2, 9), 120))))
            else:
                P = quad(rng, cx, cy, w, h)
            if len(set(P)) < 3 or _shoelace(P) == 0:
                P = [(cx, cy + h), (cx + w, cy + h), (cx + w, cy), (cx, cy)]
            lines.append(line(P, str(rng.choice(words[:6]))))
        files[key + ".txt"] = lines
    return gt, files


def timed(call, reps):
    call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = call()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=2000)
    ap.add_argument("--max-dets", type=int, default=300)
    ap.add_argument("--ring-share", type=float, default=0.3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=2026)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the benchmark needs a HIP device"
    dev = torch.device("cuda:0")
    t0 = time.perf_counter()
    gt, files = make_case(a.images, a.max_dets, a.ring_share, a.seed)
    gen_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    scorer = RRCScorer(gt, False, dev)
    torch.cuda.synchronize()
    gt_ms = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    enc = scorer.encode_submission(files, validate=False)
    torch.cuda.synchronize()
    enc_ms = (time.perf_counter() - t0) * 1e3
    G, D = enc.n_gt_per_image, enc.n_det_per_image
    chunks = scorer.chunks(D)
    n_pairs_total = int((G * D).sum())
    poly_len = np.diff(enc.poly_off.cpu().numpy())
    edge_pairs = float(sum(np.outer(poly_len[scorer._gt_off_host[i]:scorer._gt_off_host[i + 1]],
                                    poly_len[scorer.n_gt + int(D[:i].sum()):scorer.n_gt + int(D[:i + 1].sum())]).sum()
                           for i in range(len(G))))
    print(f"case: {a.images} images, {int(G.sum())} GT polygons, {int(D.sum())} detections ({int(poly_len[scorer.n_gt:].max())} points at most), "
          f"{n_pairs_total:.3e} pairs, {edge_pairs:.3e} edge pairs if none were rejected; {len(chunks)} chunk(s) of <= "
          f"{scorer.workspace_cap_bytes >> 20} MiB of inter (generated in {gen_s:.1f} s)")
    pa_med = pa_min = m_med = m_min = 0.0
    overlapping = 0
    for ca, cb in chunks:                                                   # the two kernels, chunk by chunk as score() runs them
        pair_off = K.upload(np.concatenate([[0], np.cumsum(G[ca:cb] * D[ca:cb])]).astype(np.int64), torch.int64, dev)
        n_pairs = int((G[ca:cb] * D[ca:cb]).sum())
        gt_off, det_off = enc.gt_off[ca:cb + 1], enc.det_off[ca:cb + 1]
        med, best, (area, inter) = timed(lambda: K.rrc_pair_areas(enc.pts, enc.poly_off, gt_off, det_off, pair_off, n_pairs), a.reps)
        pa_med, pa_min = pa_med + med, pa_min + best
        overlapping += int((inter > 0).sum())
        g0, g1 = int(scorer._gt_off_host[ca]), int(scorer._gt_off_host[cb])
        med, best, _ = timed(lambda: K.rrc_match(area, inter, pair_off, gt_off, det_off, scorer._gt_dc_e2e[g0:g1], scorer._gt_dc_det[g0:g1],
                                                 int(D[ca:cb].sum())), a.reps)
        m_med, m_min = m_med + med, m_min + best
    walls = []
    for _ in range(max(a.reps // 2, 2)):
        t0 = time.perf_counter()
        res = scorer.score(files, validate=False)
        walls.append((time.perf_counter() - t0) * 1e3)
    print(f"  rrc_pair_areas (polygon + pair kernels): median {pa_med:.3f} ms, min {pa_min:.3f} ms over {a.reps} reps -> "
          f"{n_pairs_total / (pa_med * 1e-3):.3e} pairs/s; {overlapping} pairs with a non-zero intersection")
    print(f"  rrc_match (one workgroup per image): median {m_med:.3f} ms, min {m_min:.3f} ms")
    print(f"  RRCScorer.score wall: median {statistics.median(walls):.0f} ms, min {min(walls):.0f} ms "
          f"(of it parsing + upload of the submission: {enc_ms:.0f} ms); ground-truth encode + upload {gt_ms:.0f} ms")
    print(f"  {res['e2e_method']}\n  {res['det_only_method']}")
    print(json.dumps({"metric": "rrc_score", "device": torch.cuda.get_device_name(0), "images": a.images, "pairs": n_pairs_total,
                      "detections": int(D.sum()), "pair_areas_ms_median": round(pa_med, 3), "pair_areas_ms_min": round(pa_min, 3),
                      "match_ms_median": round(m_med, 3), "match_ms_min": round(m_min, 3),
                      "score_wall_ms_median": round(statistics.median(walls), 1), "encode_ms": round(enc_ms, 1)}))


if __name__ == "__main__":
    main()
