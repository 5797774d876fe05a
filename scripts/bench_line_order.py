"""Page order and blocks on one device: ops.native.order_lines (glass_order_lines, csrc/line_order.hip) alone, the word
post-processor with POST_PROCESSING.ORDER_LINES on against off (GROUP_LINES on in both), and the host statement
order_lines_host for scale.

8 images of n lines each, n = 100, 300, 1024: seeded column pages (a header over three columns of paragraphs whose gaps sit
at the same height in every column, ragged last lines, indices shuffled), and one scene whose 1024 lines are a single column
(every pair overlaps: the densest relation, and a successor row of up to 1023 bits per step).  For each:
  kernels:   device time of ops.native.order_lines (HIP events around each call: the four launches and the allocation of the
             outputs and the workspace; median and minimum of --reps after a warm-up), and from it the time per line of the
             scene, which the serial emission loop dominates at 1024;
  on / off:  host wall time of PostProcessorRotatedBoxes.process_padded (no text; the call ends in its one read-back, so it
             is synchronous) on the same boxes as words - every word is a line of its own, so the page has n lines - with the
             key on and off, the same post-processor object and build, alternating call by call; median of --reps each;
  host:      wall time of order_lines_host on the same 8 images, one after the other (--host-reps, median), and whether its
             integer outputs equal the kernel's.
Writes profiles/line_order.txt.

  python scripts/bench_line_order.py [--reps 200] [--host-reps 2] [--out profiles/line_order.txt]
"""
import argparse
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

from glass_amd._lib import source_sha16
from glass_amd.config import get_glass_cfg
from glass_amd.ops import native as K
from glass_amd.postprocess import build_post_processor, order_lines_host

N_IMAGES = 8
INT_KEYS = ("page_rank", "page_order", "block_id")


def scene(kind, n, seed):
    g = np.random.default_rng([seed, n, 0 if kind == "columns" else 1])
    columns = 3 if kind == "columns" else 1
    col_w, gutter, pitch, para_gap = 300.0, 40.0, 28.0, 30.0
    width = columns * col_w + (columns - 1) * gutter
    rows = []
    if kind == "columns":
        rows.append([width / 2, 30.0, width - 4.0, 24.0, g.uniform(-0.5, 0.5)])
    body = n - len(rows)
    depth = -(-body // columns)
    for c in range(columns):
        y = 30.0 + pitch + para_gap
        for r in range(min(depth, body - c * depth)):
            last = r % 9 == 8                                          # a paragraph of nine lines, the last one ragged
            w = col_w * g.uniform(0.35, 0.8) if last else col_w - g.uniform(0, 6)
            rows.append([c * (col_w + gutter) + w / 2 + g.uniform(0, 2), y + g.uniform(-0.4, 0.4), w, 20.0 * g.uniform(0.95, 1.05),
                         g.uniform(-0.5, 0.5)])
            y += pitch + (para_gap if last else 0.0)
    boxes = np.asarray(rows, np.float32)
    assert len(boxes) == n
    return boxes[g.permutation(n)]


def device_time(call, reps):
    for _ in range(5):
        out = call()
    torch.cuda.synchronize()
    us = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = call()
        e1.record()
        torch.cuda.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3)
    return statistics.median(us), min(us), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "line_order.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_line_order.py needs a HIP device: there is nothing to time without one")
    dev = torch.device("cuda:0")
    path = os.path.join(ROOT, "configs", "glass_icdar15_mi355x.yaml")
    pp = build_post_processor(get_glass_cfg(path, ["POST_PROCESSING.GROUP_LINES", True, "POST_PROCESSING.ORDER_LINES", True]))
    pp.text_threshold = None
    on = pp.order_params
    lines = [f"# scripts/bench_line_order.py --reps {a.reps} --host-reps {a.host_reps}; {torch.cuda.get_device_name(0)}; "
             f"library {source_sha16()}",
             f"# {N_IMAGES} images per call, n lines each, K = n.  kernels = ops.native.order_lines (HIP events), median / minimum in us;",
             "# us/line = kernels_med / n (one image's lines: the 8 images run side by side);",
             "# pp_off / pp_on = process_padded wall time (ends in its read-back; GROUP_LINES on) with ORDER_LINES off / on, alternating,",
             "# median in us; host = order_lines_host on the same images one after the other, wall ms (median); equal = its page_rank,",
             "# page_order, block_id, block_start, block_count and forced are the kernel's on all 8 images",
             f"{'scene':<10} {'n':>5} {'blocks(img0)':>12} {'kernels_med':>11} {'kernels_min':>11} {'us/line':>8} {'pp_off':>9} {'pp_on':>9} "
             f"{'added':>8} {'host_ms':>9} {'host/kernels':>12} {'equal'}"]
    for kind, sizes in (("columns", (100, 300, 1024)), ("column", (1024,))):
        for n in sizes:
            imgs = [scene(kind, n, i) for i in range(N_IMAGES)]
            boxes = torch.from_numpy(np.stack(imgs)).to(dev)
            scores = torch.full((N_IMAGES, n), 0.9, device=dev)
            cnt = torch.full((N_IMAGES,), n, dtype=torch.int32, device=dev)
            med, mn, out = device_time(lambda: K.order_lines(boxes, cnt, None, **on), a.reps)
            ms = []
            for _ in range(a.host_reps):
                t0 = time.perf_counter()
                hs = [order_lines_host(b, on) for b in imgs]
                ms.append((time.perf_counter() - t0) * 1e3)
            host_ms = statistics.median(ms)
            got = {k: v.cpu().numpy() for k, v in out.items()}
            equal = all(int(got["block_count"][i]) == h["block_count"] and int(got["forced"][i]) == h["forced"]
                        and got["block_start"][i, :h["block_count"] + 1].tolist() == h["block_start"].tolist()
                        and all(got[k][i].tolist() == h[k].tolist() for k in INT_KEYS) for i, h in enumerate(hs))
            sizes_ = [(40000, 40000)] * N_IMAGES
            t_on, t_off = [], []
            for r in range(a.reps + 5):
                for params, ts in ((None, t_off), (on, t_on)):
                    pp.order_params = params
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    res = pp.process_padded(boxes, scores, cnt, None, None, sizes_)
                    torch.cuda.synchronize()
                    if r >= 5:
                        ts.append((time.perf_counter() - t0) * 1e6)
            assert res.words["count"].tolist() == [n] * N_IMAGES          # (no line of these scenes is merged or dropped)
            assert res.words["line_count"].tolist() == [n] * N_IMAGES     # (and every one is a line of its own)
            off_us, on_us = statistics.median(t_off), statistics.median(t_on)
            lines.append(f"{kind:<10} {n:>5} {hs[0]['block_count']:>12} {med:>11.1f} {mn:>11.1f} {med / n:>8.2f} {off_us:>9.1f} {on_us:>9.1f} "
                         f"{on_us - off_us:>8.1f} {host_ms:>9.1f} {host_ms * 1e3 / med:>11.0f}x {'yes' if equal else 'no'}")
            print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
