"""Rows, cells, tables and columns on one device: ops.native.row_grid (glass_row_grid, csrc/row_grid.hip) alone, the word
post-processor with POST_PROCESSING.ALIGN_ROWS on against off (GROUP_LINES on in both), and the host statement row_grid_host
for scale.

8 images of n lines each, n = 100, 300, 1024: seeded receipt-like pages (item / amount pairs, now and then a continuation
line or a heading of its own, a wider gap between groups, indices shuffled), and one scene whose 1024 lines are a staircase
(every line a row-mate of its two neighbours only: one row of diameter 1023, the longest way a label can have to travel).
For each:
  kernels:   device time of ops.native.row_grid (HIP events around each call: the three launches and the allocation of the
             outputs and the workspace; median and minimum of --reps after a warm-up);
  on / off:  host wall time of PostProcessorRotatedBoxes.process_padded (no text; the call ends in its one read-back, so it
             is synchronous) on the same boxes as words - every word is a line of its own, so the page has n lines - with the
             key on and off, the same post-processor object and build, alternating call by call; median of --reps each.  Not
             for the staircase, whose neighbours the line grouping would join into lines;
  host:      wall time of row_grid_host on the same 8 images, one after the other (--host-reps, median), and whether its
             integer outputs equal the kernel's.
Writes profiles/row_grid.txt.  With --trace SCENE:N the script only calls ops.native.row_grid --reps times on that scene (for a
kernel trace in a run of its own) and writes nothing.

  python scripts/bench_row_grid.py [--reps 200] [--host-reps 2] [--out profiles/row_grid.txt] [--trace staircase:1024]
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
from glass_amd.postprocess import build_post_processor, row_grid_host

N_IMAGES = 8
INT_KEYS = ("row_id", "row_pos", "table_id", "col_id", "row_order")


def scene(kind, n, seed):
    g = np.random.default_rng([seed, n, 0 if kind == "receipt" else 1])
    rows = []
    if kind == "staircase":
        rows = [[30.0 * k + g.uniform(-2, 2), 100.0 + 8.0 * k + g.uniform(-0.3, 0.3), g.uniform(16, 22), 20.0, g.uniform(-0.2, 0.2)]
                for k in range(n)]
    y, k = 40.0, 0
    while len(rows) < n:
        kind_k = k % 7
        h = lambda: 20.0 * g.uniform(0.97, 1.03)
        if kind_k in (3, 6) or len(rows) + 1 == n:                     # a continuation line, or a heading of its own
            w = g.uniform(100, 200)
            rows.append([(60.0 if kind_k == 3 else 0.0) + w / 2, y + g.uniform(-0.4, 0.4), w, h(), g.uniform(-0.4, 0.4)])
        else:
            w, pw = g.uniform(40, 180), g.uniform(40, 60)
            rows.append([40.0 + w / 2, y + g.uniform(-0.4, 0.4), w, h(), g.uniform(-0.4, 0.4)])
            rows.append([420.0 - pw / 2, y + g.uniform(-0.4, 0.4), pw, h(), g.uniform(-0.4, 0.4)])
        y += 28.0 + (70.0 if kind_k == 6 else 0.0)
        k += 1
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "row_grid.txt"))
    ap.add_argument("--trace", default=None, help="SCENE:N - only call ops.native.row_grid on that scene")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_row_grid.py needs a HIP device: there is nothing to time without one")
    dev = torch.device("cuda:0")
    if a.trace:
        kind, n = a.trace.split(":")
        boxes = torch.from_numpy(np.stack([scene(kind, int(n), i) for i in range(N_IMAGES)])).to(dev)
        cnt = torch.full((N_IMAGES,), int(n), dtype=torch.int32, device=dev)
        for _ in range(a.reps):
            K.row_grid(boxes, cnt, None)
        torch.cuda.synchronize()
        return
    path = os.path.join(ROOT, "configs", "glass_icdar15_mi355x.yaml")
    pp = build_post_processor(get_glass_cfg(path, ["POST_PROCESSING.GROUP_LINES", True, "POST_PROCESSING.ALIGN_ROWS", True]))
    pp.text_threshold = None
    on = pp.grid_params
    lines = [f"# scripts/bench_row_grid.py --reps {a.reps} --host-reps {a.host_reps}; {torch.cuda.get_device_name(0)}; "
             f"library {source_sha16()}",
             f"# {N_IMAGES} images per call, n lines each, K = n.  kernels = ops.native.row_grid (HIP events), median / minimum in us;",
             "# pp_off / pp_on = process_padded wall time (ends in its read-back; GROUP_LINES on) with ALIGN_ROWS off / on, alternating,",
             "# median in us (not for the staircase: the line grouping would join its neighbours); host = row_grid_host on the same",
             "# images one after the other, wall ms (median); equal = its row_id, row_pos, table_id, col_id, row_order, row_start,",
             "# table_rows, table_cols and the two counts are the kernel's on all 8 images",
             f"{'scene':<10} {'n':>5} {'rows(img0)':>10} {'tables(img0)':>12} {'kernels_med':>11} {'kernels_min':>11} {'pp_off':>9} {'pp_on':>9} "
             f"{'added':>8} {'host_ms':>9} {'host/kernels':>12} {'equal'}"]
    for kind, sizes in (("receipt", (100, 300, 1024)), ("staircase", (1024,))):
        for n in sizes:
            imgs = [scene(kind, n, i) for i in range(N_IMAGES)]
            boxes = torch.from_numpy(np.stack(imgs)).to(dev)
            scores = torch.full((N_IMAGES, n), 0.9, device=dev)
            cnt = torch.full((N_IMAGES,), n, dtype=torch.int32, device=dev)
            med, mn, out = device_time(lambda: K.row_grid(boxes, cnt, None, **on), a.reps)
            ms = []
            for _ in range(a.host_reps):
                t0 = time.perf_counter()
                hs = [row_grid_host(b, on) for b in imgs]
                ms.append((time.perf_counter() - t0) * 1e3)
            host_ms = statistics.median(ms)
            got = {k: v.cpu().numpy() for k, v in out.items()}
            equal = all(int(got["row_count"][i]) == h["row_count"] and int(got["table_count"][i]) == h["table_count"]
                        and got["row_start"][i, :h["row_count"] + 1].tolist() == h["row_start"].tolist()
                        and got["table_rows"][i, :h["table_count"]].tolist() == h["table_rows"].tolist()
                        and got["table_cols"][i, :h["table_count"]].tolist() == h["table_cols"].tolist()
                        and all(got[k][i].tolist() == h[k].tolist() for k in INT_KEYS) for i, h in enumerate(hs))
            pp_cols = f"{'-':>9} {'-':>9} {'-':>8}"
            if kind == "receipt":
                sizes_ = [(40000, 40000)] * N_IMAGES
                t_on, t_off = [], []
                for r in range(a.reps + 5):
                    for params, ts in ((None, t_off), (on, t_on)):
                        pp.grid_params = params
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        res = pp.process_padded(boxes, scores, cnt, None, None, sizes_)
                        torch.cuda.synchronize()
                        if r >= 5:
                            ts.append((time.perf_counter() - t0) * 1e6)
                assert res.words["count"].tolist() == [n] * N_IMAGES          # (no line of these scenes is merged or dropped)
                assert res.words["line_count"].tolist() == [n] * N_IMAGES     # (and every one is a line of its own)
                off_us, on_us = statistics.median(t_off), statistics.median(t_on)
                pp_cols = f"{off_us:>9.1f} {on_us:>9.1f} {on_us - off_us:>8.1f}"
            lines.append(f"{kind:<10} {n:>5} {hs[0]['row_count']:>10} {hs[0]['table_count']:>12} {med:>11.1f} {mn:>11.1f} {pp_cols} "
                         f"{host_ms:>9.1f} {host_ms * 1e3 / med:>11.0f}x {'yes' if equal else 'no'}")
            print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
