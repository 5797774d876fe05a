"""Line grouping on one device: ops.native.group_lines (glass_group_lines, csrc/line_group.hip) alone, the word
post-processor with POST_PROCESSING.GROUP_LINES on against off, and the host statement group_lines_host for scale.

8 images of n words each, n = 100, 300, 1024: seeded paragraph scenes (text lines of words that do not touch, some lines
split by a wide gap, indices shuffled), and one scene whose 1024 words are a single chain (the longest hooking sequence the
component search can meet).  For each:
  kernels:   device time of ops.native.group_lines (HIP events around each call: the two launches and the allocation of the
             outputs and the workspace; median and minimum of --reps after a warm-up);
  on / off:  host wall time of PostProcessorRotatedBoxes.process_padded (no text; the call ends in its one read-back, so it
             is synchronous) with the key on and off, the same post-processor object and build, alternating call by call;
             median of --reps each, and the difference;
  host:      wall time of group_lines_host on the same 8 images, one after the other (--host-reps, median), and whether its
             integer outputs equal the kernel's.
Writes profiles/line_grouping.txt.

  python scripts/bench_line_grouping.py [--reps 200] [--host-reps 2] [--out profiles/line_grouping.txt]
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
from glass_amd.postprocess import build_post_processor, group_lines_host

N_IMAGES = 8


def scene(kind, n, seed):
    g = np.random.default_rng([seed, n, 0 if kind == "paragraph" else 1])
    boxes = np.zeros((n, 5), np.float32)
    x, y, k = 40.0, 60.0, 0
    width = 1000.0 if kind == "paragraph" else 1e9
    while k < n:
        h = g.uniform(18, 30)
        while x < width and k < n:
            w = g.uniform(20, 90)
            boxes[k] = [x + w / 2, y + g.uniform(-0.08, 0.08) * h, w, h * g.uniform(0.9, 1.1), g.uniform(-2, 2)]
            x += w + h * (g.uniform(2.5, 4.0) if kind == "paragraph" and g.uniform() < 0.08 else g.uniform(0.25, 0.6))
            k += 1
        x, y = g.uniform(20, 120), y + h * g.uniform(1.9, 2.4)
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "line_grouping.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_line_grouping.py needs a HIP device: there is nothing to time without one")
    dev = torch.device("cuda:0")
    path = os.path.join(ROOT, "configs", "glass_icdar15_mi355x.yaml")
    pp = build_post_processor(get_glass_cfg(path, ["POST_PROCESSING.GROUP_LINES", True]))
    pp.text_threshold = None
    on = pp.line_params
    lines = [f"# scripts/bench_line_grouping.py --reps {a.reps} --host-reps {a.host_reps}; {torch.cuda.get_device_name(0)}; "
             f"library {source_sha16()}",
             f"# {N_IMAGES} images per call, n words each, K = n.  kernels = ops.native.group_lines (HIP events), median / minimum in us;",
             "# pp_off / pp_on = process_padded wall time (ends in its read-back) with GROUP_LINES off / on, alternating, median in us;",
             "# host = group_lines_host on the same images one after the other, wall ms (median); equal = its line_id, line_pos, order",
             "# and line_start are the kernel's on all 8 images",
             f"{'scene':<10} {'n':>5} {'lines(img0)':>11} {'kernels_med':>11} {'kernels_min':>11} {'pp_off':>9} {'pp_on':>9} {'added':>8} "
             f"{'host_ms':>9} {'host/kernels':>12} {'equal'}"]
    for kind, sizes in (("paragraph", (100, 300, 1024)), ("chain", (1024,))):
        for n in sizes:
            imgs = [scene(kind, n, i) for i in range(N_IMAGES)]
            boxes = torch.from_numpy(np.stack(imgs)).to(dev)
            scores = torch.full((N_IMAGES, n), 0.9, device=dev)
            cnt = torch.full((N_IMAGES,), n, dtype=torch.int32, device=dev)
            med, mn, out = device_time(lambda: K.group_lines(boxes, cnt, **on), a.reps)
            ms = []
            for _ in range(a.host_reps):
                t0 = time.perf_counter()
                hs = [group_lines_host(b, on) for b in imgs]
                ms.append((time.perf_counter() - t0) * 1e3)
            host_ms = statistics.median(ms)
            got = {k: v.cpu().numpy() for k, v in out.items()}
            equal = all(int(got["line_count"][i]) == h["line_count"] and got["line_start"][i, :h["line_count"] + 1].tolist() == h["line_start"].tolist()
                        and all(got[k][i].tolist() == h[k].tolist() for k in ("line_id", "line_pos", "order")) for i, h in enumerate(hs))
            sizes_ = [(4000, 4000)] * N_IMAGES
            t_on, t_off = [], []
            for r in range(a.reps + 5):
                for params, ts in ((None, t_off), (on, t_on)):
                    pp.line_params = params
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    res = pp.process_padded(boxes, scores, cnt, None, None, sizes_)
                    torch.cuda.synchronize()
                    if r >= 5:
                        ts.append((time.perf_counter() - t0) * 1e6)
            assert res.words["count"].tolist() == [n] * N_IMAGES          # (no word of these scenes is merged or dropped)
            off_us, on_us = statistics.median(t_off), statistics.median(t_on)
            lines.append(f"{kind:<10} {n:>5} {hs[0]['line_count']:>11} {med:>11.1f} {mn:>11.1f} {off_us:>9.1f} {on_us:>9.1f} {on_us - off_us:>8.1f} "
                         f"{host_ms:>9.1f} {host_ms * 1e3 / med:>11.0f}x {'yes' if equal else 'no'}")
            print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
