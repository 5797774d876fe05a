"""Word post-processor on one device: the all-in-LDS kernel (glass_postprocess_words, K <= 128), the dense kernel
(glass_postprocess_words_dense, K <= 1024) and the host path they replace (PostProcessorRotatedBoxes.host_call).

8 images of n words each, n = 100 (through both kernels: as K = 100, and zero-padded to K = 129), 128, 300, 512, 1024, for two
seeded scene types:
  sparse:    words on a jittered grid that do not touch, plus n / 25 near-duplicates (few merges, one or two iterations);
  paragraph: text lines of words that overlap their right neighbour by 0 - 50 % of the narrower word (many valid pairs,
             merges cascade along the lines).
For each: device time of ops.native.postprocess_words without text (HIP events around each call: the fill of the output
buffer plus the kernel; median and minimum of --reps after a warm-up), the words kept, and the merge iterations of image 0
(counted on the host path: one nms_rotated call per iteration).  For n <= 300 also the host wall time of host_call on the
same 8 images (--host-reps, median), and the ratio.  Writes profiles/postprocess_dense.txt.

  python scripts/bench_postprocess_dense.py [--reps 30] [--host-reps 2] [--out profiles/postprocess_dense.txt]
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

import glass_amd.postprocess.post_processor_rotated_boxes as PP
from glass_amd._lib import source_sha16
from glass_amd.config import get_glass_cfg
from glass_amd.ops import native as K
from glass_amd.structures.core import Instances, RotatedBoxes

N_IMAGES = 8


def scene(kind, n, seed):
    g = np.random.default_rng([seed, n, 0 if kind == "sparse" else 1])
    boxes = np.zeros((n, 5), np.float32)
    if kind == "sparse":
        cols = int(np.ceil(np.sqrt(n)))
        for k in range(n):
            r, c = divmod(k, cols)
            boxes[k] = [60 + 110 * c + g.uniform(-4, 4), 60 + 50 * r + g.uniform(-3, 3), g.uniform(40, 90), g.uniform(16, 28), g.uniform(-6, 6)]
        for k in g.choice(n - 1, size=max(1, n // 25), replace=False):
            boxes[k + 1] = boxes[k] + np.array([6.0, 1.0, 2.0, 0.5, 1.0], np.float32)
    else:
        x, y, k = 40.0, 60.0, 0
        per_line = max(8, int(np.sqrt(n) * 1.5))
        while k < n:
            h = g.uniform(20, 26)
            for _ in range(min(per_line, n - k)):
                w = g.uniform(40, 110)
                boxes[k] = [x + w / 2, y + g.uniform(-1.5, 1.5), w, h + g.uniform(-1, 1), g.uniform(-1.5, 1.5)]
                x += w - g.uniform(0.0, 0.5) * 40.0
                k += 1
            x, y = 40.0 + g.uniform(0, 30), y + 40.0
    scores = (g.permutation(n) / n * 0.7 + 0.28).astype(np.float32)
    return boxes, scores


def device_time(call, reps):
    for _ in range(3):
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
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "postprocess_dense.txt"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    pp = PP.PostProcessorRotatedBoxes(get_glass_cfg(os.path.join(ROOT, "configs", "glass_icdar15_mi355x.yaml"), []))
    thr = pp._thresholds()
    nms_calls = [0]
    nms = PP.nms_rotated

    def counting_nms(*args, **kw):
        nms_calls[0] += 1
        return nms(*args, **kw)
    PP.nms_rotated = counting_nms

    def host(b, s):
        inst = Instances((4000, 4000))
        inst.pred_boxes = RotatedBoxes(torch.from_numpy(b).to(dev))
        inst.scores = torch.from_numpy(s).to(dev)
        inst.pred_classes = torch.zeros(len(s), dtype=torch.int64, device=dev)
        return pp.host_call(inst)

    lines = [f"# scripts/bench_postprocess_dense.py --reps {a.reps} --host-reps {a.host_reps}; {torch.cuda.get_device_name(0)}; "
             f"library {source_sha16()}",
             f"# {N_IMAGES} images per call, n words each; device time = output fill + kernel (HIP events), median / minimum in us;",
             "# host = PostProcessorRotatedBoxes.host_call on the same images one after the other, wall ms (median); iterations = merge",
             "# iterations of image 0 (host path); ratio = host / device median; host_counts_equal: the host path keeps as many words per",
             "# image as the kernel (all 8 images when the host path was timed, image 0 otherwise)",
             f"{'scene':<10} {'n':>5} {'K':>5} {'kernel':<6} {'median_us':>10} {'min_us':>9} {'iters':>5} {'kept(img0..7)':<40} {'host_ms':>9} {'ratio':>8} {'host_counts_equal'}"]
    for kind in ("sparse", "paragraph"):
        for n in (100, 128, 300, 512, 1024):
            imgs = [scene(kind, n, i) for i in range(N_IMAGES)]
            nms_calls[0] = 0
            h0 = host(*imgs[0])
            iters = nms_calls[0]
            host_ms = None
            if n <= 300:
                ms = []
                for _ in range(a.host_reps):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    hs = [host(b, s) for b, s in imgs]
                    torch.cuda.synchronize()
                    ms.append((time.perf_counter() - t0) * 1e3)
                host_ms = statistics.median(ms)
            for K_ in ([100, 129] if n == 100 else [n]):
                boxes = torch.zeros((N_IMAGES, K_, 5))
                scores = torch.zeros((N_IMAGES, K_))
                for i, (b, s) in enumerate(imgs):
                    boxes[i, :n], scores[i, :n] = torch.from_numpy(b), torch.from_numpy(s)
                boxes, scores = boxes.to(dev), scores.to(dev)
                cnt = torch.full((N_IMAGES,), n, dtype=torch.int32, device=dev)
                med, mn, out = device_time(lambda: K.postprocess_words(boxes, scores, cnt, None, None, thr, 1), a.reps)
                kept = out["count"].tolist()
                same = kept == [len(h) for h in hs] if host_ms is not None else kept[0] == len(h0)      # counts, host path vs kernel
                lines.append(f"{kind:<10} {n:>5} {K_:>5} {'lds' if K_ <= K.POSTPROCESS_LDS_MAX_K else 'dense':<6} {med:>10.1f} {mn:>9.1f} {iters:>5} "
                             f"{str(kept):<40} {(f'{host_ms:.1f}' if host_ms is not None else '-'):>9} "
                             f"{(f'{host_ms * 1e3 / med:.0f}x' if host_ms is not None else '-'):>8} {'yes' if same else 'no'}")
                print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
