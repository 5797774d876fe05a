"""Detection ring check (glass_ring_check, csrc/ring_check.hip; RingChecker) on one device against the host loop it replaces.

Two workloads, each as det.zip lines `x1,y1,...,xn,yn,####word`:
  masks: the traced outlines of --masks synthetic word-shaped 28 x 28 probability masks (tests/mask_ring_cases.py word_masks)
         pasted onto a --size x --size image with seeded rotated boxes and polygonised by MaskPolygonizer (the case of
         scripts/bench_mask_rings.py);
  quads: --quads box quads from seeded rotated boxes (the line count profiles/rrc_score.txt was measured with).
For each, in one process:
  (a) the host path: [normalize_detection_line(l) for l in lines], host wall time, --host-reps times;
  (b) RingChecker.normalize_lines(lines): host wall time from the strings to the strings (parsing, upload, the two launches,
      the read-back, forming the lines), ended by its read-back; of it the native call alone (ops.native.ring_check on points
      that are already on the device, ended by a synchronise), and the kernels from HIP events: the whole call, and the call
      without tasks, which is the area launch alone.
Warm-up first, then the median and minimum of --reps.  The outputs of (a) and (b) are compared.

  python scripts/bench_ring_check.py [--masks 100] [--size 1000] [--quads 340000] [--reps 20] [--host-reps 1]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "glass-text-spotting_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np
import torch

from glass_amd._lib import check, lib
from glass_amd.evaluation import MaskPolygonizer, RingChecker, normalize_detection_line, rotated_boxes_to_polygons
from glass_amd.ops import native as K
from glass_amd.utils.synth import make_boxes
from mask_ring_cases import word_masks


def wall(call, reps):
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = call()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ms), min(ms), out


def to_lines(rings):
    return [",".join(f"{int(x)},{int(y)}" for x, y in r) + ",####word" for r in rings]


def kernel_events(pts, off, reps):
    """HIP-event times of glass_ring_check on device-resident inputs: (both launches, the area launch alone)"""
    L_, c_void_p, st = lib(), ctypes.c_void_p, ctypes.c_void_p(K.stream_handle())
    dev = pts.device
    task_off = K.ring_check_task_offsets(np.diff(off))
    n_rings, n_tasks = len(off) - 1, int(task_off[-1])
    d_off, d_task = K.upload(off, torch.int32, dev), K.upload(task_off, torch.int64, dev)
    verdict = torch.empty((n_rings,), dtype=torch.int32, device=dev)
    area2 = torch.empty((n_rings,), dtype=torch.int64, device=dev)
    both, area = [], []
    for rep in range(reps + 1):
        for tasks, sink in ((n_tasks, both), (0, area)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            check(L_.glass_ring_check(c_void_p(pts.data_ptr()), ctypes.c_int64(int(pts.shape[0])), c_void_p(d_off.data_ptr()), n_rings,
                                      c_void_p(d_task.data_ptr()), ctypes.c_int64(tasks), c_void_p(verdict.data_ptr()),
                                      c_void_p(area2.data_ptr()), st), "glass_ring_check")
            b.record()
            torch.cuda.synchronize()
            if rep:                                                        # the first round is the warm-up
                sink.append(a.elapsed_time(b))
    return (statistics.median(both), min(both)), (statistics.median(area), min(area)), n_tasks


def measure(name, lines, rc, reps, host_reps):
    host_ms = []
    for _ in range(host_reps):
        t0 = time.perf_counter()
        want = [normalize_detection_line(l) for l in lines]
        host_ms.append((time.perf_counter() - t0) * 1e3)
    rc.normalize_lines(lines)                                              # warm-up: code objects, allocator
    dev_med, dev_min, got = wall(lambda: rc.normalize_lines(lines), reps)
    assert got == want, f"{name}: device and host lines differ"
    flats = [[int(c) for c in l.split(",####")[0].split(",")] for l in lines]
    counts = np.array([len(f) // 2 for f in flats], dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(counts)])
    pts = K.upload(np.array([v for f in flats for v in f], dtype=np.int32).reshape(-1, 2), torch.int32, rc.device)
    K.ring_check(pts, off)
    nat_med, nat_min, _ = wall(lambda: K.ring_check(pts, off), reps)
    both, area, n_tasks = kernel_events(pts, off, reps)
    host_med = statistics.median(host_ms)
    kept = sum(1 for w in want if w is not None)
    print(f"{name}: {len(lines)} lines, {int(counts.sum())} vertices (mean {counts.mean():.0f}, longest {int(counts.max())}), "
          f"{n_tasks} pair-test tasks; {kept} lines kept, {sum(1 for w, l in zip(want, lines) if w is not None and w != l)} of them reversed")
    print(f"  (a) host list comprehension: median {host_med:.1f} ms, min {min(host_ms):.1f} ms over {host_reps}")
    print(f"  (b) RingChecker.normalize_lines, strings -> strings: median {dev_med:.3f} ms, min {dev_min:.3f} ms over {reps}; of it "
          f"native.ring_check (2 small uploads, 2 launches): median {nat_med:.3f} ms, min {nat_min:.3f} ms")
    print(f"      kernels by HIP events: both launches median {both[0]:.3f} ms (min {both[1]:.3f}), the area launch alone median "
          f"{area[0]:.3f} ms (min {area[1]:.3f})")
    print(f"  host / device = {host_med / dev_med:.1f}x; lines identical")
    return {"lines": len(lines), "vertices": int(counts.sum()), "tasks": n_tasks, "host_ms_median": round(host_med, 1),
            "device_total_ms_median": round(dev_med, 3), "native_ms_median": round(nat_med, 3),
            "kernels_ms_median": round(both[0], 3), "area_kernel_ms_median": round(area[0], 3),
            "speedup": round(host_med / dev_med, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--masks", type=int, default=100)
    ap.add_argument("--size", type=int, default=1000)
    ap.add_argument("--quads", type=int, default=340000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=1)
    ap.add_argument("--seed", type=int, default=7)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the benchmark needs a HIP device"
    dev = torch.device("cuda:0")
    rc = RingChecker(dev)
    H = W = a.size
    probs = torch.from_numpy(word_masks(a.masks, 28, a.seed)).to(dev)
    pred_masks = K.paste_rotated_masks(probs, make_boxes(5, a.masks, H, W).to(dev), (H, W), 0.5)
    mask_lines = to_lines([r for r in MaskPolygonizer(dev)(pred_masks) if len(r)])
    rng = np.random.RandomState(a.seed)
    boxes = np.stack([rng.uniform(100, 900, a.quads), rng.uniform(100, 900, a.quads), rng.uniform(20, 160, a.quads),
                      rng.uniform(8, 50, a.quads), rng.uniform(-90, 90, a.quads)], axis=1)
    quad_lines = to_lines(np.rint(rotated_boxes_to_polygons(boxes)).astype(np.int64).tolist())
    out = {"metric": "ring_check", "device": torch.cuda.get_device_name(0),
           "masks": measure("masks", mask_lines, rc, a.reps, a.host_reps),
           "quads": measure("quads", quad_lines, rc, max(a.reps // 4, 3), a.host_reps)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
