"""Ring simplification on the device (glass_ring_simplify_mark / glass_ring_simplify_write, csrc/ring_simplify.hip;
ops.native.simplify_rings, MaskPolygonizer(simplify=)) on one device against the unsimplified path of the same build.

The two workloads of scripts/bench_roi_mask_rings.py (synthetic word-shaped 28 x 28 probability masks, tests/mask_ring_cases.py
word_masks, and seeded rotated boxes, traced by MaskPolygonizer.from_rois): 100 masks on 1000 x 1000, and 1024 on 2000 x 3000.
In one process, per workload and per tolerance (0.5, 1 and 2 px):
  - the vertices before and after, and how many rings `keep_valid` returned unsimplified;
  - the two native calls alone, by HIP events (mark: flags, counts and the running sum; write: the compaction);
  - device tensors -> Python lists: `MaskPolygonizer(dev).from_rois` (the baseline: the parent's code, unchanged) and
    `MaskPolygonizer(dev, simplify=tol).from_rois`, alternating repetition by repetition on the same inputs, host wall time
    ended by a device synchronise; with `keep_valid=False` as well;
  - `RingChecker.normalize_lines` on the det lines of the resulting rings, both ways.
Warm-up first, then medians and minima.

  python scripts/bench_ring_simplify.py [--reps 20] [--big-reps 5] [--case both|small|big]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "glass-text-spotting_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch

from glass_amd._lib import check, lib
from glass_amd.evaluation import MaskPolygonizer, RingChecker
from glass_amd.evaluation.ring_simplify import tolerance_q4
from glass_amd.ops import native as K
from glass_amd.utils.synth import make_boxes
from mask_ring_cases import word_masks

TOLERANCES = (0.5, 1, 2)


def timed(call):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = call()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def med_min(v):
    return statistics.median(v), min(v)


def kernel_times(xy, ring_off, tol, reps):
    """HIP-event times of the two native calls of ops.native.simplify_rings, and the kept total"""
    V, R = int(xy.shape[0]), int(ring_off.shape[0]) - 1
    L_, st, dev = lib(), K.stream_handle(), xy.device
    ws_bytes = int(L_.glass_ring_simplify_workspace_bytes(V, R))
    ws = torch.empty((ws_bytes // 8,), dtype=torch.int64, device=dev)
    meta = torch.empty((R + 2,), dtype=torch.int32, device=dev)
    status = meta.data_ptr() + 4 * (R + 1)
    mark, write = [], []
    for rep in range(reps + 1):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        ev[0].record()
        check(L_.glass_ring_simplify_mark(xy.data_ptr(), V, ring_off.data_ptr(), R, tolerance_q4(tol), ws.data_ptr(), ws_bytes,
                                          meta.data_ptr(), status, st), "glass_ring_simplify_mark")
        ev[1].record()
        total, code = (int(v) for v in meta[R:].cpu())
        assert code == 0, code
        out = torch.empty((total, 2), dtype=torch.int32, device=dev)
        ev[2].record()
        check(L_.glass_ring_simplify_write(xy.data_ptr(), V, ring_off.data_ptr(), R, ws.data_ptr(), ws_bytes, meta.data_ptr(),
                                           out.data_ptr(), total, st), "glass_ring_simplify_write")
        ev[3].record()
        torch.cuda.synchronize()
        if rep:                                                            # the first round is the warm-up
            mark.append(ev[0].elapsed_time(ev[1]))
            write.append(ev[2].elapsed_time(ev[3]))
    return med_min(mark), med_min(write), total


def det_lines(rings):
    return [",".join(f"{int(x)},{int(y)}" for x, y in r) + ",####word" for r in rings if len(r) >= 3]


def case(R, H, W, reps, seed=7):
    dev = torch.device("cuda:0")
    probs = torch.from_numpy(word_masks(R, 28, seed)).to(dev)
    boxes = make_boxes(5, R, H, W).to(dev)
    plain = MaskPolygonizer(dev)
    checker = RingChecker(dev)
    xy, ring_off = K.roi_mask_rings(probs, boxes, (H, W), 0.5)
    lens = (ring_off[1:] - ring_off[:-1]).cpu().tolist()
    V = int(xy.shape[0])
    print(f"case: {R} masks on {H} x {W}, {sum(1 for n in lens if n)} non-empty rings, {V} vertices, longest {max(lens)}; "
          f"{reps} alternating repetitions")
    base_rings = plain.from_rois(probs, boxes, (H, W), 0.5)               # warm-up: code objects, allocator
    base_lines = det_lines(base_rings)
    checker.normalize_lines(base_lines)
    for tol in TOLERANCES:
        poly, loose = MaskPolygonizer(dev, simplify=tol), MaskPolygonizer(dev, simplify=tol, keep_valid=False)
        rings = poly.from_rois(probs, boxes, (H, W), 0.5)
        restored = poly.restored
        loose.from_rois(probs, boxes, (H, W), 0.5)
        lines = det_lines(rings)
        assert len(lines) == len(base_lines)
        checker.normalize_lines(lines)
        t = {"base": [], "simplify": [], "loose": [], "norm_base": [], "norm_simplify": []}
        for _ in range(reps):
            t["base"].append(timed(lambda: plain.from_rois(probs, boxes, (H, W), 0.5))[0])
            t["simplify"].append(timed(lambda: poly.from_rois(probs, boxes, (H, W), 0.5))[0])
            t["loose"].append(timed(lambda: loose.from_rois(probs, boxes, (H, W), 0.5))[0])
            t["norm_base"].append(timed(lambda: checker.normalize_lines(base_lines))[0])
            ms, normalized = timed(lambda: checker.normalize_lines(lines))
            t["norm_simplify"].append(ms)
        base_kept = sum(1 for l in checker.normalize_lines(base_lines) if l is not None)
        kept = sum(1 for l in normalized if l is not None)
        mark, write, total = kernel_times(xy, ring_off, tol, reps)
        after = sum(len(r) for r in rings)
        m = {k: med_min(v) for k, v in t.items()}
        print(f"  tolerance {tol} px: {V} -> {total} vertices ({V / max(total, 1):.2f}x fewer; {after} after keep_valid restored "
              f"{restored} rings); longest ring {max(len(r) for r in rings)}")
        print(f"      kernels by HIP events: mark median {mark[0]:.3f} ms (min {mark[1]:.3f}), write median {write[0]:.3f} ms "
              f"(min {write[1]:.3f})")
        print(f"      device tensors -> lists: unsimplified median {m['base'][0]:.3f} ms (min {m['base'][1]:.3f}); simplify "
              f"median {m['simplify'][0]:.3f} ms (min {m['simplify'][1]:.3f}); simplify, keep_valid=False median "
              f"{m['loose'][0]:.3f} ms (min {m['loose'][1]:.3f})")
        print(f"      RingChecker.normalize_lines on {len(lines)} lines: unsimplified median {m['norm_base'][0]:.3f} ms (min "
              f"{m['norm_base'][1]:.3f}), simplified median {m['norm_simplify'][0]:.3f} ms (min {m['norm_simplify'][1]:.3f}); lines "
              f"kept {base_kept} unsimplified, {kept} simplified")
        print(json.dumps({"metric": "ring_simplify", "device": torch.cuda.get_device_name(0), "masks": R, "height": H, "width": W,
                          "tolerance": tol, "vertices": V, "vertices_simplified": total, "vertices_returned": after,
                          "restored": restored, "mark_ms_median": round(mark[0], 3), "write_ms_median": round(write[0], 3),
                          "lists_ms_median": round(m["base"][0], 3), "lists_simplify_ms_median": round(m["simplify"][0], 3),
                          "lists_simplify_loose_ms_median": round(m["loose"][0], 3),
                          "normalize_ms_median": round(m["norm_base"][0], 3),
                          "normalize_simplify_ms_median": round(m["norm_simplify"][0], 3), "lines_kept": base_kept,
                          "lines_kept_simplified": kept}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--big-reps", type=int, default=5)
    ap.add_argument("--case", choices=("both", "small", "big"), default="both")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the benchmark needs a HIP device"
    if a.case in ("both", "small"):
        case(100, 1000, 1000, a.reps)
    if a.case in ("both", "big"):
        case(1024, 2000, 3000, a.big_reps)


if __name__ == "__main__":
    main()
