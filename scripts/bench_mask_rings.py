"""Mask polygonisation (glass_mask_windows / glass_mask_rings_count / glass_mask_rings_write, csrc/mask_rings.hip;
MaskPolygonizer) on one device against the host path it replaces.

The case: --masks synthetic word-shaped 28 x 28 probability masks (tests/mask_ring_cases.py word_masks) pasted by
paste_rotated_masks onto a --size x --size image with seeded rotated boxes: `pred_masks` as the model leaves it, a bool
[R, H, W] device tensor.  In one process:
  (a) the host path: `pred_masks.cpu().numpy()` (timed alone: the device-to-host copy) and then `masks_to_polygons`;
  (b) `MaskPolygonizer` from the device tensor to the Python lists (host wall time, ended by its downloads), the native
      calls alone from HIP events, and the three stages (window pass, labels + counting walk, writing walk) from events.
Warm-up first, then the median and minimum of --reps; the host tracer runs --host-reps times.  The rings of (a) and (b) are
compared.

  python scripts/bench_mask_rings.py [--masks 100] [--size 1000] [--reps 20] [--host-reps 2]
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
from glass_amd.evaluation import MaskPolygonizer, masks_to_polygons
from glass_amd.ops import native as K
from glass_amd.utils.synth import make_boxes
from mask_ring_cases import lds_words, word_masks


def wall(call, reps):
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = call()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ms), min(ms), out


def stages(masks, reps):
    """HIP-event times of the three native calls of ops.native.mask_rings, with its buffers and sizes"""
    R, H, W = (int(v) for v in masks.shape)
    L_, c_void_p, st = lib(), ctypes.c_void_p, ctypes.c_void_p(K.stream_handle())
    dev = masks.device
    win = torch.empty((R, 4), dtype=torch.int32, device=dev)
    meta = torch.empty((R + 2,), dtype=torch.int32, device=dev)
    status = c_void_p(meta.data_ptr() + 4 * (R + 1))
    times = {"window": [], "label_count": [], "write": []}
    for rep in range(reps + 1):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        ev[0].record()
        check(L_.glass_mask_windows(c_void_p(masks.data_ptr()), R, H, W, c_void_p(win.data_ptr()), st), "glass_mask_windows")
        ev[1].record()
        win_host = win.cpu()
        ws_bytes = int(L_.glass_mask_rings_workspace_bytes(c_void_p(win_host.data_ptr()), R, H, W))
        ws = torch.empty((ws_bytes // 8,), dtype=torch.int64, device=dev)
        a = torch.cuda.Event(enable_timing=True)
        a.record()
        check(L_.glass_mask_rings_count(c_void_p(masks.data_ptr()), R, H, W, c_void_p(win.data_ptr()), c_void_p(ws.data_ptr()),
                                        ctypes.c_int64(ws_bytes), c_void_p(meta.data_ptr()), status, st), "glass_mask_rings_count")
        ev[2].record()
        total, code = (int(v) for v in meta[R:].cpu())
        assert code == 0, code
        xy = torch.empty((total, 2), dtype=torch.int32, device=dev)
        b = torch.cuda.Event(enable_timing=True)
        b.record()
        check(L_.glass_mask_rings_write(R, H, W, c_void_p(win.data_ptr()), c_void_p(ws.data_ptr()), ctypes.c_int64(ws_bytes),
                                        c_void_p(meta.data_ptr()), c_void_p(xy.data_ptr()), ctypes.c_int64(total), status, st),
              "glass_mask_rings_write")
        ev[3].record()
        torch.cuda.synchronize()
        if rep:                                                            # the first round is the warm-up
            times["window"].append(ev[0].elapsed_time(ev[1]))
            times["label_count"].append(a.elapsed_time(ev[2]))
            times["write"].append(b.elapsed_time(ev[3]))
    return {k: (statistics.median(v), min(v)) for k, v in times.items()}, ws_bytes, total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--masks", type=int, default=100)
    ap.add_argument("--size", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--seed", type=int, default=7)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the benchmark needs a HIP device"
    dev = torch.device("cuda:0")
    H = W = a.size
    probs = torch.from_numpy(word_masks(a.masks, 28, a.seed)).to(dev)
    boxes = make_boxes(5, a.masks, H, W).to(dev)
    pred_masks = K.paste_rotated_masks(probs, boxes, (H, W), 0.5)
    torch.cuda.synchronize()
    poly = MaskPolygonizer(dev)

    poly(pred_masks)                                                       # warm-up: code objects, allocator
    pred_masks.cpu()
    copy_med, copy_min, host_masks = wall(lambda: pred_masks.cpu().numpy(), a.reps)
    dev_med, dev_min, rings = wall(lambda: poly(pred_masks), a.reps)
    nat_med, nat_min, _ = wall(lambda: K.mask_rings(pred_masks), a.reps)
    st, ws_bytes, total = stages(pred_masks, a.reps)
    host_ms = []
    for _ in range(a.host_reps):
        t0 = time.perf_counter()
        host_rings = masks_to_polygons(host_masks)
        host_ms.append((time.perf_counter() - t0) * 1e3)
    assert rings == host_rings, "device and host rings differ"
    lens = [len(r) for r in rings]
    words = [lds_words(m) for m in host_masks]
    kern = sum(v[0] for v in st.values())
    print(f"case: {a.masks} masks on {H} x {W} ({pred_masks.numel() / 1e6:.0f} MB), {sum(1 for n in lens if n)} non-empty rings, "
          f"mean {np.mean(lens):.0f} vertices, longest {max(lens)}, {total} in all; windows of {int(np.mean(words))} LDS words on "
          f"average, {max(words)} at most (limit {K.MASK_RINGS_LDS_WORDS}); workspace {ws_bytes / 1e6:.2f} MB")
    print(f"  (a) host path: device-to-host copy median {copy_med:.2f} ms, min {copy_min:.2f} ms over {a.reps} reps; "
          f"masks_to_polygons median {statistics.median(host_ms):.0f} ms, min {min(host_ms):.0f} ms over {a.host_reps}")
    print(f"  (b) MaskPolygonizer, device tensor -> lists: median {dev_med:.3f} ms, min {dev_min:.3f} ms; "
          f"of it native.mask_rings (3 calls, 2 small read-backs): median {nat_med:.3f} ms, min {nat_min:.3f} ms")
    print("      kernels by HIP events: " + ", ".join(f"{k} median {v[0]:.3f} ms (min {v[1]:.3f})" for k, v in st.items()) +
          f"; sum of medians {kern:.3f} ms")
    print(f"  device total / copy alone = {dev_med / copy_med:.3f}; host path / device total = "
          f"{(copy_med + statistics.median(host_ms)) / dev_med:.0f}x; rings identical")
    print(json.dumps({"metric": "mask_rings", "device": torch.cuda.get_device_name(0), "masks": a.masks, "size": a.size,
                      "vertices": total, "copy_ms_median": round(copy_med, 3), "host_trace_ms_median": round(statistics.median(host_ms), 1),
                      "device_total_ms_median": round(dev_med, 3), "native_ms_median": round(nat_med, 3),
                      "window_ms_median": round(st["window"][0], 3), "label_count_ms_median": round(st["label_count"][0], 3),
                      "write_ms_median": round(st["write"][0], 3), "faster_than_copy_alone": bool(dev_med < copy_med)}))


if __name__ == "__main__":
    main()
