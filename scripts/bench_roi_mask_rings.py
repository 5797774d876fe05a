"""Mask polygons straight from the RoI masks (glass_roi_mask_windows / glass_roi_mask_rings_count / glass_mask_rings_write,
csrc/mask_rings.hip; ops.native.roi_mask_rings, MaskPolygonizer.from_rois) on one device against the two-step path of the
same build: paste_rotated_masks into a bool [R, H, W] tensor, then mask_rings on it.

Two cases, the inputs of both paths being the same device tensors (synthetic word-shaped 28 x 28 probability masks,
tests/mask_ring_cases.py word_masks, and seeded rotated boxes): 100 masks on 1000 x 1000, and 1024 on 2000 x 3000.  In one
process, after a warm-up, the two paths alternate repetition by repetition:
  (a) paste + MaskPolygonizer.__call__: device tensors -> Python lists (host wall time, ended by its downloads);
  (b) MaskPolygonizer.from_rois: the same.
Then the native calls of each path alone, stage by stage, from HIP events, and the peak device memory each path adds
(torch.cuda.max_memory_allocated above what is allocated before the call).  The rings of (a) and (b) are compared.

  python scripts/bench_roi_mask_rings.py [--reps 20] [--big-reps 5] [--case both|small|big]
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

import torch

from glass_amd._lib import check, lib
from glass_amd.evaluation import MaskPolygonizer
from glass_amd.ops import native as K
from glass_amd.utils.synth import make_boxes
from mask_ring_cases import word_masks


def timed(call):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = call()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def peak(call):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = call()
    torch.cuda.synchronize()
    added = torch.cuda.max_memory_allocated() - before
    del out
    return added


def stages(probs, boxes, hw, roi, reps):
    """HIP-event times of the native calls of one path, with the wrappers' buffers and sizes"""
    R, M, (H, W) = int(probs.shape[0]), int(probs.shape[1]), hw
    L_, vp, st = lib(), ctypes.c_void_p, ctypes.c_void_p(K.stream_handle())
    dev = probs.device
    win = torch.empty((R, 4), dtype=torch.int32, device=dev)
    meta = torch.empty((R + 2,), dtype=torch.int32, device=dev)
    status = vp(meta.data_ptr() + 4 * (R + 1))
    times = {"paste": [], "window": [], "label_count": [], "write": []}
    ws_bytes = 0
    for rep in range(reps + 1):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(8)]
        pasted = None
        ev[0].record()
        if not roi:
            pasted = K.paste_rotated_masks(probs, boxes, hw, 0.5)
        ev[1].record()
        if roi:
            check(L_.glass_roi_mask_windows(vp(probs.data_ptr()), vp(boxes.data_ptr()), R, M, H, W, 0.5, vp(win.data_ptr()), st), "windows")
        else:
            check(L_.glass_mask_windows(vp(pasted.data_ptr()), R, H, W, vp(win.data_ptr()), st), "windows")
        ev[2].record()
        win_host = win.cpu()
        ws_bytes = int(L_.glass_mask_rings_workspace_bytes(vp(win_host.data_ptr()), R, H, W))
        ws = torch.empty((ws_bytes // 8,), dtype=torch.int64, device=dev)
        ev[3].record()
        if roi:
            check(L_.glass_roi_mask_rings_count(vp(probs.data_ptr()), vp(boxes.data_ptr()), R, M, H, W, 0.5, vp(win.data_ptr()),
                                                vp(ws.data_ptr()), ctypes.c_int64(ws_bytes), vp(meta.data_ptr()), status, st), "count")
        else:
            check(L_.glass_mask_rings_count(vp(pasted.data_ptr()), R, H, W, vp(win.data_ptr()), vp(ws.data_ptr()),
                                            ctypes.c_int64(ws_bytes), vp(meta.data_ptr()), status, st), "count")
        ev[4].record()
        total, code = (int(v) for v in meta[R:].cpu())
        assert code == 0, code
        xy = torch.empty((total, 2), dtype=torch.int32, device=dev)
        ev[5].record()
        check(L_.glass_mask_rings_write(R, H, W, vp(win.data_ptr()), vp(ws.data_ptr()), ctypes.c_int64(ws_bytes), vp(meta.data_ptr()),
                                        vp(xy.data_ptr()), ctypes.c_int64(total), status, st), "write")
        ev[6].record()
        torch.cuda.synchronize()
        if rep:                                                            # the first round is the warm-up
            times["paste"].append(ev[0].elapsed_time(ev[1]))
            times["window"].append(ev[1].elapsed_time(ev[2]))
            times["label_count"].append(ev[3].elapsed_time(ev[4]))
            times["write"].append(ev[5].elapsed_time(ev[6]))
        del pasted, ws, xy
    return {k: (statistics.median(v), min(v)) for k, v in times.items()}, ws_bytes


def case(R, H, W, reps, seed=7):
    dev = torch.device("cuda:0")
    probs = torch.from_numpy(word_masks(R, 28, seed)).to(dev)
    boxes = make_boxes(5, R, H, W).to(dev)
    poly = MaskPolygonizer(dev)
    two_step = lambda: poly(K.paste_rotated_masks(probs, boxes, (H, W), 0.5))
    direct = lambda: poly.from_rois(probs, boxes, (H, W), 0.5)
    want, got = two_step(), direct()                                       # warm-up: code objects, allocator
    assert got == want, "the rings of the two paths differ"
    a_ms, b_ms = [], []
    for _ in range(reps):                                                  # alternating
        a_ms.append(timed(two_step)[0])
        b_ms.append(timed(direct)[0])
    a_st, ws_a = stages(probs, boxes, (H, W), False, reps)
    b_st, ws_b = stages(probs, boxes, (H, W), True, reps)
    assert ws_a == ws_b                                                    # the same windows
    a_mem = peak(lambda: K.mask_rings(K.paste_rotated_masks(probs, boxes, (H, W), 0.5)))
    b_mem = peak(lambda: K.roi_mask_rings(probs, boxes, (H, W), 0.5))
    lens = [len(r) for r in want]
    fmt = lambda st, keys: ", ".join(f"{k} median {st[k][0]:.3f} ms (min {st[k][1]:.3f})" for k in keys)
    a_k, b_k = sum(a_st[k][0] for k in a_st), sum(b_st[k][0] for k in ("window", "label_count", "write"))
    print(f"case: {R} masks on {H} x {W} (pasted: {R * H * W / 1e6:.0f} MB), {sum(1 for n in lens if n)} non-empty rings, "
          f"{sum(lens)} vertices, longest {max(lens)}; workspace {ws_b / 1e6:.2f} MB; {reps} alternating repetitions")
    print(f"  (a) paste_rotated_masks + mask_rings, device tensors -> lists: median {statistics.median(a_ms):.3f} ms, min {min(a_ms):.3f} ms; "
          f"peak extra device memory {a_mem / 1e6:.2f} MB")
    print(f"      kernels by HIP events: {fmt(a_st, ('paste', 'window', 'label_count', 'write'))}; sum of medians {a_k:.3f} ms")
    print(f"  (b) roi_mask_rings, device tensors -> lists: median {statistics.median(b_ms):.3f} ms, min {min(b_ms):.3f} ms; "
          f"peak extra device memory {b_mem / 1e6:.2f} MB")
    print(f"      kernels by HIP events: {fmt(b_st, ('window', 'label_count', 'write'))}; sum of medians {b_k:.3f} ms")
    print(f"  (b) / (a): time {statistics.median(b_ms) / statistics.median(a_ms):.3f}, kernels {b_k / a_k:.3f}, memory {b_mem / a_mem:.4f}; rings identical")
    print(json.dumps({"metric": "roi_mask_rings", "device": torch.cuda.get_device_name(0), "masks": R, "height": H, "width": W,
                      "vertices": sum(lens), "two_step_ms_median": round(statistics.median(a_ms), 3),
                      "roi_ms_median": round(statistics.median(b_ms), 3), "two_step_kernels_ms": round(a_k, 3),
                      "roi_kernels_ms": round(b_k, 3), "two_step_peak_bytes": a_mem, "roi_peak_bytes": b_mem,
                      **{f"two_step_{k}_ms": round(v[0], 3) for k, v in a_st.items()},
                      **{f"roi_{k}_ms": round(b_st[k][0], 3) for k in ("window", "label_count", "write")}}))


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
