"""Test-time ResizeShortestEdge front end (glass_resize_u8_pil_into_batch, csrc/resize_pil.hip) on one device against the
only other way to get the same bytes, PIL on the host.

Two workloads: --images (8) uint8 images of 720 x 1280 resized to short side 1000 (1000 x 1778, the evaluation protocol's
IC15 shape), and one 2000 x 3000 image reduced to short side 1000 (1000 x 1500).  For each, in one process, alternating:
  (a) fused:  ops.native.pil_resize_into_batch per image, from the uint8 image already on the device to its slot of the
              padded float NHWC4 batch (two launches per image); host wall time ended by a synchronise, and HIP events;
  (b) PIL:    PIL.Image.resize(BILINEAR) on this machine's host, the H2D copy of its result, the cast to float CHW and
              ops.native.preprocess_image; wall time ended by a synchronise, the PIL part of it also on its own;
  (c) scale:  the GlassRunner front end at the same output size, ops.native.image_u8hwc_to_chw + preprocess_image: different
              arithmetic (F.interpolate bilinear, no anti-aliasing), here only to say what a front end of this size costs.
(a) and (b) are compared bit for bit.  Warm-up first, then the median and minimum of --reps.

  python scripts/bench_resize_pil.py [--images 8] [--reps 20] [--warmup 3] [--step-ms 25.3]
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
from PIL import Image

from glass_amd.data import ResizeShortestEdge
from glass_amd.ops import native as K
from glass_amd.utils.synth import make_image

MEAN, STD = [103.53, 116.28, 123.675], [57.375, 57.12, 58.395]
BILINEAR = getattr(Image, "Resampling", Image).BILINEAR


def wall(call):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    call()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def events(call):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    call()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def measure(name, hw, count, reps, warmup, step_ms):
    dev = torch.device("cuda:0")
    H, W = hw
    Ho, Wo = ResizeShortestEdge(1000, 1000000).get_output_shape(H, W)
    Hp, Wp = (Ho + 31) // 32 * 32, (Wo + 31) // 32 * 32
    host = [make_image(i, H, W).numpy() for i in range(count)]
    u8 = [torch.from_numpy(h).to(dev) for h in host]
    pil = [Image.fromarray(h) for h in host]
    batch_a = torch.empty((count, Hp, Wp, 4), dtype=torch.float32, device=dev)
    batch_b, batch_c = torch.empty_like(batch_a), torch.empty_like(batch_a)
    ws = K.pil_resize_workspace(H, W, Ho, Wo, dev)
    pil_ms = []

    def fused():
        for n, im in enumerate(u8):
            K.pil_resize_into_batch(im, (Ho, Wo), MEAN, STD, batch_a, n, workspace=ws)

    def through_pil():
        t0 = time.perf_counter()
        small = [np.array(p.resize((Wo, Ho), BILINEAR)) for p in pil]
        pil_ms.append((time.perf_counter() - t0) * 1e3)
        for n, s in enumerate(small):
            K.preprocess_image(torch.from_numpy(s).to(dev).permute(2, 0, 1).float().contiguous(), MEAN, STD, batch_b, n)

    def runner_front_end():
        for n, im in enumerate(u8):
            K.preprocess_image(K.image_u8hwc_to_chw(im, (Ho, Wo)), MEAN, STD, batch_c, n)

    for _ in range(warmup):
        fused(); through_pil(); runner_front_end()
    torch.cuda.synchronize()
    assert torch.equal(batch_a.view(torch.int32), batch_b.view(torch.int32)), f"{name}: fused and PIL batches differ"
    pil_ms.clear()
    t = {"a": [], "a_ev": [], "b": [], "c": [], "c_ev": []}
    for _ in range(reps):
        t["a"].append(wall(fused)); t["b"].append(wall(through_pil)); t["c"].append(wall(runner_front_end))
        t["a_ev"].append(events(fused)); t["c_ev"].append(events(runner_front_end))
    med = {k: statistics.median(v) for k, v in t.items()}
    mn = {k: min(v) for k, v in t.items()}
    pil_med = statistics.median(pil_ms)
    out_mb = count * Hp * Wp * 16 / 1e6
    print(f"{name}: {count} x ({H} x {W} -> {Ho} x {Wo}, slot {Hp} x {Wp}), {out_mb:.1f} MB of float4 written; median (min) of {reps} in ms")
    print(f"  (a) fused, {2 * count} launches:          wall {med['a']:8.3f} ({mn['a']:8.3f})  HIP events {med['a_ev']:8.3f} ({mn['a_ev']:8.3f})"
          f"  = {med['a_ev'] / count:.3f} per image, {out_mb / med['a_ev']:.0f} GB/s of output")
    print(f"  (b) PIL + H2D + cast + preprocess: wall {med['b']:8.3f} ({mn['b']:8.3f})  of it PIL.Image.resize {pil_med:8.3f} ({min(pil_ms):8.3f})"
          f"  = {pil_med / count:.3f} per image on one core")
    print(f"  (c) image_u8hwc_to_chw + preprocess: wall {med['c']:8.3f} ({mn['c']:8.3f})  HIP events {med['c_ev']:8.3f} ({mn['c_ev']:8.3f})   (other arithmetic)")
    print(f"  (b) / (a) = {med['b'] / med['a']:.1f}x wall; (a) is {100 * med['a'] / step_ms:.1f} % (wall) / {100 * med['a_ev'] / step_ms:.1f} % (events) "
          f"of one {step_ms} ms step; (a) and (b) bit-equal")
    return {"name": name, "count": count, "in": [H, W], "out": [Ho, Wo], "fused_wall_ms": round(med["a"], 3),
            "fused_events_ms": round(med["a_ev"], 3), "pil_path_wall_ms": round(med["b"], 3), "pil_resize_ms": round(pil_med, 3),
            "runner_front_end_wall_ms": round(med["c"], 3), "runner_front_end_events_ms": round(med["c_ev"], 3),
            "fused_share_of_step_pct": round(100 * med["a"] / step_ms, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=8)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--step-ms", type=float, default=25.3, help="one 8-image model step, for the share (a) takes of it")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the benchmark needs a HIP device"
    res = [measure("ic15", (720, 1280), a.images, a.reps, a.warmup, a.step_ms),
           measure("large", (2000, 3000), 1, a.reps, a.warmup, a.step_ms)]
    print(json.dumps({"metric": "resize_pil", "device": torch.cuda.get_device_name(0), "reps": a.reps, "results": res}))


if __name__ == "__main__":
    main()
