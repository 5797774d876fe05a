"""Image rotation on the device (glass_rotate_u8 / glass_rotate_boxes, csrc/image_rotate.hip) on one device against the only
other way to get the same bytes, PIL.Image.rotate on the host plus the upload.

Two images, 720 x 1280 and 2000 x 3000 (seeded synthetic uint8), each at 33.3 degrees (the affine bilinear form) and at 90
degrees (a transpose).  For each, in one process, alternating:
  (a) device: ops.native.rotate_u8 from the uint8 image already on the device, the allocation of the output included (one
              launch); HIP events around the call, and host wall time ended by a synchronise;
  (b) PIL:    PIL.Image.rotate(angle, BILINEAR, expand=True, fillcolor) on one host core, np.asarray of the result and its
              H2D copy; wall time ended by a synchronise, the PIL part of it also on its own.
(a) and (b) are compared byte for byte after warm-up.  Then ops.native.rotate_boxes on 1024 boxes, forward and inverse.
Warm-up first, then the median and minimum of --reps.  The lines are printed and written to --out.

  python scripts/bench_rotate.py [--reps 20] [--warmup 3] [--out profiles/rotate.txt]
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

from glass_amd.data import RotationTransform
from glass_amd.ops import native as K
from glass_amd.utils.synth import make_image

BILINEAR = getattr(Image, "Resampling", Image).BILINEAR
FILL = (7, 200, 255)


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


def measure(hw, angle, reps, warmup, say):
    dev = torch.device("cuda:0")
    H, W = hw
    host = make_image(H + W, H, W).numpy()
    u8 = torch.from_numpy(host).to(dev)
    pil = Image.fromarray(host)
    t = RotationTransform(H, W, angle)
    Ho, Wo = t.out_hw
    keep, pil_ms = {}, []

    def device():
        keep["a"] = K.rotate_u8(u8, t, FILL)

    def through_pil():
        t0 = time.perf_counter()
        r = np.asarray(pil.rotate(angle, resample=BILINEAR, expand=True, fillcolor=FILL))
        pil_ms.append((time.perf_counter() - t0) * 1e3)
        keep["b"] = torch.from_numpy(r).to(dev)

    for _ in range(warmup):
        device(); through_pil()
    torch.cuda.synchronize()
    assert torch.equal(keep["a"], keep["b"]), f"{hw} at {angle}: the device and PIL differ"
    pil_ms.clear()
    ms = {"a": [], "a_ev": [], "b": []}
    for _ in range(reps):
        ms["a_ev"].append(events(device)); ms["b"].append(wall(through_pil)); ms["a"].append(wall(device))
    med = {k: statistics.median(v) for k, v in ms.items()}
    mn = {k: min(v) for k, v in ms.items()}
    pil_med = statistics.median(pil_ms)
    moved = (H * W + Ho * Wo) * 3 / 1e6
    say(f"{H} x {W} at {angle} degrees (kind {t.kind}) -> {Ho} x {Wo}, {moved:.1f} MB read + written; median (min) of {reps} in ms")
    say(f"  (a) rotate_u8, 1 launch + the output's allocation: HIP events {med['a_ev']:8.3f} ({mn['a_ev']:8.3f})  wall {med['a']:8.3f} "
        f"({mn['a']:8.3f})  = {moved / med['a_ev']:.0f} GB/s by events")
    say(f"  (b) PIL.Image.rotate + np.asarray + H2D:            wall {med['b']:8.3f} ({mn['b']:8.3f})  of it PIL on one core {pil_med:8.3f} "
        f"({min(pil_ms):8.3f})")
    say(f"  (b) / (a) = {med['b'] / med['a']:.1f}x wall; (a) and (b) byte-equal")
    return {"in": [H, W], "angle": angle, "kind": t.kind, "out": [Ho, Wo], "device_events_ms": round(med["a_ev"], 4),
            "device_wall_ms": round(med["a"], 4), "pil_path_wall_ms": round(med["b"], 3), "pil_rotate_ms": round(pil_med, 3)}


def measure_boxes(n, reps, warmup, say):
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(n)
    b = np.stack([rng.uniform(0, 1280, n), rng.uniform(0, 720, n), rng.uniform(1, 300, n), rng.uniform(1, 80, n), rng.uniform(-180, 180, n)], 1)
    boxes = torch.from_numpy(b.astype(np.float32)).to(dev)
    t = RotationTransform(720, 1280, 33.3)
    out = {}
    for name, inverse in (("forward", False), ("inverse", True)):
        call = lambda: K.rotate_boxes(boxes, t, inverse=inverse)       # noqa: E731
        for _ in range(warmup):
            call()
        ev, wl = [], []
        for _ in range(reps):
            ev.append(events(call)); wl.append(wall(call))
        say(f"rotate_boxes, {n} boxes, {name}: HIP events {statistics.median(ev):.4f} ({min(ev):.4f}) ms, wall {statistics.median(wl):.4f} "
            f"({min(wl):.4f}) ms; 1 launch + the output's allocation")
        out[name] = {"events_ms": round(statistics.median(ev), 4), "wall_ms": round(statistics.median(wl), 4)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rotate.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the benchmark needs a HIP device"
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    res = [measure(hw, angle, a.reps, a.warmup, say) for hw in ((720, 1280), (2000, 3000)) for angle in (33.3, 90)]
    boxes = measure_boxes(1024, a.reps, a.warmup, say)
    say(json.dumps({"metric": "rotate", "device": torch.cuda.get_device_name(0), "reps": a.reps, "results": res, "boxes_1024": boxes}))
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
