"""Beam-search text decoding on one device: ASTER_V2.beam_decode (glass_beam_search: the whole search behind one call, no host
synchronisation, x / xproj not inflated) against the unchanged host path ASTER_V2.beam_search (one glass_attention_decode_step
plus about ten torch ops per step, CPU copies and a Python back-tracking loop) on the same inputs, in the same process,
alternating; the greedy decode (ASTER_V2.forward, as routed by default) beside them.

The shipped decoder shape: T = 32 encoder steps, D = 256, 97 classes, 26 decoding steps; seeded random encoder outputs and the
synthetic decoder weights with a sharper output layer and a boosted <eos> row (as in oracle/make_golden.py --beam), so that
beams separate and end at different steps.  For every (RoIs, width):
  device / host / greedy - wall time of one call ending in a device synchronise, median and min of --reps after --warmup;
  peak extra memory      - torch.cuda.max_memory_allocated over one call minus what was allocated before it (inputs excluded);
  agreement              - RoIs whose best hypothesis (up to its length) differs between the two paths, largest |dscore|.

  python scripts/bench_beam_search.py [--reps 20] [--warmup 2] [--out profiles/beam_search.txt]
"""
import argparse
import json
import os
import statistics
import sys
import time
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "glass-text-spotting_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch

from glass_amd.modeling.recognition.recognizer_decoder import ASTER_V2
from glass_amd.structures.core import ShapeSpec
from glass_amd.utils.synth import make_state_dict

PRE = "roi_heads.recognizer_head.decoder."
C, L, T, D = 97, 26, 32, 256


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def peak_extra_mib(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    del out
    return (peak - base) / 2 ** 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_beam_search.py measures on a HIP device; none found")
    dev = torch.device("cuda:0")
    sd = dict(make_state_dict(1234, parts=("recog",)))
    q = PRE + "recognizer.decoder."
    sd[q + "fc.weight"] = sd[q + "fc.weight"] * 6.0
    sd[q + "fc.bias"] = sd[q + "fc.bias"].clone()
    sd[q + "fc.bias"][0] += 2.0
    rc = SimpleNamespace(CHARACTER_SET=[chr(0x100 + i) for i in range(C - 2)], MAX_WORD_LENGTH=L - 1)
    dec = ASTER_V2(SimpleNamespace(MODEL=SimpleNamespace(ROI_RECOGNIZER_HEAD=rc)), ShapeSpec(channels=D))
    dec.import_weights(sd, dev, PRE)
    lines = [f"beam search: T={T} D={D} classes={C} steps={L}, device {torch.cuda.get_device_name(0)}, "
             f"median (min) of {args.reps} alternating reps after {args.warmup} warm-up calls, times in ms"]
    records = []
    for R in (256, 1024):
        g = torch.Generator(device="cpu")
        g.manual_seed(R)
        x = torch.randn((R, T, D), generator=g).to(dev)
        greedy = lambda: dec(x)
        for k in (1, 5, 8):
            device = lambda: dec.beam_decode(x, k, 0, path_probs=True)
            host = lambda: dec.beam_search(x, k, 0)
            for _ in range(args.warmup):
                device(); host(); greedy()
            td, th, tg = [], [], []
            for _ in range(args.reps):
                ms, rd = timed(device); td.append(ms)
                ms, (hp, hs) = timed(host); th.append(ms)
                ms, _ = timed(greedy); tg.append(ms)
            n = rd.lengths[:, 0].cpu()
            hp, dp = hp.cpu(), rd.symbols[:, 0].cpu().long()
            differ = sum(1 for r in range(R) if not torch.equal(hp[r, :n[r]], dp[r, :n[r]]))
            ds = rd.scores[:, 0].cpu().double() - hs.cpu().double()
            dscore = float(ds[torch.isfinite(ds)].abs().max())
            md, mh = peak_extra_mib(device), peak_extra_mib(host)
            med = statistics.median
            rec = {"rois": R, "width": k, "device_ms": round(med(td), 3), "device_ms_min": round(min(td), 3),
                   "host_ms": round(med(th), 3), "host_ms_min": round(min(th), 3), "greedy_ms": round(med(tg), 3),
                   "device_peak_mib": round(md, 1), "host_peak_mib": round(mh, 1), "best_differs": differ,
                   "max_abs_dscore": dscore}
            records.append(rec)
            lines.append(f"  RoIs {R:5d} width {k}: device {med(td):8.3f} ({min(td):8.3f})  host {med(th):8.3f} ({min(th):8.3f})  "
                         f"host/device {med(th) / med(td):5.1f}x  greedy {med(tg):7.3f} ({min(tg):7.3f})  peak extra MiB device "
                         f"{md:7.1f} host {mh:7.1f}  best hypothesis differs for {differ} of {R} RoIs, max |dscore| {dscore:.2e}")
            print(lines[-1], flush=True)
    lines.append(json.dumps({"metric": "beam_search", "device": torch.cuda.get_device_name(0), "reps": args.reps, "results": records}))
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
