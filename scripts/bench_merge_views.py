"""Cross-view merge of tiled inference on one device: glass_merge_views alone, and what it adds to a tiled step.

Kernel alone (seeded synthetic detections; words drawn over the whole image, a jittered copy of each in every tile that holds
it whole - up to K per tile by score - and, for the plan with a full view, in the whole image at 1600 / long side):
  41 x 100    a 5 x 8 plan of 1024-pixel tiles (overlap 256, border 16) over 4096 x 6400, plus the full view;
  8 x 1024    a 2 x 4 plan over 1792 x 3328, 1024 small words per tile (the 8192-slot limit), no full view.
For each: candidates after the border / size filters, cross-view duplicates among them (candidates - kept before the cap), and
  kernel   device-event time of --inner back-to-back glass_merge_views launches on preallocated outputs, per launch;
  call     wall time of one ops.native.merge_views call ending in a device synchronise (output fill and workspace included);
  host     the float64 restatement of tests/view_merge_cases.py on the same inputs, once, for scale (not a competitor).
Median and min of --reps after --warmup.  The kernel's outputs are checked against the float64 restatement first.

Tiled step (synthetic weights, one seeded 1536 x 2048 image, INPUT.MIN_SIZE_TEST 1024 so that a 1024-pixel crop is not resized):
  run_tiled    GlassRunner.run_tiled(image): 6 tiles + the full view, merge, one post-processing of the merged set;
  run_batch    GlassRunner.run_batch(the 6 crops + the image): the same model inputs, no merge, seven post-processed sets.
alternating, wall time ending in a device synchronise.

  python scripts/bench_merge_views.py [--reps 20] [--warmup 3] [--out profiles/merge_views.txt]
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

import numpy as np
import torch

import view_merge_cases as C
from glass_amd import _lib
from glass_amd.config import get_glass_cfg
from glass_amd.inference.glass_runner import GlassRunner
from glass_amd.inference.tiling import plan_tiles
from glass_amd.ops import native as K
from glass_amd.utils.synth import make_image, make_state_dict

INF = float("inf")


def synthetic_views(seed, H, W, tile, overlap, border, Kdet, n_words, wr, hr, full_view):
    """-> case dict as tests/view_merge_cases.py builds them (without its margins: nothing is compared bit for bit here
    unless the float64 restatement agrees, which is checked)"""
    g = np.random.default_rng(seed)
    plan = plan_tiles(H, W, tile, overlap, border)
    L = float(plan.max_whole)
    V = len(plan.tiles) + int(full_view)
    rho = 1600.0 / max(H, W)
    xform = [[t.x0, t.y0, 1.0] for t in plan.tiles] + ([[0.0, 0.0, 1.0 / rho]] if full_view else [])
    keep = [list(t.keep) for t in plan.tiles] + ([[-INF, -INF, INF, INF]] if full_view else [])
    band = [[-INF, L if full_view else INF] for _ in plan.tiles] + ([[L, INF]] if full_view else [])
    words = np.stack([g.uniform(0, W, n_words), g.uniform(0, H, n_words), g.uniform(*wr, n_words), g.uniform(*hr, n_words),
                      g.uniform(-30, 30, n_words)], 1)
    score = g.permutation(np.linspace(0.05, 0.99, n_words))
    rows = [[] for _ in range(V)]
    for w, s in zip(words, score):
        x0, y0, x1, y1 = C.extents(w)
        for v, t in enumerate(plan.tiles):
            if t.x0 <= x0 and x1 <= t.x0 + t.w and t.y0 <= y0 and y1 <= t.y0 + t.h:
                rows[v].append((s + g.uniform(-0.02, 0.02), C._jitter(g, w)))
        if full_view:
            rows[-1].append((s + g.uniform(-0.02, 0.02), C._jitter(g, w)))
    boxes, scores = np.zeros((V, Kdet, 5), dtype=np.float32), np.zeros((V, Kdet), dtype=np.float32)
    counts = np.zeros((V,), dtype=np.int32)
    for v, r in enumerate(rows):
        r.sort(key=lambda x: -x[0])
        r = r[:Kdet]
        counts[v] = len(r)
        ox, oy, inv = xform[v]
        for s, (sc, b) in enumerate(r):
            boxes[v, s] = [(b[0] - ox) / inv, (b[1] - oy) / inv, b[2] / inv, b[3] / inv, b[4]]
            scores[v, s] = sc
    f = lambda a: np.asarray(a, dtype=np.float32)
    return dict(boxes=boxes, scores=scores, counts=counts, xform=f(xform), keep=f(keep), band=f(band), V=V, K=Kdet)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def med_min(v):
    return statistics.median(v), min(v)


def bench_kernel(name, case, thr, args, lines, results):
    dev = torch.device("cuda:0")
    t = {k: torch.from_numpy(case[k]).to(dev) for k in ("boxes", "scores", "counts", "xform", "keep", "band")}
    V, Kd = case["V"], case["K"]
    call = lambda: K.merge_views(t["boxes"], t["scores"], t["counts"], t["xform"], t["keep"], t["band"], thr, 1024)
    out = {k: v.cpu().numpy() for k, v in call().items()}
    h0 = time.perf_counter()
    ref = C.merge_ref(case["boxes"], case["scores"], case["counts"], case["xform"], case["keep"], case["band"], thr, 1024)
    host_ms = (time.perf_counter() - h0) * 1e3
    uncapped = C.merge_ref(case["boxes"], case["scores"], case["counts"], case["xform"], case["keep"], case["band"], thr, 1 << 30)
    n = ref["count"]
    same = (out["count"].tolist() == [n, ref["flag"]] and np.array_equal(out["src"][:n], ref["src"])
            and np.array_equal(out["boxes"][:n].view(np.uint32), ref["boxes"].view(np.uint32)))
    # the kernel alone: the C entry point on preallocated outputs
    L = _lib.lib()
    nb = int(L.glass_merge_views_workspace_bytes(V, Kd))
    ws = torch.empty((nb,), dtype=torch.uint8, device=dev)
    ob, os_ = torch.zeros((1024, 5), device=dev), torch.zeros((1024,), device=dev)
    src, cnt = torch.zeros((1024,), dtype=torch.int32, device=dev), torch.zeros((2,), dtype=torch.int32, device=dev)
    ptrs = [t[k].data_ptr() for k in ("boxes", "scores", "counts", "xform", "keep", "band")]

    def launches():
        for _ in range(args.inner):
            _lib.check(L.glass_merge_views(*ptrs, V, Kd, thr, 1024, ob.data_ptr(), os_.data_ptr(), src.data_ptr(), cnt.data_ptr(),
                                           ws.data_ptr(), nb, K.stream_handle()))
    kern, wall = [], []
    for rep in range(args.warmup + args.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        launches()
        e1.record()
        torch.cuda.synchronize()
        ms, _ = timed(call)
        if rep >= args.warmup:
            kern.append(e0.elapsed_time(e1) / args.inner)
            wall.append(ms)
    (km, kmin), (wm, wmin) = med_min(kern), med_min(wall)
    cands, dups = uncapped["candidates"], uncapped["candidates"] - uncapped["count"]
    lines.append(f" {name}: {int(case['counts'].sum())} detections in {V} views of {Kd} slots, {cands} candidates after the filters, "
                 f"{dups} cross-view duplicates ({100.0 * dups / max(cands, 1):.0f} %), {n} out, flag {ref['flag']}; equals the float64 "
                 f"restatement: {same}")
    lines.append(f"   kernel {km:8.3f} ({kmin:8.3f}) ms   call {wm:8.3f} ({wmin:8.3f}) ms   host float64 restatement {host_ms:9.1f} ms (once)")
    results.append(dict(case=name, views=V, slots=Kd, detections=int(case["counts"].sum()), candidates=cands, duplicates=dups, out=n,
                        flag=ref["flag"], same_as_reference=bool(same), kernel_ms=round(km, 4), kernel_ms_min=round(kmin, 4),
                        call_ms=round(wm, 4), call_ms_min=round(wmin, 4), host_ref_ms=round(host_ms, 1)))
    return same


def bench_runner(args, lines, results):
    cfg = get_glass_cfg(os.path.join(ROOT, "configs", "glass_icdar15_mi355x.yaml"),
                        ["MODEL.DEVICE", "cuda:0", "INPUT.MIN_SIZE_TEST", 1024, "POST_PROCESSING.TEXT_THRESHOLD", 0.0])
    runner = GlassRunner(None, None, cfg=cfg, state_dict=make_state_dict(1234), post_process=True)
    H, W = 1536, 2048
    img = make_image(7, H, W).numpy()
    plan = plan_tiles(H, W, 1024, 256, 16)
    crops = [np.ascontiguousarray(img[t.y0:t.y0 + t.h, t.x0:t.x0 + t.w]) for t in plan.tiles]
    tiled = lambda: runner.run_tiled(img)
    batch = lambda: runner.run_batch(crops + [img])
    a, b = [], []
    reps = max(args.reps // 4, 3)
    for rep in range(2 + reps):
        ta, ra = timed(tiled)
        tb, rb = timed(batch)
        if rep >= 2:
            a.append(ta)
            b.append(tb)
    (am, amin), (bm, bmin) = med_min(a), med_min(b)
    lines.append(f" tiled step, {H} x {W}, {len(plan.tiles)} tiles of 1024 + the full view, {reps} alternating reps after 2 warm-up: "
                 f"run_tiled {am:8.2f} ({amin:8.2f}) ms, {len(ra)} words   run_batch over the same 7 inputs {bm:8.2f} ({bmin:8.2f}) ms, "
                 f"{sum(len(r) for r in rb)} words in 7 sets   run_tiled / run_batch {am / bm:.3f}x")
    results.append(dict(case="tiled_step", height=H, width=W, tiles=len(plan.tiles), run_tiled_ms=round(am, 2),
                        run_tiled_ms_min=round(amin, 2), run_batch_ms=round(bm, 2), run_batch_ms_min=round(bmin, 2),
                        words_tiled=len(ra), words_batch=sum(len(r) for r in rb)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "merge_views.txt"))
    ap.add_argument("--skip-runner", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_merge_views.py needs an MI355X: a timing taken without one says nothing")
    thr = 0.35                     # MODEL.ROI_HEADS.NMS_THRESH_TEST of the shipped config
    lines = [f"cross-view merge (glass_merge_views), library {_lib.source_sha16()}, device {torch.cuda.get_device_name(0)}, median (min) of "
             f"{args.reps} reps after {args.warmup} warm-up, nms_thresh {thr}, max_out 1024, times in ms; kernel = device events around "
             f"{args.inner} back-to-back launches, per launch"]
    results = []
    ok = bench_kernel("41 x 100", synthetic_views(1, 4096, 6400, 1024, 256, 16, 100, 2200, (30.0, 120.0), (12.0, 30.0), True), thr,
                      args, lines, results)
    ok &= bench_kernel("8 x 1024", synthetic_views(2, 1792, 3328, 1024, 256, 16, 1024, 6400, (14.0, 28.0), (6.0, 10.0), False), thr,
                       args, lines, results)
    if not args.skip_runner:
        bench_runner(args, lines, results)
    lines.append("not measured: per-kernel counters, real images (the synthetic weights give arbitrary detections, so the word counts say "
                 "nothing about accuracy), plans of more than 7 views end to end, a merge that walks all 8192 candidates without reaching the 1024 outputs (both "
                 "kernel inputs fill them, so the walk ends there), the merge beside a concurrent fp16-mode step")
    lines.append(json.dumps({"metric": "merge_views", "device": torch.cuda.get_device_name(0), "reps": args.reps, "results": results}))
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text + "\n")
    if not ok:                     # (these inputs are drawn without the tests' decision margins: a pair within float32 rounding of
        print("note: a kernel output differs from the float64 restatement on a benchmark input", file=sys.stderr)      # the threshold can differ)


if __name__ == "__main__":
    main()
