"""Forced decoding on one device: ASTER_V2.score (glass_forced_decode: the decoder with the emitted symbols given, one ABI call,
x / xproj not inflated, no host synchronisation) against the only other way to the same numbers - a forced replay driven
through the step kernel, one glass_attention_decode_step (3 launches) per step on x / xproj inflated to RoIs * n rows, plus
the log-softmax and the gather in torch - on the same inputs, in the same process, alternating.

The shipped decoder shape: T = 32 encoder steps, D = 256, 97 classes, 26 decoding steps; seeded random encoder outputs and the
synthetic decoder weights of scripts/bench_beam_search.py.  Targets are the n hypotheses (and lengths) of a beam search of
width n on the same inputs.  For every (RoIs, n):
  forced / +probs  - wall time of one ASTER_V2.score call (device targets) ending in a device synchronise, without / with
                     the full [RoIs, n, 26, 97] probability rows; median and min of --reps after --warmup;
  driven           - the kernel-driven replay (logits of every step, log-softmax, gather, running sum);
  peak extra memory - torch.cuda.max_memory_allocated over one call minus what was allocated before it (inputs excluded);
  agreement        - largest |dscore| between the two.
Then, at the bench configuration's RoI count (8 images x 32 RoIs = 256), what MODEL.ROI_RECOGNIZER_HEAD.BEAM_DISTRIBUTIONS
adds to a width-5 beam_decode: the call with distributions="best" minus the call without, per call and per decoding step.

  python scripts/bench_forced_decode.py [--reps 20] [--warmup 2] [--out profiles/forced_decode.txt]
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
from glass_amd.ops import native as K
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


def driven_replay(dec, x, targets, lengths):
    """scores [R,n] of the given sequences through glass_attention_decode_step on inflated inputs"""
    R, n, _ = targets.shape
    xproj = K.linear(x.view(R * T, D), dec.w["xW"], dec.w["xB"]).view(R, T, D)
    xi = x.unsqueeze(1).expand(R, n, T, D).reshape(R * n, T, D).contiguous()
    xpi = xproj.unsqueeze(1).expand(R, n, T, D).reshape(R * n, T, D).contiguous()
    state = torch.zeros((R * n, D), dtype=torch.float32, device=x.device)
    y_prev = torch.zeros((R * n,), dtype=torch.int32, device=x.device)
    tg = targets.reshape(R * n, L)
    ln = lengths.reshape(R * n)
    score = torch.zeros((R * n,), dtype=torch.float32, device=x.device)
    for t in range(L):
        logits, _, state = K.attention_decode_step(xi, xpi, dec.w, state, y_prev, C)
        lp = torch.log_softmax(logits, dim=1).gather(1, tg[:, t:t + 1].long()).squeeze(1)
        score = torch.where(ln > t, score + lp, score)
        y_prev = tg[:, t].contiguous()
    return score.view(R, n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_forced_decode.py measures on a HIP device; none found")
    dev = torch.device("cuda:0")
    sd = dict(make_state_dict(1234, parts=("recog",)))
    q = PRE + "recognizer.decoder."
    sd[q + "fc.weight"] = sd[q + "fc.weight"] * 6.0
    sd[q + "fc.bias"] = sd[q + "fc.bias"].clone()
    sd[q + "fc.bias"][0] += 2.0
    rc = SimpleNamespace(CHARACTER_SET=[chr(0x100 + i) for i in range(C - 2)], MAX_WORD_LENGTH=L - 1)
    dec = ASTER_V2(SimpleNamespace(MODEL=SimpleNamespace(ROI_RECOGNIZER_HEAD=rc)), ShapeSpec(channels=D))
    dec.import_weights(sd, dev, PRE)
    med = statistics.median
    lines = [f"forced decoding: T={T} D={D} classes={C} steps={L}, device {torch.cuda.get_device_name(0)}, "
             f"median (min) of {args.reps} alternating reps after {args.warmup} warm-up calls, times in ms"]
    records = []
    for R in (256, 1024):
        g = torch.Generator(device="cpu")
        g.manual_seed(R)
        x = torch.randn((R, T, D), generator=g).to(dev)
        for n in (1, 5, 8):
            hyp = dec.beam_decode(x, n, 0)
            tg, ln = hyp.symbols.contiguous(), hyp.lengths.contiguous()
            forced = lambda: dec.score(x, tg, ln)
            forced_p = lambda: dec.score(x, tg, ln, probs=True)
            driven = lambda: driven_replay(dec, x, tg, ln)
            for _ in range(args.warmup):
                forced(); forced_p(); driven()
            tf, tp, td = [], [], []
            for _ in range(args.reps):
                ms, rf = timed(forced); tf.append(ms)
                ms, _ = timed(forced_p); tp.append(ms)
                ms, rd = timed(driven); td.append(ms)
            dscore = float((rf.scores.double() - rd.double()).abs().max())
            dbeam = float((rf.scores.double() - hyp.scores.double()).abs().max())
            mf, mp, md = peak_extra_mib(forced), peak_extra_mib(forced_p), peak_extra_mib(driven)
            rec = {"rois": R, "n": n, "forced_ms": round(med(tf), 3), "forced_ms_min": round(min(tf), 3),
                   "forced_probs_ms": round(med(tp), 3), "forced_probs_ms_min": round(min(tp), 3), "driven_ms": round(med(td), 3),
                   "driven_ms_min": round(min(td), 3), "forced_peak_mib": round(mf, 1), "forced_probs_peak_mib": round(mp, 1),
                   "driven_peak_mib": round(md, 1), "max_abs_dscore_driven": dscore, "max_abs_dscore_beam": dbeam}
            records.append(rec)
            lines.append(f"  RoIs {R:5d} n {n}: forced {med(tf):8.3f} ({min(tf):8.3f})  +probs {med(tp):8.3f} ({min(tp):8.3f})  driven "
                         f"{med(td):8.3f} ({min(td):8.3f})  driven/forced {med(td) / med(tf):5.1f}x  peak extra MiB forced {mf:7.1f} "
                         f"+probs {mp:7.1f} driven {md:7.1f}  max |dscore| vs driven {dscore:.2e}, vs the search {dbeam:.2e}")
            print(lines[-1], flush=True)
    # ---- what BEAM_DISTRIBUTIONS adds to the recognizer head's decode at the bench configuration (8 x 32 RoIs, width 5)
    R, k = 256, 5
    g = torch.Generator(device="cpu")
    g.manual_seed(R)
    x = torch.randn((R, T, D), generator=g).to(dev)
    plain = lambda: dec.beam_decode(x, k, 0, path_probs=True)
    with_d = lambda: dec.beam_decode(x, k, 0, path_probs=True, distributions="best")
    for _ in range(args.warmup):
        plain(); with_d()
    ta, tb = [], []
    for _ in range(args.reps):
        ms, _ = timed(plain); ta.append(ms)
        ms, _ = timed(with_d); tb.append(ms)
    add = med(tb) - med(ta)
    lines.append(f"  BEAM_DISTRIBUTIONS at {R} RoIs, width {k}: beam_decode {med(ta):.3f} ({min(ta):.3f}) -> with distributions=\"best\" "
                 f"{med(tb):.3f} ({min(tb):.3f}): +{add:.3f} ms per call, +{add / L * 1e3:.1f} us per decoding step")
    print(lines[-1], flush=True)
    lines.append(json.dumps({"metric": "forced_decode", "device": torch.cuda.get_device_name(0), "reps": args.reps, "results": records,
                             "beam_distributions": {"rois": R, "width": k, "beam_ms": round(med(ta), 3), "with_best_ms": round(med(tb), 3),
                                                    "added_ms": round(add, 3), "added_us_per_step": round(add / L * 1e3, 1)}}))
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
