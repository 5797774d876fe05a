"""Character boxes on one device (include/glass_hip_feature_chars.h), same process, same build, alternating call by call:

  replay   - glass_forced_attention against glass_forced_decode at 256 and 1024 RoIs, n = 1, L = 26, C = 97, T = 32: wall time
             of one ops.native.forced_decode call (xproj given, device targets) ending in a device synchronise, with and
             without the attention rows; median and min of --reps after --warmup, the two alternating;
  spans    - ops.native.char_spans and ops.native.char_quads alone at 256 and 1024 words, the same way;
  head     - one RecognizerRCNNHeadV3.forward_nhwc call (synthetic weights, 256 RoIs of random fused features over 8 images)
             with MODEL.ROI_RECOGNIZER_HEAD.CHAR_BOXES on against off, greedy and at BEAM_WIDTH 5, two heads alternating;
  monotone - the share of words of that call whose centres do not strictly increase.  The synthetic weights attend almost
             uniformly, so this share says nothing about a trained model.

Not measured here: real checkpoints, the localisation accuracy of the quads, and the whole pipelined step.

  python scripts/bench_char_boxes.py [--reps 30] [--warmup 3] [--out profiles/char_boxes.txt]
"""
import argparse
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
Q = PRE + "recognizer.decoder."
C, L, T, D = 97, 26, 32, 256


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def alternate(fns, reps, warmup):
    """{name: fn} -> {name: [ms]}: the calls alternate, so drift of the machine hits them alike"""
    for _ in range(warmup):
        for fn in fns.values():
            timed(fn)
    ms = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            ms[k].append(timed(fn)[0])
    return ms


def stat(v):
    return f"median {statistics.median(v):7.3f} ms  min {min(v):7.3f} ms  (stdev {statistics.pstdev(v):.3f})"


def sharp_sd(stop=0):
    """the synthetic decoder weights of the tests: a sharper output layer, a boosted stop so that words end at different steps"""
    sd = dict(make_state_dict(1234, parts=("recog",)))
    sd[Q + "fc.weight"] = sd[Q + "fc.weight"] * 6.0
    sd[Q + "fc.bias"] = sd[Q + "fc.bias"].clone()
    sd[Q + "fc.bias"][stop] += 2.0
    return sd


def head(opts):
    from glass_amd.config import get_glass_cfg
    from glass_amd.modeling.recognition.recognizer_head_v2 import RecognizerRCNNHeadV3
    cfg = get_glass_cfg(os.path.join(ROOT, "configs", "glass_icdar15_mi355x.yaml"), ["MODEL.DEVICE", "cuda:0"] + list(opts))
    h = RecognizerRCNNHeadV3(cfg, ShapeSpec(channels=256))
    ch = h.text_encoder.character
    stop, seven = ch.index("[s]"), ch.index("7")
    sd = dict(make_state_dict(1234, parts=("recog",)))
    sd[Q + "fc.weight"] = sd[Q + "fc.weight"] * 6.0
    sd[Q + "fc.bias"] = sd[Q + "fc.bias"].clone()
    sd[Q + "fc.weight"][stop] = sd[Q + "fc.weight"][seven]
    sd[Q + "fc.bias"][stop] = sd[Q + "fc.bias"][seven] + 0.5
    h.import_weights(sd, torch.device("cuda:0"), "roi_heads.recognizer_head.")
    return h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_char_boxes.py needs a HIP device: a timing taken anywhere else says nothing")
    dev = torch.device("cuda:0")
    lines = [f"character boxes on {torch.cuda.get_device_name(0)}; reps {a.reps}, warmup {a.warmup}; library {K.lib()._name.split('/')[-1]}"]
    say = lambda s: (print(s, flush=True), lines.append(s))

    rc = SimpleNamespace(CHARACTER_SET=[chr(0x100 + i) for i in range(C - 2)], MAX_WORD_LENGTH=L - 1)
    dec = ASTER_V2(SimpleNamespace(MODEL=SimpleNamespace(ROI_RECOGNIZER_HEAD=rc)), ShapeSpec(channels=256))
    dec.import_weights(sharp_sd(), dev, PRE)
    g = torch.Generator(device="cpu")
    g.manual_seed(5)
    for R in (256, 1024):
        x = torch.randn((R, T, D), generator=g).to(dev)
        xproj = K.linear(x.view(R * T, D), dec.w["xW"], dec.w["xB"]).view(R, T, D)
        sym, _, ln = K.beam_search(x, xproj, dec.w, 1, C, L, 0)
        sym, ln = sym.contiguous(), ln.contiguous()
        plain = lambda: K.forced_decode(x, xproj, dec.w, sym, ln, C, L, 0)
        rows = lambda: K.forced_decode(x, xproj, dec.w, sym, ln, C, L, 0, attention=True)
        ms = alternate({"forced_decode": plain, "forced_attention": rows}, a.reps, a.warmup)
        out_p, out_r = plain(), rows()
        same = all(torch.equal(p, q) for p, q in zip(out_p[:3], out_r[:3]))
        say(f"replay, {R} RoIs (n 1, L {L}, C {C}, T {T}; lengths {int(ln.min())}..{int(ln.max())}; the rows are "
            f"{R * L * T * 4 / 1e6:.1f} MB); shared outputs equal: {same}")
        for k, v in ms.items():
            say(f"  {k:<17s} {stat(v)}")
        d = statistics.median(ms["forced_attention"]) - statistics.median(ms["forced_decode"])
        say(f"  difference of the medians {d:+.3f} ms ({100.0 * d / statistics.median(ms['forced_decode']):+.1f} %)")
        att, tg, n = out_r[5][:, 0].contiguous(), sym[:, 0].contiguous(), out_r[2][:, 0].contiguous()
        spans = K.char_spans(att, tg, n, 0)
        frames = torch.tensor([[400.0, 300.0, 120.0, 32.0, 10.0]], device=dev).repeat(R, 1).contiguous()
        ms = alternate({"char_spans": lambda: K.char_spans(att, tg, n, 0),
                        "char_quads": lambda: K.char_quads(spans["spans"], spans["count"], frames)}, a.reps, a.warmup)
        say(f"spans and quads alone, {R} words (one launch each, the call's allocations included)")
        for k, v in ms.items():
            say(f"  {k:<17s} {stat(v)}")

    R, N = 256, 8
    x = torch.randn((R, 8, 32, 256), generator=g).to(dev)
    roi_image = (torch.arange(R, dtype=torch.int32) * N // R).to(dev)
    for name, opts in (("greedy", []), ("BEAM_WIDTH 5", ["MODEL.ROI_RECOGNIZER_HEAD.BEAM_WIDTH", 5])):
        off, on = head(opts), head(opts + ["MODEL.ROI_RECOGNIZER_HEAD.CHAR_BOXES", True])
        ms = alternate({"key off": lambda: off.forward_nhwc(x, roi_image, N), "key on": lambda: on.forward_nhwc(x, roi_image, N)},
                       a.reps, a.warmup)
        say(f"recogniser head, {R} RoIs over {N} images, {name}")
        for k, v in ms.items():
            say(f"  {k:<17s} {stat(v)}")
        d = statistics.median(ms["key on"]) - statistics.median(ms["key off"])
        say(f"  difference of the medians {d:+.3f} ms ({100.0 * d / statistics.median(ms['key off']):+.1f} %)")
        packed = on.forward_nhwc(x, roi_image, N)[2]
        count, mono, valid = packed[:, -1, 0], packed[:, -1, 1], packed[:, -1, 2]
        words = int((count > 1).sum())
        say(f"  words with two or more characters {words} of {R}; of these non-monotone {int(((mono == 0) & (count > 1)).sum())}; "
            f"invalid {int((valid == 0).sum())} (synthetic weights attend almost uniformly: no statement about a trained model)")
    say("not measured: real checkpoints, localisation accuracy, the whole pipelined step")
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
