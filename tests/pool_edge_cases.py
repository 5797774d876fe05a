"""Inputs of tests/test_gpu_pool_edges.py that the CPU suite also looks at (tests/test_oracle_d2ops.py measures the oracle's
fp32 RoIAlign against the float64 helper on exactly these boxes and checks the level-assignment list).  Test helper."""
import numpy as np

ROI_H, ROI_W, ROI_C = 24, 40, 8


def roi_features():
    """[ROI_C, 24, 40] float64, every value exactly representable in fp16 (the same numbers feed the fp32 and the fp16 levels):
    a gentle ramp plus a random part of amplitude 0.25"""
    g = np.random.default_rng(5)
    y, x = np.meshgrid(np.arange(ROI_H), np.arange(ROI_W), indexing="ij")
    c = np.arange(ROI_C)[:, None, None]
    f = 0.02 * (x - 0.5 * y)[None] * (c + 1) / ROI_C + 0.25 * g.uniform(-1, 1, (ROI_C, ROI_H, ROI_W))
    return f.astype(np.float16).astype(np.float64)


# ---------------------------------------------------------------------------------------------- samples on the boundary
# angle 0, scale 1, dyadic coordinates: every sample coordinate is exact in fp32, so a sample sits exactly where it is put.
# A box of h = 2 PH g (w = 2 PW g) has its sample rows (columns) 2 apart, the first one at -h/2 + 1 from the centre.
BOUNDARY_CONFIGS = ((1, (2, 2)), (2, (2, 2)), (1, (3, 5)), (2, (3, 5)))      # (sampling_ratio, (PH, PW))


def boundary_targets(n):
    """coordinates for the first (low) and the last (high) sample row of a box on an axis of n cells: on -1, -0.5, 0, n-1,
    n-0.5, n, n+0.5 and 1/16 outside the two inclusive limits; `skipped` says what the sampling rule does with each"""
    low = [(-1.5, True), (-1.0625, True), (-1.0, False), (-0.5, False), (0.0, False)]
    high = [(n - 1.0, False), (n - 0.5, False), (float(n), False), (n + 0.0625, True), (n + 0.5, True)]
    return low, high


def boundary_boxes(sr, out_hw):
    """[(name, box, (target_y or None, target_x or None))] for one configuration"""
    PH, PW = out_hw
    h, w = 2.0 * PH * sr, 2.0 * PW * sr
    ylow, yhigh = boundary_targets(ROI_H)
    xlow, xhigh = boundary_targets(ROI_W)
    cy_of = {"lo": lambda t: t + h / 2 - 1 + 0.5, "hi": lambda t: t - h / 2 + 1 + 0.5}
    cx_of = {"lo": lambda t: t + w / 2 - 1 + 0.5, "hi": lambda t: t - w / 2 + 1 + 0.5}
    out = []
    for side, ts in (("lo", ylow), ("hi", yhigh)):
        for t, _ in ts:
            out.append((f"y{side}={t}", (20.0, cy_of[side](t), w, h, 0.0), (t, None)))
    for side, ts in (("lo", xlow), ("hi", xhigh)):
        for t, _ in ts:
            out.append((f"x{side}={t}", (cx_of[side](t), 12.0, w, h, 0.0), (None, t)))
    for (sy, ys), (sx, xs) in ((("lo", ylow), ("lo", xlow)), (("hi", yhigh), ("hi", xhigh)), (("hi", yhigh), ("lo", xlow))):
        for (ty, _), (tx, _) in zip(ys, xs):
            out.append((f"y{sy}={ty},x{sx}={tx}", (cx_of[sx](tx), cy_of[sy](ty), w, h, 0.0), (ty, tx)))
    return out


# sampling_ratio 0: ceil(roi / bins) samples per bin - none for an empty box, one row for h smaller than a bin
DEGENERATE_BOXES = ((20.0, 12.0, 0.0, 6.0, 0.0), (20.0, 12.0, 10.0, 0.0, 0.0), (20.0, 12.0, 0.0, 0.0, 0.0),
                    (20.0, 12.0, 10.0, 0.75, 0.0), (20.0, 12.0, 0.0, 6.0, 30.0), (20.0, 12.0, 0.5, 0.25, -45.0),
                    (20.0, 12.0, 10.0, 6.0, 0.0))
DEGENERATE_EMPTY = (True, True, True, False, True, False, False)            # sample count 0 -> all-zero output
DEGENERATE_OUT = ((2, 2), (3, 5))

# rotated boxes hanging over each of the four corners of the map (and one that covers a corner from far outside)
CORNER_BOXES = ((2.0, 1.5, 14.0, 9.0, 30.0), (39.0, 2.0, 16.0, 8.0, -45.0), (1.0, 23.0, 12.0, 10.0, 120.0),
                (38.5, 22.0, 15.0, 7.0, 77.0), (0.0, 0.0, 20.0, 12.0, -160.0), (41.0, 25.0, 9.0, 30.0, 10.0))
CORNER_OUT, CORNER_SR = (3, 5), 2


def all_roi_cases():
    """every RoIAlign known-answer case of the GPU test: (name, boxes [R,5] float64, out_hw, sampling_ratio)"""
    cases = [(f"boundary sr={sr} out={o}", np.array([b for _, b, _ in boundary_boxes(sr, o)]), o, sr) for sr, o in BOUNDARY_CONFIGS]
    cases += [(f"degenerate out={o}", np.array(DEGENERATE_BOXES), o, 0) for o in DEGENERATE_OUT]
    cases.append(("corners", np.array(CORNER_BOXES), CORNER_OUT, CORNER_SR))
    return cases


# ---------------------------------------------------------------------------------------------- level assignment
LEVEL_MIN, LEVEL_NUM = 2, 5
LEVEL_BOUNDARIES = (112.0, 224.0, 448.0, 896.0)        # sqrt(w h) at which the level index steps 0|1, 1|2, 2|3, 3|4


def _level_from_log2(lg):
    lvl = np.floor(np.float32(4.0) + np.float32(lg))
    return int(min(max(lvl, LEVEL_MIN), LEVEL_MIN + LEVEL_NUM - 1)) - LEVEL_MIN


def level_log2(w, h):
    """the fp32 formula of d2 assign_boxes_to_levels up to its log2: log2(sqrt(w h) / 224 + 1e-8), all in float32"""
    w, h = np.float32(w), np.float32(h)
    with np.errstate(divide="ignore"):
        return np.log2(np.sqrt(w * h) / np.float32(224.0) + np.float32(1e-8))


def expected_level(w, h):
    return _level_from_log2(level_log2(w, h))


def level_is_robust(w, h):
    """the level does not change when the log2 result moves by up to 2 ulp either way"""
    lg = level_log2(w, h)
    want = _level_from_log2(lg)
    lo = hi = lg
    for _ in range(2):
        lo, hi = np.nextafter(lo, np.float32(-np.inf)), np.nextafter(hi, np.float32(np.inf))
        if _level_from_log2(lo) != want or _level_from_log2(hi) != want:
            return False
    return True


def _ulps(v, k):
    v = np.float32(v)
    for _ in range(abs(k)):
        v = np.nextafter(v, np.float32(np.inf if k > 0 else -np.inf))
    return float(v)


def level_cases():
    """[(family, w, h, expected level)]: only boxes whose level survives a +-2 ulp error of log2 (level_is_robust).
    Families: `exact` sqrt(w h) = 56 ... 896 as squares and 4:1 boxes; `ulp` the same boxes with w moved 1 and 2 fp32 ulps
    down and up - where none of them is a surviving case on its own side of a boundary (fp32 rounds sqrt(w h) / 224 + 1e-8
    back onto the boundary for the nearest few), the next ulp counts (3, 4, ...) are tried until one is, so that both sides
    of every boundary stay covered; `rel` sqrt(w h) a relative 1e-3 off; `clamp` far outside."""
    bases = []
    for s in (56.0, 112.0, 224.0, 448.0, 896.0):
        bases += [(s, s), (2.0 * s, s / 2.0)]
    out = []

    def add(fam, w, h):
        if level_is_robust(w, h):
            out.append((fam, float(w), float(h), expected_level(w, h)))
            return True
        return False

    for w, h in bases:
        add("exact", w, h)
        s = float(np.sqrt(w * h))
        for sign in (-1, 1):
            for k in (1, 2):
                add("ulp", _ulps(w, sign * k), h)
            if s in LEVEL_BOUNDARIES:                      # the side of the boundary this direction is meant to reach
                side = LEVEL_BOUNDARIES.index(s) + (1 if sign > 0 else 0)
                k = 3
                while not any(f == "ulp" and hh == h and lv == side and abs(ww / w - 1.0) < 1e-3 for f, ww, hh, lv in out):
                    assert k <= 4096, (w, h, sign)
                    add("ulp", _ulps(w, sign * k), h)
                    k += 1
        for r in (1.0 - 2e-3, 1.0 + 2e-3):
            add("rel", float(np.float32(w * r)), h)
    for w, h in ((0.0, 0.0), (1.0, 1.0), (10.0, 5.0), (30.0, 100.0), (4000.0, 4000.0), (1e5, 1e4), (3e4, 50.0)):
        add("clamp", w, h)
    return out
