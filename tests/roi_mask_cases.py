"""Seeded cases for mask polygons straight from the RoI masks (ops.native.roi_mask_rings, MaskPolygonizer.from_rois): boxes
that leave the image on every side, every angle the paste treats specially, extents from below one pixel to wider than the
image, degenerate and non-finite boxes; masks with one region, two regions, holes and pinches; M = 28, 7 and 4."""
import numpy as np

from mask_ring_cases import word_masks

NAN, INF = float("nan"), float("inf")
ANGLES = (0.0, 90.0, -90.0, 180.0, 45.0, -135.0, 750.0)


def boxes_for(H, W, seed=31):
    """float32 [R, 5] (cx, cy, w, h, angle in degrees) for an H x W image; the lengths are fractions of the image so the same
    list serves 211 x 317 and 37 x 53"""
    rng = np.random.RandomState(seed)
    u, v = W / 317.0, H / 211.0
    b = []
    # fully outside, beyond each side and a corner
    b += [(-60 * u, 50 * v, 40 * u, 20 * v, 0), (W + 83 * u, 100 * v, 50 * u, 20 * v, 30), (100 * u, -50 * v, 30 * u, 20 * v, 0),
          (100 * u, H + 89 * v, 60 * u, 20 * v, 45), (-40 * u, -40 * v, 30 * u, 30 * v, 45)]
    # cut by the left, right, top and bottom edge, and by two corners
    b += [(5 * u, 100 * v, 60 * u, 30 * v, 0), (W - 5 * u, 100 * v, 60 * u, 30 * v, 10), (150 * u, 3 * v, 80 * u, 24 * v, 0),
          (150 * u, H - 3 * v, 80 * u, 24 * v, -5), (4 * u, 4 * v, 50 * u, 30 * v, 45), (W - 3 * u, H - 2 * v, 70 * u, 30 * v, -135)]
    # every angle, exact and jittered, inside the image
    for a in ANGLES:
        b.append((158 * u, 105 * v, 90 * u, 30 * v, a))
        b.append((rng.uniform(80, 240) * u, rng.uniform(60, 150) * v, rng.uniform(30, 120) * u, rng.uniform(8, 40) * v,
                  a + rng.uniform(-3, 3)))
    # extents: no pixel centre inside (empty ring), around one pixel, a sliver, wider than the image
    b += [(100.5 * u, 70.5 * v, 0.3, 0.3, 0), (100.2, 70.2, 0.3, 0.3, 45), (120 * u, 80 * v, 0.3, 40 * v, 20), (60.5, 30.5, 1, 1, 0),
          (61.0, 20.0, 2.5, 1.2, 30), (W / 2, H / 2, 1.3 * W, 1.4 * H, 0), (W / 2, H / 2, 1.2 * W, 0.3 * H, 45),
          (W / 2, H / 2, 180 * u, 12 * v, -135), (W / 2 + 30 * u, H / 2 - 30 * v, 180 * u, 100 * v, 750)]
    # degenerate and non-finite
    ok = (150 * u, 100 * v, 60 * u, 24 * v, 15)
    b += [(150 * u, 100 * v, 0, 24 * v, 15), (150 * u, 100 * v, 60 * u, 0, 15), (150 * u, 100 * v, -60 * u, 24 * v, 15),
          (150 * u, 100 * v, 60 * u, -24 * v, 100)]
    for k in range(5):
        for bad in (NAN, INF, -INF):
            q = list(ok)
            q[k] = bad
            b.append(tuple(q))
    # seeded: centres up to 30 px outside, mixed sizes and angles
    for _ in range(24):
        b.append((rng.uniform(-30, W + 30), rng.uniform(-30, H + 30), rng.uniform(2, 180) * u, rng.uniform(2, 60) * v,
                  float(rng.choice(ANGLES)) + (rng.uniform(-20, 20) if rng.rand() < 0.5 else 0.0)))
    return np.asarray(b, dtype=np.float32)


def shaped_masks(M):
    """[(name, float32 [M, M])]: probabilities near 0 / 1 with the regions the tracer's rules are about"""
    lo, hi = 0.02, 0.98
    out = [("all ones", np.full((M, M), 1.0)), ("all zeros", np.zeros((M, M)))]
    q = max(M // 7, 1)
    two = np.full((M, M), lo); two[q:2 * q, q:3 * q] = hi; two[4 * q:7 * q, q:6 * q] = hi          # the larger blob comes second
    out.append(("two blobs, larger second", two))
    eq = np.full((M, M), lo); eq[q:3 * q, q:3 * q] = hi; eq[q:3 * q, 4 * q:6 * q] = hi           # equal: the first raster pixel wins
    out.append(("two equal blobs", eq))
    ring = np.full((M, M), hi); ring[(M // 2 - q):(M // 2 + q + (M % 2)), (M // 2 - q):(M // 2 + q + (M % 2))] = lo
    out.append(("ring with a hole", ring))
    yy, xx = np.mgrid[0:M, 0:M]
    out.append(("checkerboard", np.where((yy + xx) % 2 == 0, hi, lo)))
    return [(n, m.astype(np.float32)) for n, m in out]


def masks_for(R, M, seed=7):
    """float32 [R, M, M]: word-like masks and the shaped ones, interleaved; every second one of the first 40 is all ones"""
    words = word_masks(R, M, seed)
    shaped = shaped_masks(M)
    out = words.copy()
    for r in range(R):
        if r % 3 == 1:
            out[r] = shaped[(r // 3) % len(shaped)][1]
        elif r < 40 and r % 2 == 0:
            out[r] = 1.0
    return out


def cases():
    """[dict(name, hw, M, threshold, masks [R, M, M], boxes [R, 5])]"""
    out = []
    for hw, M, t in (((211, 317), 28, 0.5), ((211, 317), 7, 0.3), ((211, 317), 4, 0.9), ((37, 53), 28, 0.5), ((37, 53), 7, 0.9),
                     ((37, 53), 4, 0.3)):
        boxes = boxes_for(*hw)
        out.append(dict(name=f"{hw[0]} x {hw[1]}, M = {M}, t = {t}", hw=hw, M=M, threshold=t, masks=masks_for(len(boxes), M), boxes=boxes))
    # 640 x 704: a window of 640 rows x 11 words > MASK_RINGS_LDS_WORDS (the global-memory walk), with windows that cross the
    # 64-column label seam beside it
    big = np.asarray([(352, 320, 690, 600, 0), (352, 320, 690, 600, 0), (352, 320, 690, 600, 0), (200, 300, 150, 40, 12),
                      (352, 320, 690, 600, 180)], dtype=np.float32)
    shaped = dict(shaped_masks(28))
    mk = np.stack([np.ones((28, 28), np.float32), word_masks(1, 28, 3)[0], shaped["checkerboard"], word_masks(1, 28, 4)[0],
                   shaped["ring with a hole"]])
    out.append(dict(name="640 x 704, window beyond the LDS bitmap", hw=(640, 704), M=28, threshold=0.5, masks=mk, boxes=big))
    return out


def outside(pasted, rects):
    """number of set pixels of pasted bool [R, H, W] outside rects int [R, 4] (x0, y0, x1, y1 inclusive; x1 < x0 = empty)"""
    pasted = np.asarray(pasted).astype(bool)
    n = 0
    for m, (x0, y0, x1, y1) in zip(pasted, np.asarray(rects).tolist()):
        inside = np.zeros_like(m)
        if x1 >= x0 and y1 >= y0:
            inside[y0:y1 + 1, x0:x1 + 1] = True
        n += int((m & ~inside).sum())
    return n


def memory_case(R=64, H=4096, W=4096, M=28, seed=5):
    """64 boxes of at most 200 x 40 px at mixed angles on a 4096 x 4096 image (1 GiB pasted)"""
    rng = np.random.RandomState(seed)
    boxes = np.stack([rng.uniform(100, W - 100, R), rng.uniform(100, H - 100, R), rng.uniform(40, 200, R), rng.uniform(10, 40, R),
                      rng.choice(ANGLES, R) + rng.uniform(-10, 10, R)], 1).astype(np.float32)
    return word_masks(R, M, seed), boxes, (H, W)
