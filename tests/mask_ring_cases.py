"""Cases and an independent checker for the mask polygoniser (glass_amd.evaluation.masks_to_polygons on the host,
MaskPolygonizer / csrc/mask_rings.hip on the device).

`check_ring` never walks a boundary: it refills the ring by even-odd parity over its vertical edges and requires the
filled pixels to equal the largest 4-connected region with its holes filled (scipy.ndimage.label with the 4-structure,
first maximum = first region in raster order; binary_fill_holes with the 3 x 3 structure), and the ring to be closed, to
start at the top-left corner of the region's first raster pixel, to be clockwise in image coordinates (positive sum of
x_i * y_{i+1} - x_{i+1} * y_i) and to turn at every vertex."""
import numpy as np
from scipy import ndimage

FOUR = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]])


def expected_region(mask):
    """(largest 4-connected region with its holes filled, (row, column) of its first raster pixel); (None, None) if empty"""
    m = np.asarray(mask).astype(bool)
    lab, n = ndimage.label(m, structure=FOUR)
    if n == 0:
        return None, None
    k = int(np.argmax(np.bincount(lab.ravel())[1:])) + 1
    reg = lab == k
    r0 = int(np.nonzero(reg.any(axis=1))[0][0])
    c0 = int(np.nonzero(reg[r0])[0][0])
    return ndimage.binary_fill_holes(reg, structure=np.ones((3, 3))), (r0, c0)


def check_ring(mask, ring):
    """raises AssertionError with the reason if `ring` is not the ring of `mask`"""
    m = np.asarray(mask).astype(bool)
    H, W = m.shape
    filled, first = expected_region(m)
    if filled is None:
        assert ring == [], "empty mask must give an empty ring"
        return
    assert len(ring) >= 5 and ring[0] == ring[-1], "ring not closed"
    pts = np.asarray(ring, dtype=np.float64)
    assert pts.ndim == 2 and pts.shape[1] == 2 and np.all(pts == np.round(pts)), "vertices must be integral [x, y] pairs"
    pts = pts.astype(np.int64)
    assert pts[:, 0].min() >= 0 and pts[:, 0].max() <= W and pts[:, 1].min() >= 0 and pts[:, 1].max() <= H, "vertex outside the lattice"
    assert (int(pts[0, 0]), int(pts[0, 1])) == (first[1], first[0]), f"ring starts at {tuple(pts[0])}, region at x, y = {first[1], first[0]}"
    d = np.diff(pts, axis=0)
    assert np.all((d[:, 0] == 0) != (d[:, 1] == 0)), "an edge is diagonal or has no length"
    horizontal = d[:, 1] == 0
    assert np.all(horizontal != np.roll(horizontal, -1)), "two consecutive collinear edges"
    x, y = pts[:, 0], pts[:, 1]
    assert int((x[:-1] * y[1:] - x[1:] * y[:-1]).sum()) > 0, "ring is not clockwise in image coordinates"
    cross = np.zeros((H, W + 1), dtype=np.int64)
    for (xa, ya), (xb, yb) in zip(pts[:-1], pts[1:]):
        if xa == xb:
            cross[min(ya, yb):max(ya, yb), xa] ^= 1
    inside = (np.cumsum(cross, axis=1)[:, :W] % 2).astype(bool)        # odd number of vertical edges left of the pixel
    assert np.array_equal(inside, filled), f"refilled ring differs from the region in {int((inside != filled).sum())} pixels"


# ---------------------------------------------------------------------------------------------------------- cases

def _z(h, w):
    return np.zeros((h, w), dtype=bool)


def hand_made():
    """[(name, mask)]: the shapes of test_masks_to_polygons_ring_tracer_known_answers and the corner cases"""
    out = []
    rect = _z(6, 8); rect[1:4, 2:6] = True
    out.append(("rectangle", rect))
    ell = _z(6, 6); ell[1:5, 1:3] = True; ell[3:5, 3:5] = True
    out.append(("L", ell))
    holed = np.ones((5, 5), bool); holed[2, 2] = False
    out.append(("holed square", holed))
    two = _z(5, 9); two[1:3, 1:3] = True; two[1:4, 5:8] = True
    out.append(("two regions", two))
    diag = _z(4, 4); diag[0, 0] = diag[1, 1] = diag[1, 2] = diag[2, 1] = True
    out.append(("diagonal contact", diag))
    out.append(("empty", _z(3, 3)))
    one = _z(5, 7); one[3, 4] = True
    out.append(("single pixel", one))
    out.append(("1 x 1 full", np.ones((1, 1), bool)))
    out.append(("full frame", np.ones((9, 13), bool)))
    row = _z(1, 67); row[0, 3:66] = True
    out.append(("1 x N", row))
    out.append(("N x 1", np.ones((70, 1), bool)))
    cross = _z(11, 15); cross[5, :] = True; cross[:, 7] = True
    out.append(("touches all four borders", cross))
    tie = _z(7, 12); tie[4:6, 1:4] = True; tie[1:3, 7:10] = True; tie[1, 0] = True      # 6 = 6 > 1: of the two largest, the one starting in row 1 wins
    out.append(("equal sizes", tie))
    tie2 = _z(4, 9); tie2[1:3, 0:2] = True; tie2[1:3, 3:5] = True; tie2[1:3, 6:8] = True
    out.append(("three equal sizes in one row", tie2))
    inner = _z(12, 12); inner[0, :] = inner[-1, :] = True; inner[:, 0] = inner[:, -1] = True; inner[2:10, 2:10] = True   # 44 < 64
    out.append(("larger region inside a smaller ring", inner))
    outer = _z(12, 12); outer[0:2, :] = outer[-2:, :] = True; outer[:, 0:2] = outer[:, -2:] = True; outer[4:8, 4:8] = True   # 80 > 16
    out.append(("smaller region inside a larger ring", outer))
    yy, xx = np.mgrid[0:9, 0:10]
    out.append(("checkerboard", (yy + xx) % 2 == 0))
    out.append(("checkerboard, other phase", (yy + xx) % 2 == 1))
    pinch = _z(6, 6); pinch[0:2, 0:2] = True; pinch[2:4, 2:4] = True; pinch[1, 2] = True; pinch[4, 4] = True
    out.append(("pinched corners on the ring", pinch))
    spiral = _z(9, 9); spiral[0, :] = spiral[:, 8] = spiral[8, :] = True; spiral[2:, 0] = True; spiral[2, 0:7] = True
    spiral[2:7, 6] = True; spiral[6, 2:7] = True; spiral[4:7, 2] = True; spiral[4, 2:5] = True
    out.append(("spiral", spiral))
    return out


def noise_batches(seed=20260):
    """[(name, masks bool [R, H, W])]: seeded noise at densities 0.3 / 0.5 / 0.6 / 0.8, H and W drawn from 1..70 plus fixed
    sizes around the 4- and 64-column seams, one batch of 300 masks; a few masks of every batch are left empty"""
    rng = np.random.RandomState(seed)
    sizes = [(1, 1), (1, 70), (70, 1), (2, 3), (33, 65), (64, 64), (17, 63), (70, 70), (5, 66), (39, 39)]
    sizes += [(int(rng.randint(1, 71)), int(rng.randint(1, 71))) for _ in range(14)]
    out = []
    for i, (h, w) in enumerate(sizes):
        R = 300 if (h, w) == (39, 39) else int(rng.randint(3, 25))
        dens = rng.choice([0.3, 0.5, 0.6, 0.8], size=R)
        masks = rng.rand(R, h, w) < dens[:, None, None]
        masks[rng.rand(R) < 0.08] = False
        out.append((f"noise {h} x {w} x {R}", masks))
    return out


def serpentine(h, w):
    """one region one pixel wide that fills every other row and turns at the ends: perimeter ~ 2 * area"""
    m = _z(h, w)
    m[0::2, :] = True
    for k, r in enumerate(range(1, h, 2)):
        m[r, w - 1 if k % 2 == 0 else 0] = True
    return m


def comb(h, w):
    """a spine along the top with one-pixel teeth in every other column"""
    m = _z(h, w)
    m[0, :] = True
    m[:, 0::2] = True
    return m


def big_window(n=1600):
    """one region spanning an n x n window with a long outline: a jagged diagonal band, a cross reaching the four borders and
    combs hanging from the cross, a hole, and a second smaller region"""
    m = _z(n, n)
    m[n // 2 - 2:n // 2 + 2, :] = True
    m[:, n // 3:n // 3 + 5] = True
    for k in range(0, n - 8, 4):
        m[k:k + 6, k:k + 6] = True
    m[n // 2:n // 2 + 90, 0:n // 4:2] = True
    m[n // 2 - 60:n // 2, n // 2 + 40:n - 1:3] = True
    m[n // 8:n // 8 + 40, n // 2 + 100:n // 2 + 300] = True
    m[n // 2 - 1:n // 2 + 1, 40:60] = False
    return m


def lds_words(mask):
    """64-bit words of the window's bitmap as csrc/mask_rings.hip lays it out: rows of ceil(w / 64) words"""
    rows, cols = np.nonzero(np.asarray(mask))
    if len(rows) == 0:
        return 0
    return (int(rows.max() - rows.min()) + 1) * ((int(cols.max() - cols.min()) + 1 + 63) // 64)


def word_masks(R=100, M=28, seed=7):
    """float32 [R, M, M] probabilities shaped like a word's mask: a rounded box with a wavy outline, and a few stray blobs"""
    rng = np.random.RandomState(seed)
    v, u = np.mgrid[0:M, 0:M]
    u = (u + 0.5) / M * 2 - 1
    v = (v + 0.5) / M * 2 - 1
    out = np.zeros((R, M, M), dtype=np.float32)
    for r in range(R):
        a, b = rng.uniform(0.75, 0.95), rng.uniform(0.6, 0.9)
        wob = 0.12 * np.sin(u * rng.uniform(3, 9) + rng.uniform(0, 6)) + 0.1 * np.cos(v * rng.uniform(2, 6) + rng.uniform(0, 6))
        logit = 6.0 * (1.0 - (np.abs(u / a) ** 4 + np.abs((v + wob) / b) ** 4)) + rng.normal(0, 0.8, (M, M))
        out[r] = 1.0 / (1.0 + np.exp(-logit))
    return out
