"""Cases shared by tests/test_rotate.py (host, against Pillow and the committed golden) and tests/test_gpu_rotate.py (device,
against the host statement).  Inputs are seeded, so every file that names a case sees the same bytes.

`contracted_pixel` is the statement of one output pixel as a compiler that fuses multiply-adds would evaluate it, emulated with
exact rational arithmetic rounded once per fused operation; `search_fma_case` looks for an image on which that differs from
the statement (python tests/rotate_cases.py prints what it finds), and FMA_CASE is what it found."""
import math
import os
from fractions import Fraction

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rotate_pil.npz")

SIZES = [(1, 1), (1, 9), (9, 1), (2, 2), (7, 5), (33, 64), (64, 64), (100, 37), (130, 257)]   # the last crosses tile and dword
ANGLES = [0, 90, 180, 270, 360, -90, 15, 30, 45, 60, 75, -170, 33.3, 359.9, 1e-3, 89.999]    # boundaries on both axes
FILLS = [(0, 0, 0), (7, 200, 255)]
KINDS = ("noise", "ones", "checker")

# the search's finding: (h, w), angle, input kind, fill, and one pixel (x, y, channel) of the output at which the contracted
# evaluation gives another byte than the statement
FMA_CASE = {"hw": (1, 9), "angle": 75, "kind": "noise", "fill": (0, 0, 0), "pixel": (2, 4, 2), "statement": 176, "contracted": 175}


def make_image(h: int, w: int, kind: str = "noise") -> np.ndarray:
    if kind == "ones":                      # truncation must give 255 inside, never 254
        return np.full((h, w, 3), 255, dtype=np.uint8)
    if kind == "checker":
        y, x = np.mgrid[0:h, 0:w]
        return np.repeat((((x + y) & 1) * 255).astype(np.uint8)[:, :, None], 3, axis=2)
    rng = np.random.default_rng(1000 * h + w)
    return rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)


def all_cases():
    """(name, image, angle, fill): every size x angle x fill with noise, plus a constant-255 image and a checkerboard at every
    angle on two sizes, plus the contraction case"""
    out = []
    for h, w in SIZES:
        for a in ANGLES:
            for fill in FILLS:
                out.append((f"noise_{h}x{w}_{a}_{fill[0]}", make_image(h, w), a, fill))
    for h, w in ((7, 5), (33, 64)):
        for a in ANGLES:
            out.append((f"ones_{h}x{w}_{a}", make_image(h, w, "ones"), a, FILLS[1]))
            out.append((f"checker_{h}x{w}_{a}", make_image(h, w, "checker"), a, FILLS[0]))
    c = FMA_CASE
    out.append(("fma_case", make_image(*c["hw"], c["kind"]), c["angle"], c["fill"]))
    return out


GOLDEN_CASES = [(h, w, a, f) for (h, w) in SIZES[:5] for a, f in ((0, 0), (90, 0), (180, 1), (270, 1), (15, 0), (45, 1), (-170, 0),
                                                                    (33.3, 1), (359.9, 0), (1e-3, 1), (89.999, 0))]


def golden_name(h, w, a, f) -> str:
    return f"r_{h}x{w}_{a!r}_{f}"


def pil_rotate(img: np.ndarray, angle: float, fill) -> np.ndarray:
    from PIL import Image
    bilinear = getattr(Image, "Resampling", Image).BILINEAR
    return np.asarray(Image.fromarray(img).rotate(angle, resample=bilinear, expand=True, fillcolor=tuple(fill)))


def write_golden() -> None:
    """regenerate tests/golden/rotate_pil.npz with Pillow"""
    np.savez_compressed(GOLDEN, **{golden_name(h, w, a, f): pil_rotate(make_image(h, w), a, FILLS[f]) for h, w, a, f in GOLDEN_CASES})


# ------------------------------------------------------------------ the fused-multiply-add question
def _fma(a: float, b: float, c: float) -> float:
    """a * b + c rounded once (Fraction -> float is correctly rounded)"""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def contracted_pixel(img: np.ndarray, m, x: int, y: int, fill):
    """the three bytes of output pixel (x, y) with every `p * q + r` of the statement fused: the coordinates as
    fma(m0, xc, m1 * yc) + m2 (the contraction a compiler makes of a sum of two products), v = fma(b - a, d, a)"""
    h, w = img.shape[:2]
    xc, yc = x + 0.5, y + 0.5
    xin = _fma(m[0], xc, m[1] * yc) + m[2]
    yin = _fma(m[3], xc, m[4] * yc) + m[5]
    if not (0.0 <= xin < w and 0.0 <= yin < h):
        return tuple(fill)
    xin -= 0.5
    yin -= 0.5
    x0, y0 = math.floor(xin), math.floor(yin)
    dx, dy = xin - x0, yin - y0
    xa, xb, ya = min(max(x0, 0), w - 1), min(max(x0 + 1, 0), w - 1), min(max(y0, 0), h - 1)
    out = []
    for c in range(3):
        a, b = float(img[ya, xa, c]), float(img[ya, xb, c])
        v1 = _fma(b - a, dx, a)
        v2 = v1
        if 0 <= y0 + 1 < h:
            p, q = float(img[y0 + 1, xa, c]), float(img[y0 + 1, xb, c])
            v2 = _fma(q - p, dx, p)
        out.append(int(_fma(v2 - v1, dy, v1)))
    return tuple(out)


def search_fma_case(sizes=((1, 9), (9, 1), (2, 2), (7, 5)), angles=tuple(ANGLES) + (60 - 1e-9, 60 + 1e-9), kinds=KINDS):
    """every (size, angle, input kind) -> the first output pixel and channel at which the contracted evaluation differs from the
    statement; yields (h, w, angle, kind, (x, y, c), statement byte, contracted byte)"""
    from glass_amd.data import RotationTransform, rotate_u8_host
    for h, w in sizes:
        for a in angles:
            t = RotationTransform(h, w, a)
            if t.kind < 4:
                continue
            for kind in kinds:
                img = make_image(h, w, kind)
                want = rotate_u8_host(img, t, FILLS[0])
                hit = None
                for y in range(t.out_hw[0]):
                    for x in range(t.out_hw[1]):
                        got = contracted_pixel(img, t.matrix, x, y, FILLS[0])
                        for c in range(3):
                            if got[c] != int(want[y, x, c]) and hit is None:
                                hit = (h, w, a, kind, (x, y, c), int(want[y, x, c]), got[c])
                if hit is not None:
                    yield hit


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "glass-text-spotting_amd"))
    if sys.argv[1:] == ["golden"]:
        write_golden()
    else:
        for found in search_fma_case():
            print(found)
