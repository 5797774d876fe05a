"""Cases shared by tests/test_resize_pil.py (host, against PIL and the committed golden) and tests/test_gpu_resize_pil.py
(device, against the host statement).  Inputs are seeded uint8 noise unless a fill value is given, so every file that
names a case sees the same bytes."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "resize_pil.npz")

# name -> ((H, W), (Ho, Wo), fill): fill None = seeded noise, else a constant image
CASES = {
    "up_7x5": ((7, 5), (13, 9), None),                    # upscale; 1 or 2 taps at the clipped borders
    "down_37x53": ((37, 53), (20, 31), None),             # non-integer reduction
    "down_401x603": ((401, 603), (40, 31), None),         # factors 10.0 and 19.5: ksize 23 and 41
    "to_1x1": ((3, 3), (1, 1), None),
    "one_row": ((1, 9), (4, 2), None),                    # 1-pixel axis, up on one axis and down on the other
    "x_only": ((50, 64), (50, 23), None),                 # vertical pass skipped
    "y_only": ((33, 17), (8, 17), None),                  # horizontal pass skipped
    "same": ((12, 12), (12, 12), None),                   # both skipped
    "wide": ((20, 1030), (31, 1285), None),               # width no multiple of a block or wavefront, more than one block
    "zeros_up": ((7, 5), (13, 9), 0),
    "zeros_down": ((37, 53), (20, 31), 0),
    "ones_up": ((7, 5), (13, 9), 255),
    "ones_down": ((37, 53), (20, 31), 255),
}
PROTOCOL = ((720, 1280), (1000, 1778), None)              # the evaluation protocol's own shape: index width only
GOLDEN_CASES = [n for n in CASES if n != "wide"]          # the small ones (the file is a few KB)


def make_input(name_or_case) -> np.ndarray:
    (H, W), _, fill = CASES[name_or_case] if isinstance(name_or_case, str) else name_or_case
    if fill is not None:
        return np.full((H, W, 3), fill, dtype=np.uint8)
    rng = np.random.default_rng(1000 * H + W)
    return rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)


def pil_resize(img: np.ndarray, out_hw) -> np.ndarray:
    from PIL import Image
    bilinear = getattr(Image, "Resampling", Image).BILINEAR
    return np.asarray(Image.fromarray(img).resize((int(out_hw[1]), int(out_hw[0])), bilinear))


def write_golden() -> None:
    """regenerate tests/golden/resize_pil.npz with PIL (python tests/resize_pil_cases.py)"""
    np.savez_compressed(GOLDEN, **{n: pil_resize(make_input(n), CASES[n][1]) for n in GOLDEN_CASES})


if __name__ == "__main__":
    write_golden()
