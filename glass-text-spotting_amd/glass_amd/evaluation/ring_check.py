"""`sort_detection`'s per-line test on the device: which detection rings are dropped (fewer than 3 points, zero area, two
properly crossing sides) and which are reversed (csrc/ring_check.hip through ops.native.ring_check; reference
glass/evaluation/text_evaluator.py:112-137).  The host function `text_evaluator.normalize_detection_line` is the definition:
its pair loop is quadratic in the ring length, which is nothing for a box and everything for a traced mask outline; here all
rings of a call are checked in one device call, in exact integer arithmetic, and only the strings are formed on the host."""
from __future__ import annotations

from itertools import chain
from typing import List, Optional, Sequence

import numpy as np

from .text_evaluator import normalize_detection_line

DROP, KEEP, REVERSE = 0, 1, 2


def host_verdict(flat: Sequence[int]) -> int:
    """The verdict of `normalize_detection_line` for one ring [x1, y1, ..., xn, yn] of Python integers of any size."""
    if normalize_detection_line(",".join(str(int(v)) for v in flat) + ",####") is None:
        return DROP
    xs, ys = flat[0::2], flat[1::2]
    n = len(xs)
    return KEEP if sum(xs[i] * ys[(i + 1) % n] - xs[(i + 1) % n] * ys[i] for i in range(n)) < 0 else REVERSE


class RingChecker:
    """Batched validity / winding check of integer rings on `device` (a HIP device; there is no CPU fallback: without a
    checker the callers use `normalize_detection_line`).  Hand one to `TextResultWriter(..., ring_checker=)` and
    `RRCScorer(..., ring_checker=)`."""

    def __init__(self, device):
        import torch
        from ..ops import native as K
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise K.GlassLibraryError(f"RingChecker needs a HIP device (got {self.device}); without one use normalize_detection_line")
        self.max_coord, self.max_points = K.RING_CHECK_MAX_COORD, K.RING_CHECK_MAX_POINTS

    def out_of_range(self, flats: Sequence[Sequence[int]]) -> np.ndarray:
        """bool [n]: rings the kernel's exactness bounds exclude (a coordinate beyond 2^20 in magnitude, more than 2^20 points)"""
        n = len(flats)
        counts = np.fromiter((len(f) // 2 for f in flats), dtype=np.int64, count=n)
        big = counts > self.max_points
        try:
            flat = np.fromiter(chain.from_iterable(flats), dtype=np.int64, count=int(sum(len(f) for f in flats)))
        except OverflowError:                                          # a coordinate beyond int64: ask ring by ring
            return big | np.fromiter((any(abs(v) > self.max_coord for v in f) for f in flats), dtype=bool, count=n)
        far = np.abs(flat) > self.max_coord
        if far.any():
            ring_of = np.repeat(np.arange(n), [len(f) for f in flats])
            big[np.unique(ring_of[far])] = True
        return big

    def check_flat(self, flats: Sequence[Sequence[int]]) -> np.ndarray:
        """`check` for rings given as [x1, y1, ..., xn, yn]"""
        import torch
        from ..ops import native as K
        n = len(flats)
        verdict = np.zeros((n,), dtype=np.int32)
        if n == 0:
            return verdict
        big = self.out_of_range(flats)
        on_device = np.nonzero(~big)[0]
        for k in np.nonzero(big)[0]:
            verdict[k] = host_verdict(list(flats[k]))
        if on_device.size:
            mine = flats if on_device.size == n else [flats[k] for k in on_device]
            counts = np.fromiter((len(f) // 2 for f in mine), dtype=np.int64, count=len(mine))
            flat = np.fromiter(chain.from_iterable(mine), dtype=np.int32, count=int(counts.sum()) * 2)
            off = np.concatenate([[0], np.cumsum(counts)])
            pts = K.upload(flat.reshape(-1, 2), torch.int32, self.device)
            verdict[on_device] = K.ring_check(pts, off)[0].cpu().numpy()
        return verdict

    def check(self, rings: Sequence[Sequence[Sequence[int]]]) -> np.ndarray:
        """int32 [n] verdicts of `normalize_detection_line` for a sequence of point lists [(x, y), ...] of integers: 0 the line
        is dropped, 1 kept as it stands, 2 kept with the point order reversed.  One device call for all rings; a ring outside
        the kernel's bounds (a coordinate beyond 2^20 in magnitude, more than 2^20 points) is decided on the host."""
        return self.check_flat([[int(v) for p in r for v in p] for r in rings])

    def normalize_lines(self, lines: Sequence[str]) -> List[Optional[str]]:
        """[normalize_detection_line(l) for l in lines], element for element, with the rings of all lines checked in one
        device call.  Lines are split and parsed as the host function does, and a malformed one raises what it raises; a
        line outside the kernel's bounds goes through the host function."""
        recs, flats = [], []
        for line in lines:
            ptr = line.strip().split(",####")
            rec = ptr[1]
            cors = ptr[0].split(",")
            assert len(cors) % 2 == 0, "cors invalid."
            flats.append([int(c) for c in cors])
            recs.append(rec)
        if not flats:
            return []
        big = self.out_of_range(flats)
        verdict = self.check_flat([[] if b else f for f, b in zip(flats, big)])
        out: List[Optional[str]] = []
        for line, rec, f, v, b in zip(lines, recs, flats, verdict.tolist(), big.tolist()):
            if b:
                out.append(normalize_detection_line(line))
            elif v == DROP:
                out.append(None)
            else:
                if v == REVERSE:
                    g = [0] * len(f)
                    g[0::2], g[1::2] = f[0::2][::-1], f[1::2][::-1]
                    f = g
                out.append(",".join(map(str, f)) + ",####" + rec)
        return out
