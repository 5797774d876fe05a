"""Tile plan of tiled inference (`GlassRunner.run_tiled`): overlapping equal tiles over a large image, and per tile the
rectangle inside which a detection counts as whole.  Pure Python, no device.

Along one axis the tiles start at 0, step, 2*step, ... (step = tile - overlap) while a further tile would still end inside the
extent, and one last tile lies flush with the far edge.  A detection is taken from a tile only if its corners lie inside the
tile's keep rectangle: the tile pulled in by `border` on every side that is not an image edge (a box whose corner comes
nearer to an interior tile edge than that may be a fragment of a word the edge cut).  Consecutive tiles overlap by at least
`overlap`, so every interval of length at most L = overlap - 2*border lies inside the keep interval of some tile: a word
whose axis-aligned extent is at most L is seen whole, with the margin, by at least one tile."""
from __future__ import annotations

import math
from typing import List, NamedTuple, Tuple


class Tile(NamedTuple):
    y0: int
    x0: int
    h: int
    w: int
    keep: Tuple[float, float, float, float]      # kx0, ky0, kx1, ky1 in the image's frame; -inf / +inf on an image edge


class TilePlan(NamedTuple):
    height: int
    width: int
    tile: int
    overlap: int
    border: int
    ys: Tuple[int, ...]                          # tile origins along y
    xs: Tuple[int, ...]                          # tile origins along x
    tiles: Tuple[Tile, ...]                      # row-major: ys outer, xs inner

    @property
    def max_whole(self) -> int:
        """L: the largest extent that is guaranteed to lie whole inside some tile's keep rectangle"""
        return self.overlap - 2 * self.border


def axis_origins(extent: int, tile: int, overlap: int) -> List[int]:
    if extent <= tile:
        return [0]
    step = tile - overlap
    origins = []
    o = 0
    while o + tile < extent:
        origins.append(o)
        o += step
    if extent - tile not in origins:
        origins.append(extent - tile)
    return origins


def axis_keep(origin: int, size: int, extent: int, border: int) -> Tuple[float, float]:
    lo = -math.inf if origin == 0 else float(origin + border)
    hi = math.inf if origin + size == extent else float(origin + size - border)
    return lo, hi


def plan_tiles(height: int, width: int, tile: int, overlap: int, border: int) -> TilePlan:
    height, width, tile, overlap, border = int(height), int(width), int(tile), int(overlap), int(border)
    if height < 1 or width < 1:
        raise ValueError(f"plan_tiles: image of {height} x {width}")
    if tile < 32 or tile % 32 != 0:
        raise ValueError(f"plan_tiles: tile={tile} must be a positive multiple of 32")
    if not 0 <= 2 * border < overlap < tile:
        raise ValueError(f"plan_tiles: needs 0 <= 2*border < overlap < tile (border={border}, overlap={overlap}, tile={tile})")
    ys, xs = axis_origins(height, tile, overlap), axis_origins(width, tile, overlap)
    h, w = min(tile, height), min(tile, width)
    tiles = []
    for y0 in ys:
        ky0, ky1 = axis_keep(y0, h, height, border)
        for x0 in xs:
            kx0, kx1 = axis_keep(x0, w, width, border)
            tiles.append(Tile(y0, x0, h, w, (kx0, ky0, kx1, ky1)))
    return TilePlan(height, width, tile, overlap, border, tuple(ys), tuple(xs), tuple(tiles))
