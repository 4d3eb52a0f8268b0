"""The tile grid of tiled inference (MODEL.CATSEG_HIP.TILED): the one definition of its geometry.

Per axis, for image extent L, tile t and stride s:

    t'  = min(t, L)
    n   = max(L - t' + s - 1, 0) // s + 1
    o_i = min(i * s, L - t')          i = 0 .. n-1

The last tile is shifted back to end at L, never padded.  With t / 2 <= s <= t a position is covered by 1
to 3 tiles per axis (3 where the shifted last tile overlaps two regular ones).  Tiles are row-major: tile
row r at oy_r, column c at ox_c, all of extent (th, tw).  The kernels (csrc/post_tiled.hip) receive
(L, t', s) as scalars and evaluate the same o_i."""
from __future__ import annotations

from typing import Iterator, List, NamedTuple, Tuple


def _pair(v) -> Tuple[int, int]:
    if isinstance(v, (tuple, list)):
        a, b = v
        return int(a), int(b)
    return int(v), int(v)


def check_tile_stride(tile: int, stride: int, divisibility: int = 1) -> None:
    """The rule of one axis: TILE a positive multiple of size_divisibility, TILE / 2 <= STRIDE <= TILE."""
    if tile <= 0 or (divisibility > 1 and tile % divisibility):
        raise ValueError(f"tiling: TILE must be a positive multiple of the size divisibility {divisibility}, got {tile}")
    if not (tile <= 2 * stride and stride <= tile):
        raise ValueError(f"tiling: need TILE / 2 <= STRIDE <= TILE (a pixel is then covered by at most 3 tiles per "
                         f"axis), got TILE {tile}, STRIDE {stride}")


def grid_1d(L: int, t: int, s: int) -> Tuple[int, List[int]]:
    """(t', [o_0 .. o_{n-1}]) of one axis."""
    L, t, s = int(L), int(t), int(s)
    if L <= 0 or t <= 0 or s <= 0:
        raise ValueError(f"tiling: extent, tile and stride must be positive, got {L}, {t}, {s}")
    t = min(t, L)
    n = max(L - t + s - 1, 0) // s + 1
    return t, [min(i * s, L - t) for i in range(n)]


class TileGrid(NamedTuple):
    H: int
    W: int
    th: int
    tw: int
    sy: int
    sx: int
    oys: Tuple[int, ...]
    oxs: Tuple[int, ...]

    @property
    def ny(self) -> int:
        return len(self.oys)

    @property
    def nx(self) -> int:
        return len(self.oxs)

    def origins(self, r: int) -> List[Tuple[int, int]]:
        """(oy, ox) of the tiles of tile row r, in order."""
        return [(self.oys[r], ox) for ox in self.oxs]


def tile_grid(H: int, W: int, tile, stride) -> TileGrid:
    """The grid of an (H, W) image; tile / stride an int or a (y, x) pair."""
    (ty, tx), (sy, sx) = _pair(tile), _pair(stride)
    check_tile_stride(ty, sy)
    check_tile_stride(tx, sx)
    th, oys = grid_1d(H, ty, sy)
    tw, oxs = grid_1d(W, tx, sx)
    return TileGrid(int(H), int(W), th, tw, sy, sx, tuple(oys), tuple(oxs))


def covering(origins, t: int, p: int) -> Tuple[int, int]:
    """(first, last) index of the tiles of one axis that cover position p; they are contiguous."""
    idx = [i for i, o in enumerate(origins) if o <= p < o + t]
    return idx[0], idx[-1]


WINDOWS = ("uniform", "pyramid")                 # catseg_tiled_blend's window 0 / 1
PYRAMID_MAX_TILE = 2048                          # sum(w) <= 2.25 t'^2 < 2^24: the fp32 weights stay exact


def check_window(kind: str, tile=None) -> int:
    """The kernel's code of a window kind; "pyramid" refuses a tile extent above PYRAMID_MAX_TILE."""
    if kind not in WINDOWS:
        raise ValueError(f"tiling: the window must be one of {WINDOWS}, got {kind!r}")
    if kind == "pyramid" and tile is not None and max(_pair(tile)) > PYRAMID_MAX_TILE:
        raise ValueError(f"tiling: the pyramid window needs a tile extent of at most {PYRAMID_MAX_TILE} (its weights "
                         f"must sum below 2^24 to be exact in fp32), got {tile}")
    return WINDOWS.index(kind)


def window_weights(t: int, kind: str) -> List[int]:
    """The weights w(l), l = 0 .. t-1, of one axis of a tile of extent t (the t' of the grid): "uniform" 1,
    "pyramid" min(l + 1, t - l).  Integers, at least 1 everywhere.  A pixel of tile i has the weight
    w(y - oy_i) * w(x - ox_i); the merge is sum(w_i p_i) / sum(w_i) over the covering tiles
    (csrc/post_tiled.hip: catseg_tiled_blend evaluates the same integers)."""
    check_window(kind)
    t = int(t)
    return [min(l + 1, t - l) if kind == "pyramid" else 1 for l in range(t)]


def weight_sum(origins, t: int, L: int, kind: str) -> List[int]:
    """sum of w(p - o_i) over the tiles of one axis that cover p, for p = 0 .. L-1.  A pixel's sum(w_i) is
    the product of its two axes' sums."""
    w = window_weights(t, kind)
    out = [0] * int(L)
    for o in origins:
        for l in range(int(t)):
            out[o + l] += w[l]
    return out


def merge_schedule(H: int, th: int, sy: int) -> Iterator[Tuple[int, int, int, int]]:
    """Steps (row0, rows, y0, y1) of a streaming merge: output rows [y0, y1) are final once tile rows
    row0 .. row0 + rows - 1 are known.  The [y0, y1) ranges partition [0, H) in order, each window holds
    every tile row that covers a row of its range and at most 3 tile rows, and row0 never decreases: a
    ring of 3 tile rows of logits serves the whole image.  One step per tile row: after tile row r the
    rows up to the origin of tile row r + 1 (up to H after the last) can be no further covered."""
    _, oys = grid_1d(H, th, sy)
    th = min(th, H)
    y0 = 0
    for r in range(len(oys)):
        y1 = oys[r + 1] if r + 1 < len(oys) else H
        if y1 <= y0:
            continue
        row0 = covering(oys, th, y0)[0]
        last = covering(oys, th, y1 - 1)[1]
        assert last <= r and r - row0 < 3
        yield row0, last - row0 + 1, y0, y1
        y0 = y1
