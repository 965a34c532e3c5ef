"""Tile plans for the tiled restore loop (dac_sde_reverse_tiled).

Pure Python: no GPU, no library load. A plan is separable: row offsets `ys`, column offsets
`xs`, tiles of (th, tw) at their product. Along an axis of length L with tile l and overlap ov
the stride is s = l - ov; n = 1 if L <= l, else ceil((L - l) / s) + 1 tiles, tile j at
min(j * s, L - l): the last tile is clamped inward and overlaps its neighbour by more than ov.
The blend weight of position i of a tile side l is the integer ramp min(i + 1, l - i, ov + 1).
"""
from __future__ import annotations

from typing import List, Sequence, Tuple, Union


def plan_axis(L: int, tile: int, overlap: int) -> Tuple[int, List[int]]:
    """(effective tile l = min(tile, L), ascending offsets) along one axis."""
    L, tile, overlap = int(L), int(tile), int(overlap)
    if L < 1 or tile < 1:
        raise ValueError(f"plan_axis: L = {L}, tile = {tile} must be positive")
    l = min(tile, L)
    if overlap < 0 or overlap >= l:
        raise ValueError(f"plan_axis: overlap {overlap} must be in [0, {l}) for a tile of {l}")
    if L <= l:
        return l, [0]
    s = l - overlap
    n = -(-(L - l) // s) + 1
    return l, [min(j * s, L - l) for j in range(n)]


def tile_pair(tile: Union[int, Sequence[int]]) -> Tuple[int, int]:
    if isinstance(tile, (tuple, list)):
        if len(tile) != 2:
            raise ValueError(f"tile must be an int or (th, tw), got {tile!r}")
        return int(tile[0]), int(tile[1])
    return int(tile), int(tile)


def plan(H: int, W: int, tile: Union[int, Sequence[int]], overlap: int):
    """(th', tw', ys, xs) for an H x W image; `tile` is an int or (th, tw)."""
    th, tw = tile_pair(tile)
    th2, tw2 = min(th, int(H)), min(tw, int(W))
    if th2 < 2 or tw2 < 2:
        raise ValueError(f"plan: tile sides must be >= 2 (got {th2} x {tw2})")
    if overlap < 0 or overlap >= min(th2, tw2):
        raise ValueError(f"plan: overlap {overlap} must be in [0, min(th, tw) = {min(th2, tw2)})")
    _, ys = plan_axis(H, th2, overlap)
    _, xs = plan_axis(W, tw2, overlap)
    return th2, tw2, ys, xs


def axis_weights(l: int, overlap: int) -> List[int]:
    """w1(i) = min(i + 1, l - i, overlap + 1) for i < l."""
    return [min(i + 1, l - i, overlap + 1) for i in range(l)]
