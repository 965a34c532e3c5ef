"""Tile plans of the tiled restore loop (daclip_amd/tiling.py): pure Python, no GPU.

For a sweep of (L, tile, overlap) every plan must ascend, stay in bounds, cover the axis, give
every position a positive weight sum and end at L - l; and the blend of constant tiles, restated
in numpy exactly as the kernel defines it (fp32, tiles in ascending order, separate multiply and
add, one division, single-covered pixels copied), must return the constant.
"""
import numpy as np
import pytest

from daclip_amd import tiling

# (L, tile, overlap): L < tile, L == tile, L == tile + 1, overlap 0, exact multiples of the
# stride, a clamped last tile, the largest overlap (stride 1), odd sizes.
SWEEP = [(20, 32, 8), (32, 32, 16), (33, 32, 16), (33, 32, 0), (64, 32, 0), (96, 32, 0),
         (48, 32, 16), (64, 32, 16), (40, 32, 16), (34, 32, 16), (100, 32, 31), (37, 5, 2),
         (1024, 256, 32), (2048, 256, 32), (3072, 256, 32), (257, 256, 32), (7, 2, 1), (2, 2, 0)]


@pytest.mark.parametrize("L,tile,ov", SWEEP)
def test_plan_axis_properties(L, tile, ov):
    l, offs = tiling.plan_axis(L, tile, ov)
    assert l == min(tile, L)
    assert offs[0] == 0
    assert all(b > a for a, b in zip(offs, offs[1:]))                  # ascending
    assert all(0 <= o <= L - l for o in offs)                          # in bounds
    assert offs[-1] == L - l                                           # the last tile ends the axis
    s = l - ov
    assert len(offs) == (1 if L <= l else -(-(L - l) // s) + 1)
    assert all(b - a <= s for a, b in zip(offs, offs[1:]))             # overlap >= ov everywhere
    w1 = tiling.axis_weights(l, ov)
    assert w1 == [min(i + 1, l - i, ov + 1) for i in range(l)] and min(w1) >= 1
    cover = np.zeros(L, np.int64)
    wsum = np.zeros(L, np.int64)
    for o in offs:
        cover[o:o + l] += 1
        wsum[o:o + l] += np.asarray(w1)
    assert (cover >= 1).all()                                          # every position covered
    assert (wsum > 0).all()


def test_plan_matches_the_documented_grids():
    assert tiling.plan(48, 40, 32, 16) == (32, 32, [0, 16], [0, 8])
    assert tiling.plan(30, 34, 32, 16) == (30, 32, [0], [0, 2])
    assert tiling.plan(64, 64, 32, 0) == (32, 32, [0, 32], [0, 32])
    assert tiling.plan(32, 32, 32, 16) == (32, 32, [0], [0])
    assert tiling.plan(48, 40, (32, 24), 8) == (32, 24, [0, 16], [0, 16])
    th, tw, ys, xs = tiling.plan(2048, 3072, 256, 32)
    assert (th, tw, len(ys), len(xs)) == (256, 256, 9, 14)


@pytest.mark.parametrize("args", [(48, 40, 32, 32), (48, 40, 32, -1), (48, 40, 1, 0), (30, 34, 32, 30),
                                  (48, 40, (32, 32, 32), 8)])
def test_plan_refuses(args):
    with pytest.raises(ValueError):
        tiling.plan(*args)


def blend_numpy(tiles, B, H, W, th, tw, ov, ys, xs):
    """The blend as the kernel defines it, in fp32 numpy."""
    wy = np.asarray(tiling.axis_weights(th, ov), np.float32)
    wx = np.asarray(tiling.axis_weights(tw, ov), np.float32)
    w = wy[:, None] * wx[None, :]
    acc = np.zeros((B, 3, H, W), np.float32)
    ws = np.zeros((H, W), np.float32)
    cnt = np.zeros((H, W), np.int64)
    copy = np.zeros((B, 3, H, W), np.float32)
    for iy, y0 in enumerate(ys):
        for ix, x0 in enumerate(xs):
            cnt[y0:y0 + th, x0:x0 + tw] += 1
            ws[y0:y0 + th, x0:x0 + tw] += w
            for b in range(B):
                t = tiles[(b * len(ys) + iy) * len(xs) + ix]
                prod = (w[None] * t).astype(np.float32)                # one rounding
                acc[b, :, y0:y0 + th, x0:x0 + tw] += prod               # another
                copy[b, :, y0:y0 + th, x0:x0 + tw] = t
    assert (cnt >= 1).all()
    with np.errstate(invalid="ignore", divide="ignore"):
        out = acc / ws
    return np.where(cnt == 1, copy, out), cnt


@pytest.mark.parametrize("H,W,tile,ov", [(48, 40, 32, 16), (30, 34, 32, 16), (64, 64, 32, 0), (70, 45, 32, 31),
                                         (33, 33, 32, 5)])
@pytest.mark.parametrize("c", [1.0, -0.3, 1e-3, 12345.678])
def test_constant_tiles_blend_to_the_constant(H, W, tile, ov, c):
    th, tw, ys, xs = tiling.plan(H, W, tile, ov)
    B = 2
    tiles = np.full((B * len(ys) * len(xs), 3, th, tw), c, np.float32)
    out, cnt = blend_numpy(tiles, B, H, W, th, tw, ov, ys, xs)
    assert (out[:, :, cnt == 1] == np.float32(c)).all()                # single cover: a copy
    if c == 1.0:
        assert (out == 1.0).all()          # integer products and sums are exact in fp32
    # K covering tiles: K products, K - 1 sums and one division, each within half an ulp
    # (eps / 2) of exact on positive terms, so the quotient is within (2 K) * eps / 2 of c.
    np.testing.assert_allclose(out, np.float32(c), rtol=int(cnt.max()) * np.finfo(np.float32).eps, atol=0)
