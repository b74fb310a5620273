"""NumPy restatement of ``cv2.createCLAHE(clipLimit, tileGridSize).apply(u8 plane)`` -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.

Written from OpenCV's algorithm (modules/imgproc/src/clahe.cpp), not from oracle/cvref.c: whole-array NumPy where cvref.c
loops, modular arithmetic where cvref.c reflects step by step.  tests/test_clahe_cases.py holds the two against each other;
neither has been held against cv2 itself, which is not installed where this was written.

The algorithm, in OpenCV's order:
  * a frame that is ragged in EITHER direction is padded in BOTH: ``copyMakeBorder(src, 0, ty - H % ty, 0, tx - W % tx,
    BORDER_REFLECT_101)`` (a direction that divides evenly gets a whole extra tile row / column share), and a pad wider
    than the plane reflects again and again (borderInterpolate's loop): period ``2 (len - 1)``, a plane of one sample
    repeats it;
  * integer clip limit ``max(int(clipLimit * area / 256), 1)``, none at all for ``clipLimit <= 0``;
  * per tile: 256-bin histogram, counts above the limit cut off, the cut total handed back as ``total // 256`` to every
    bin plus one more to every ``max(256 // residual, 1)``-th bin from bin 0 until the residual is used up;
  * tile LUT ``saturate_cast<uchar>(cumulative * lutScale)`` with the float32 ``lutScale = 255.f / area``: one float32
    product, cvRound (half to even);
  * per pixel the tile coordinates ``x * (1.f / tw) - 0.5f`` (float32), ``floor``, the weights before the indices are
    clamped, and ``(l11 * xa1 + l12 * xa) * ya1 + (l21 * xa1 + l22 * xa) * ya`` in float32, cvRound, saturate.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

F32 = np.float32


class Clahe(NamedTuple):
    out: np.ndarray      # uint8 [H, W]
    luts: np.ndarray     # uint8 [tiles_y, tiles_x, 256]
    lut_ties: int        # LUT entries whose scaled cumulative count is exactly k + 0.5
    blend_ties: int      # pixels whose blended value is exactly k + 0.5
    info: dict           # geometry and clipping figures, for the preconditions of tests/test_clahe_cases.py


def reflect101(idx, n: int):
    """BORDER_REFLECT_101 (gfedcb|abcdefgh|gfedcba) of any integer index into ``n`` samples."""
    idx = np.asarray(idx, dtype=np.int64)
    if n == 1:
        return np.zeros_like(idx)
    period = 2 * (n - 1)
    m = np.mod(idx, period)
    return np.where(m < n, m, period - m)


def geometry(H: int, W: int, tiles=(8, 8), clip_limit: float = 2.0) -> dict:
    """Padded size, tile size and integer clip limit of an H x W plane under ``tiles = (tiles_x, tiles_y)``."""
    tx, ty = int(tiles[0]), int(tiles[1])
    padded = W % tx != 0 or H % ty != 0
    He, We = (H + (ty - H % ty), W + (tx - W % tx)) if padded else (H, W)
    tw, th = We // tx, He // ty
    area = tw * th
    limit = max(int(float(clip_limit) * area / 256), 1) if clip_limit > 0 else 0
    return dict(padded=padded, He=He, We=We, tw=tw, th=th, area=area, limit=limit)


def tile_histograms(plane, tiles=(8, 8)):
    """int64 [tiles_y * tiles_x, 256]: the histogram of every tile of the padded plane, row-major over the tile grid."""
    src = np.asarray(plane)
    assert src.dtype == np.uint8 and src.ndim == 2
    H, W = src.shape
    g = geometry(H, W, tiles)
    tx, ty = int(tiles[0]), int(tiles[1])
    ext = src[reflect101(np.arange(g["He"]), H)[:, None], reflect101(np.arange(g["We"]), W)[None, :]]
    tile_of = (np.arange(g["He"]) // g["th"])[:, None] * tx + (np.arange(g["We"]) // g["tw"])[None, :]
    return np.bincount((tile_of * 256 + ext).ravel(), minlength=tx * ty * 256).reshape(tx * ty, 256)


def redistribute(hist, limit: int):
    """Clip every row of ``hist`` at ``limit`` and hand the cut counts back; returns (hist, cut total per row)."""
    hist = hist.copy()
    cut = np.maximum(hist - limit, 0).sum(axis=1)
    np.minimum(hist, limit, out=hist)
    batch = cut // 256
    residual = cut - batch * 256
    hist += batch[:, None]
    for k in np.flatnonzero(residual):
        step = max(256 // int(residual[k]), 1)
        hist[k, np.arange(0, 256, step)[:int(residual[k])]] += 1
    return hist, cut


def half(x):
    """Elements of a float32 array that sit exactly on k + 0.5."""
    return (x - np.floor(x)) == F32(0.5)


def round_u8(x):
    """saturate_cast<uchar>(float): cvRound (nearest, ties to even), then the clamp."""
    assert x.dtype == F32
    return np.clip(np.rint(x), 0, 255).astype(np.uint8)


def clahe(plane, clip_limit: float, tiles=(8, 8)) -> Clahe:
    src = np.ascontiguousarray(plane)
    assert src.dtype == np.uint8 and src.ndim == 2 and src.size
    H, W = src.shape
    tx, ty = int(tiles[0]), int(tiles[1])
    g = geometry(H, W, tiles, clip_limit)
    hist = tile_histograms(src, tiles)
    info = dict(g, hist_max=int(hist.max()), cut=np.zeros(tx * ty, np.int64))
    if g["limit"] > 0:
        hist, info["cut"] = redistribute(hist, g["limit"])
    assert (hist.sum(axis=1) == g["area"]).all()
    lut_scale = F32(255) / F32(g["area"])
    scaled = np.cumsum(hist, axis=1).astype(F32) * lut_scale
    luts = round_u8(scaled).reshape(ty, tx, 256)
    # ties that rounding half UP would send elsewhere: those above an even integer (below 255)
    info["lut_ties_up"] = int(np.count_nonzero(half(scaled) & (np.floor(scaled) % 2 == 0) & (scaled < 255)))

    def axis(n, size, count):
        f = np.arange(n).astype(F32) * (F32(1) / F32(size)) - F32(0.5)
        i1 = np.floor(f).astype(np.int64)
        a = f - i1.astype(F32)
        return np.maximum(i1, 0), np.minimum(i1 + 1, count - 1), a, F32(1) - a

    ty1, ty2, ya, ya1 = axis(H, g["th"], ty)
    tx1, tx2, xa, xa1 = axis(W, g["tw"], tx)
    lf = luts.astype(F32)
    l11, l12 = lf[ty1[:, None], tx1[None, :], src], lf[ty1[:, None], tx2[None, :], src]
    l21, l22 = lf[ty2[:, None], tx1[None, :], src], lf[ty2[:, None], tx2[None, :], src]
    xa, xa1, ya, ya1 = xa[None, :], xa1[None, :], ya[:, None], ya1[:, None]
    res = (l11 * xa1 + l12 * xa) * ya1 + (l21 * xa1 + l22 * xa) * ya
    assert res.dtype == F32
    return Clahe(round_u8(res), luts, int(np.count_nonzero(half(scaled))), int(np.count_nonzero(half(res))), info)
