"""The frames that hold uwie_feature_extractor_u8's row to a float64 statement of the same definitions (features79_ref.features79_f64),
its own RGB -> LAB / RGB -> HSV to the oracle on all 2^24 colours, and its DCT to one output and one input at a time; and
the checkers both sides use.  NumPy, SciPy and the oracle only, seeded, no GPU.  tests/test_fx_cases.py asserts on the CPU
that the cases resolve what they claim to resolve; tests/test_gpu_fx_pin.py compares the device with them.

  A  row_frames / sparse_frames / batch3 / float_image    every index outside 57-61 at 1e-9 relative + 1e-12
  B  slabs(shuffled)                                       the colour block of 2 x 256 frames of 256 x 256: every colour once
  C  dct_batches                                           basis frames (one coefficient) and impulse frames (one input), by shape
"""
from __future__ import annotations

import os
from typing import NamedTuple

import numpy as np
from scipy import fft as sfft

import colour_cases as cc
import features79_ref as R
from oracle import uwie_oracle as orc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "features79.npz")

RTOL, ATOL = 1e-9, 1e-12  # "a float64 evaluation of the same definition" (test_gpu_quality et al.) + the floor against SciPy
DCT = tuple(range(57, 62))
COLOUR_BLOCK = tuple(range(35)) + (76, 77)  # L a b H S V, cast factor, R G B, and the quality block's saturation


def layout(n):
    """positions in the 79-value layout of an n-value row (74: the DCT block is absent)."""
    return np.arange(79) if n == 79 else np.r_[np.arange(57), np.arange(62, 79)]


def tol(want):
    return RTOL * np.abs(want) + ATOL


def row_failures(got, want, indices=None, tag=""):
    """The compared indices (layout numbers; default: all but the DCT block) at which got is not want to RTOL, ATOL; NaN must
    meet NaN.  Also the largest distance in tolerance units."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    bad, worst = [], 0.0
    for pos, i in enumerate(layout(got.size)):
        if i in DCT or (indices is not None and i not in indices):
            continue
        g, w = got[pos], want[pos]
        if np.isnan(w) or np.isnan(g):
            if np.isnan(w) != np.isnan(g):
                bad.append(f"{tag} index {i}: got {g!r} want {w!r}")
            continue
        u = abs(g - w) / tol(w)
        worst = max(worst, u)
        if u > 1.0:
            bad.append(f"{tag} index {i}: got {g!r} want {w!r} ({u:.3g} tolerances)")
    return bad, worst


# the bounds tests/test_gpu_feature_extractor.py holds the device to against the float32 reference, stated
# here so that the CPU tests need no GPU test module: exact, GLCM, DCT, SciPy's float32 moments, the rest
F32_EXACT = set(range(35, 45)) | {65, 66, 67, 68, 70, 72, 73, 74, 75, 25, 26, 29, 30, 33, 34}
F32_GLCM, F32_MOMENTS = set(range(45, 57)), {2, 3, 6, 7, 10, 11}


def assert_row_f32(got, want, tag=""):
    """got is want to the old float32-reference bounds."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), (tag, np.flatnonzero(np.isnan(got) != nan))
    bad = []
    for pos, i in enumerate(layout(got.size)):
        if nan[pos]:
            continue
        g, w = got[pos], want[pos]
        if i in F32_EXACT:
            bound = 1e-12 * abs(w)
        elif i in F32_GLCM:
            bound = 1e-12 * abs(w) + 1e-13
        elif i in DCT:
            bound = 2e-5 * abs(w) + 1e-9
        else:
            bound = 2e-5 * abs(w) + (1e-5 if i in F32_MOMENTS else 1e-6)
        if not abs(g - w) <= bound:
            bad.append(f"index {i} got {g!r} want {w!r}")
    assert not bad, f"{tag}: " + "; ".join(bad)


# ------------------------------------------------------------------------------------------------------------- part A
def golden_frames():
    with np.load(GOLDEN, allow_pickle=False) as z:
        return [(k[6:], z[k]) for k in z.files if k.startswith("frame_")]


def row_frames():
    """(tag, u8 frame): the golden shapes, R.frame of all four kinds, and the two smallest frames that send k_fx_maps /
    k_fx_stencil round their grid-stride loop a second time (1024 blocks x 256 = 262 144 pixels)."""
    out = golden_frames()
    out += [(kind, R.frame(kind, 64, 96, seed=11 + i)) for i, kind in enumerate(("underwater", "noise", "hazy", "gray"))]
    out += [("underwater 512x514", R.frame("underwater", 512, 514, seed=5)), ("noise 1026x256", R.frame("noise", 1026, 256, seed=6))]
    return out


def batch3():
    """three different frames of one shape: the per-frame offsets of isum, gmax, lbp and mpart."""
    return np.stack([R.frame(kind, 70, 54, seed=21 + i) for i, kind in enumerate(("noise", "underwater", "hazy"))])


def float_image():
    """a float32 image that is not u8 / 255 data (color_correction's attenuation): the has_f32 sums and the min / max keys."""
    img = R.frame("underwater", 64, 96, seed=31).astype(np.float32) / np.float32(255.0)
    img[:, :, 2] *= np.float32(0.85)
    return img


SPARSE_SHAPE = (12, 26)  # 312 pixels: not a multiple of 256, raster pixels 255 / 256 / 257 are (9, 21..23), both dimensions even
SPARSE_FLAT = (37, 140, 201)
SPARSE_RAISED = (97, 180, 231)


def sparse_positions():
    H, W = SPARSE_SHAPE
    pos = {"corner": [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)],
           "border": [(0, W // 2), (H - 1, W // 2), (H // 2, 0), (H // 2, W - 1)],
           "one in": [(1, W // 2), (H - 2, W // 2), (H // 2, 1), (H // 2, W - 2), (1, 1), (H - 2, W - 2)],
           "seam": [divmod(p, W) for p in (255, 256, 257)],
           "last": [divmod(H * W - 1, W)]}
    return [(f"{k} {p}", p) for k, v in pos.items() for p in v]


def sparse_frames():
    """(tags, [B, H, W, 3]): a flat frame with one pixel raised, at each place a 3 x 3 stencil or a block seam can go wrong."""
    H, W = SPARSE_SHAPE
    tags, frames = [], []
    for tag, (y, x) in sparse_positions():
        f = np.empty((H, W, 3), np.uint8)
        f[:] = SPARSE_FLAT
        f[y, x] = SPARSE_RAISED
        tags.append(tag)
        frames.append(f)
    return tags, np.stack(frames)


def planes(frame):
    """The element planes the colour block and the quality block's saturation read: integer LAB, HSV, the float32 image."""
    x = np.asarray(frame)
    if x.dtype == np.uint8:
        u8, img = x, x.astype(np.float32) / np.float32(255.0)
    else:
        img = np.asarray(x, np.float32)
        u8 = (img * 255).astype(np.uint8)
    return orc.cv_rgb2lab_u8(u8).astype(np.int64), orc.cv_rgb2hsv_u8(u8).astype(np.int64), img


def colour_block(lab, hsv, img):
    """indices COLOUR_BLOCK, from planes."""
    sm, ss = R.mean_std_f64(hsv[:, :, 1].astype(np.float32) / np.float32(255.0))
    return np.r_[R.color_f64(lab, hsv, img), sm, ss]


def histogram_moves(lab, hsv, img, rng):
    """Nine plane triples, each with one element of one of L, a, b, H, S, V, R, G, B moved to the neighbouring byte: what one
    count in the wrong bin of that histogram is."""
    H, W = lab.shape[:2]
    for which in range(9):
        y, x = int(rng.integers(H)), int(rng.integers(W))
        l2, h2, i2 = lab, hsv, img
        if which < 3:
            l2 = lab.copy()
            l2[y, x, which] += 1 if l2[y, x, which] < 255 else -1
        elif which < 6:
            h2 = hsv.copy()
            h2[y, x, which - 3] += 1 if h2[y, x, which - 3] < (179 if which == 3 else 255) else -1
        else:
            i2 = img.copy()
            b = int(np.rint(np.float64(img[y, x, which - 6]) * 255.0))
            i2[y, x, which - 6] = np.float32(b + (1 if b < 255 else -1)) / np.float32(255.0)
        yield "LabHSVRGB"[which], l2, h2, i2


def moved(a, b):
    """The largest move between two value vectors in tolerance units of the first (NaN against NaN is no move)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    with np.errstate(invalid="ignore"):
        u = np.abs(a - b) / tol(a)
    return float(np.nanmax(np.where(np.isnan(a) | np.isnan(b), 0.0, u)))


# ------------------------------------------------------------------------------------------------------------- part B
def slabs(shuffled: bool):
    """[256, 256, 256, 3]: frame r holds every colour with red byte r, G down and B across; or the same 2^24 colours under a
    seeded permutation, cut into 256 frames (a colour's neighbours, lane and block change)."""
    if not shuffled:
        return cc.cube_pixels().reshape(256, 256, 256, 3)
    return cc.shuffled(seed=9)[0].reshape(256, 256, 256, 3)


def hsv_numpy(u8, hrange=180, sat_scale=255, half=1 << 11):
    """cvtColor(u8, RGB2HSV) restated in NumPy with its constants as arguments (the mutation check turns one of them)."""
    p = np.asarray(u8).reshape(-1, 3).astype(np.int64)
    r, g, b = p[:, 0], p[:, 1], p[:, 2]
    i = np.arange(1, 256, dtype=np.float64)
    sdiv = np.r_[0, np.rint((sat_scale << 12) / i)].astype(np.int64)
    hdiv = np.r_[0, np.rint((hrange << 12) / (6.0 * i))].astype(np.int64)
    v, vmin = p.max(axis=1), p.min(axis=1)
    diff = v - vmin
    s = (diff * sdiv[v] + half) >> 12
    h = np.where(v == r, g - b, np.where(v == g, b - r + 2 * diff, r - g + 4 * diff))
    h = (h * hdiv[diff] + half) >> 12
    h = h + np.where(h < 0, hrange, 0)
    return np.stack([h, s, v], axis=1).reshape(np.asarray(u8).shape)


# ------------------------------------------------------------------------------------------------------------- part C
DCT_LENGTHS = (2, 4, 6, 126, 128, 130, 254, 256, 258)
DCT_SQUARES = ((130, 130), (258, 66), (66, 258))
DCT_PICKS = (0, 1, 31, 32, 33, 63, 64, 65, 127, 128, 129)
DCT_AMPLITUDE = 127  # the largest the bytes hold: the peak stands furthest above the quantisation noise
IMPULSE_SHAPES = ((130, 66), (66, 130), (258, 6), (2, 130), (1, 130), (130, 1))


class DctCase(NamedTuple):
    kind: str   # "basis", "impulse" or "mirror"
    a: int      # basis: k; impulse / mirror: y
    b: int      # basis: c; impulse / mirror: x
    axis: int   # mirror: the axis the partner is mirrored along, else -1


def basis_frame(H, W, k, c, A=DCT_AMPLITUDE):
    y, x = np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64)
    g = 128.0 + A * np.outer(np.cos(np.pi * k * (2 * y + 1) / (2 * H)), np.cos(np.pi * c * (2 * x + 1) / (2 * W)))
    return np.rint(g).astype(np.uint8)


def impulse_positions(N):
    K = N // 2
    return sorted({p for p in (0, 1, K - 1, K, N - 2, N - 1, 63, 64) if 0 <= p < N})


def dct_batches():
    """{(H, W): (cases, [B, H, W] u8 gray planes)}: one device call per shape."""
    out = {}

    def add(shape, case, g):
        cases, frames = out.setdefault(shape, ([], []))
        cases.append(case)
        frames.append(g)

    for N in DCT_LENGTHS:
        for k in range(N):
            for o in (0, 1, 5):
                add((N, 6), DctCase("basis", k, o, -1), basis_frame(N, 6, k, o))
                add((6, N), DctCase("basis", o, k, -1), basis_frame(6, N, o, k))
    for H, W in DCT_SQUARES:
        for k in DCT_PICKS:
            for c in DCT_PICKS:
                if k < H and c < W:
                    add((H, W), DctCase("basis", k, c, -1), basis_frame(H, W, k, c))
    for H, W in IMPULSE_SHAPES:
        ys, xs = impulse_positions(H), impulse_positions(W)
        for y in ys:
            for x in xs:
                g = np.zeros((H, W), np.uint8)
                g[y, x] = 255
                add((H, W), DctCase("impulse", y, x, -1), g)
        for axis, ps in ((0, ys), (1, xs)):
            if (H, W)[axis] == 1:
                continue
            other = (xs, ys)[axis][min(1, len((xs, ys)[axis]) - 1)]
            for p in ps:
                g = np.zeros((H, W), np.uint8)
                y, x = (p, other) if axis == 0 else (other, p)
                my, mx = (H - 1 - p, other) if axis == 0 else (other, W - 1 - p)
                g[y, x] = 255
                g[my, mx] = 100
                add((H, W), DctCase("mirror", y, x, axis), g)
    return {s: (c, np.stack(f)) for s, (c, f) in out.items()}


def cos_matrix(N, dtype=np.float64):
    """the orthonormal DCT-II matrix C[k, n] = s_k cos(pi k (2n + 1) / 2N)."""
    k, n = np.arange(N, dtype=np.float64)[:, None], np.arange(N, dtype=np.float64)[None, :]
    C = np.cos(np.pi * k * (2 * n + 1) / (2 * N)) * np.sqrt(2.0 / N)
    C[0] = np.sqrt(1.0 / N)
    return C.astype(dtype)


def dct_planes(frames):
    """[B, H, W] float64: dct2's values (the float64 transform, rounded to float32 as cv2.dct's output is)."""
    d = sfft.dctn(np.asarray(frames, np.float64), type=2, norm="ortho", axes=(1, 2))
    return d.astype(np.float32).astype(np.float64)


def dct_planes_f32(frames):
    """The same transform as two NumPy float32 products with float32 cosine matrices: a clean float32 evaluation.  einsum's
    own loops, not matmul: which BLAS a machine has, and with how many threads, must not decide a tolerance."""
    g = np.asarray(frames, np.float32)
    H, W = g.shape[1:]
    z = np.einsum("bhn,wn->bhw", g, cos_matrix(W, np.float32))
    return np.einsum("kh,bhw->bkw", cos_matrix(H, np.float32), z).astype(np.float64)


DCT_RTOL, DCT_FLOOR, DCT_MARGIN = 2e-5, 1e-9, 4.0  # DESIGN section 9 (f32 MFMA); the margin over a restatement's own distance


def dct_reference(frames):
    """want [B, 5], tolerance [B, 5] and where the raised floor applies [B, 5] (bool): each value's tolerance is
    max(2e-5 |w| + 1e-9, 4 |float32 evaluation - float64|), the float32 evaluation being NumPy's, never the device's."""
    want = R.dct_values(dct_planes(frames))
    f32 = R.dct_values(dct_planes_f32(frames))
    base = DCT_RTOL * np.abs(want) + DCT_FLOOR
    lift = DCT_MARGIN * np.abs(f32 - want)
    return want, np.maximum(base, lift), lift > base


def dct_units(got, want, tolerance):
    """|got - want| in tolerance units, [B, 5]; a NaN (0 / 0 region fraction) must meet a NaN and counts as 0."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want)), np.argwhere(np.isnan(got) != np.isnan(want))[:5]
    return np.where(np.isnan(want), 0.0, np.abs(got - want) / tolerance)


def gray_rgb(planes_u8):
    """[B, H, W] gray planes as R = G = B frames."""
    return np.repeat(np.asarray(planes_u8)[..., None], 3, axis=-1)


def dct_split(frames, mutate=None):
    """The even / odd split the kernels use, stated in float64: d[k] = s_k sum_{n < K} (x_n +- x_{N-1-n}) cos(pi m / 2N), with
    m = k (2n + 1) mod 4N read from a 4N-entry table, along W and then along H.  ``mutate(axis, m, k, n)`` may return another
    table index (the mutation check: a step taken once too often)."""
    x = np.asarray(frames, np.float64)
    for axis in (2, 1):
        N = x.shape[axis]
        x = np.moveaxis(x, axis, -1)
        if N > 1:
            K = N // 2
            k, n = np.arange(N)[:, None], np.arange(K)[None, :]
            m = (k * (2 * n + 1)) % (4 * N)
            if mutate is not None:
                m = mutate(axis, m, k, n) % (4 * N)
            tab = np.cos(np.pi * np.arange(4 * N) / (2.0 * N))
            C = tab[m] * np.where(k == 0, np.sqrt(1.0 / N), np.sqrt(2.0 / N))
            lo, hi = x[..., :K], x[..., ::-1][..., :K]
            even, odd = (lo + hi) @ C.T, (lo - hi) @ C.T
            x = np.where(np.arange(N) % 2 == 0, even, odd)
        x = np.moveaxis(x, -1, axis)
    return x
