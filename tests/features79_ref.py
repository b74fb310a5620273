"""NumPy / SciPy restatement of feature_extraction.FeatureExtractor (feature_extraction.py:13-295), the classifier input of
main.py:116,420 -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.

Two layers:

* primitives with the signatures the reference calls (``cv2.resize``, ``cv2.dct``, ``cv2.Sobel``, ``cv2.Laplacian``,
  ``skimage.feature.local_binary_pattern`` / ``graycomatrix`` / ``graycoprops``, ``skimage.measure.shannon_entropy``),
  restated from the libraries' published algorithms.  LAB, HSV, gray and Canny come from ``oracle.uwie_oracle``.  These
  are PARITY UNPINNED: neither OpenCV nor scikit-image is installed where this was written; each is held by known-answer
  tests (tests/test_feature_extractor_ref.py).
* ``extract_*_features`` / ``features79``: the reference's glue (float32 NumPy arithmetic, SciPy's skew / kurtosis, the
  odd-size DCT drop) on those primitives.  PINNED: tests/gen_golden_features79.py runs the real feature_extraction.py on
  the same primitives and tests/golden/features79.npz holds its rows.

``FEATURE_EXTRACTOR_KEYS`` (the package's) names the 79 entries.
"""
from __future__ import annotations

import numpy as np
from scipy import fft as sfft
from scipy import stats

from oracle import uwie_oracle as orc


class OddSizeDCT(ValueError):
    """cv2.dct's "Odd-size DCT's are not implemented" (raised for a dimension that is odd and greater than 1)."""


# --------------------------------------------------------------------------------------------------------- OpenCV
def resize128(gray_u8: np.ndarray) -> np.ndarray:
    """cv2.resize(gray_u8, (128, 128)), INTER_LINEAR on 8-bit data: OpenCV's fixed-point path (11-bit coefficients, the
    SIMD vertical pass VResizeLinearVec_32s8u), the INTER_AREA fast path for an exact 2x downscale, a copy for 128x128."""
    g = np.ascontiguousarray(gray_u8, dtype=np.uint8)
    H, W = g.shape
    if (H, W) == (128, 128):
        return g.copy()
    if (H, W) == (256, 256):  # is_area_fast with iscale_x == iscale_y == 2 -> INTER_AREA
        s = g.astype(np.int32)
        return ((s[0::2, 0::2] + s[0::2, 1::2] + s[1::2, 0::2] + s[1::2, 1::2] + 2) >> 2).astype(np.uint8)

    def taps(src: int):
        scale = 1.0 / (128.0 / src)  # resizeGeneric: scale = 1 / inv_scale
        o = np.arange(128, dtype=np.float64)
        f = ((o + 0.5) * scale - 0.5).astype(np.float32)  # (float)((dx + 0.5) * scale_x - 0.5)
        s = np.floor(f).astype(np.int64)
        f = (f - s.astype(np.float32)).astype(np.float32)
        lo = s < 0
        f[lo], s[lo] = 0, 0
        hi = s >= src - 1
        f[hi], s[hi] = 0, src - 1
        c0 = np.rint((np.float32(1) - f) * np.float32(2048)).astype(np.int64)  # saturate_cast<short>(cbuf * 2048)
        c1 = np.rint(f * np.float32(2048)).astype(np.int64)
        return s, np.minimum(s + 1, src - 1), c0, c1

    xs0, xs1, a0, a1 = taps(W)
    ys0, ys1, b0, b1 = taps(H)
    gi = g.astype(np.int64)
    D = gi[:, xs0] * a0 + gi[:, xs1] * a1  # HResizeLinear: int rows
    S0, S1 = D[ys0], D[ys1]
    v = (((S0 >> 4) * b0[:, None]) >> 16) + (((S1 >> 4) * b1[:, None]) >> 16)
    return np.clip((v + 2) >> 2, 0, 255).astype(np.uint8)


def _reflect101(i: np.ndarray, n: int) -> np.ndarray:
    if n == 1:
        return np.zeros_like(i)
    i = np.where(i < 0, -i, i)
    return np.where(i >= n, 2 * (n - 1) - i, i)


def _win(a: np.ndarray, dy: int, dx: int) -> np.ndarray:
    H, W = a.shape
    ys = _reflect101(np.arange(H) + dy, H)
    xs = _reflect101(np.arange(W) + dx, W)
    return a[ys][:, xs]


def sobel_int(gray_u8: np.ndarray):
    """cv2.Sobel(gray, ksize=3) x and y derivatives of the byte plane as exact integers (BORDER_REFLECT_101)."""
    g = np.asarray(gray_u8, dtype=np.int64)
    w = {(dy, dx): _win(g, dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1)}
    gx = (w[-1, 1] - w[-1, -1]) + 2 * (w[0, 1] - w[0, -1]) + (w[1, 1] - w[1, -1])
    gy = (w[1, -1] - w[-1, -1]) + 2 * (w[1, 0] - w[-1, 0]) + (w[1, 1] - w[-1, 1])
    return gx, gy


def sobel_f32(gray_f32: np.ndarray, dx: int, dy: int) -> np.ndarray:
    """cv2.Sobel(gray/255 float32, CV_32F, dx, dy, ksize=3): the integer derivative of the bytes over 255, in float32."""
    g = np.asarray(gray_f32, dtype=np.float32)
    u8 = np.rint(g.astype(np.float64) * 255.0).astype(np.uint8)
    gx, gy = sobel_int(u8)
    return (gx if dx else gy).astype(np.float64).__truediv__(255.0).astype(np.float32)


def laplacian3(gray_u8: np.ndarray) -> np.ndarray:
    """cv2.Laplacian(gray_u8, CV_64F, ksize=3): aperture [[2,0,2],[0,-8,0],[2,0,2]], BORDER_REFLECT_101."""
    g = np.asarray(gray_u8, dtype=np.int64)
    lap = 2 * (_win(g, -1, -1) + _win(g, -1, 1) + _win(g, 1, -1) + _win(g, 1, 1)) - 8 * g
    return lap.astype(np.float64)


def dct2(gray_f32: np.ndarray) -> np.ndarray:
    """cv2.dct of a float32 plane: orthonormal 2-D DCT-II; raises OddSizeDCT like OpenCV for an odd dimension > 1."""
    a = np.asarray(gray_f32, dtype=np.float32)
    if any(n > 1 and n % 2 for n in a.shape):
        raise OddSizeDCT("Odd-size DCT's are not implemented")
    return sfft.dctn(a.astype(np.float64), type=2, norm="ortho").astype(np.float32)


def canny(gray_u8, low, high):
    return orc.cv_canny_u8(gray_u8, low, high)


# ----------------------------------------------------------------------------------------------------- scikit-image
_LBP_R = np.round(-np.sin(2 * np.pi * np.arange(8, dtype=np.float64) / 8), 5)
_LBP_C = np.round(np.cos(2 * np.pi * np.arange(8, dtype=np.float64) / 8), 5)


def local_binary_pattern_uniform(gray_u8: np.ndarray) -> np.ndarray:
    """skimage.feature.local_binary_pattern(image, 8, 1, 'uniform'): 8 bilinear samples at offsets round(-sin, 5),
    round(cos, 5) in float64 (constant 0 outside), bit = sample - centre >= 0, the count of set bits when the pattern has
    at most 2 transitions among p = 0..7, else 9.  Vectorised in the library's operation order (NumPy does not fuse)."""
    img = np.asarray(gray_u8, dtype=np.float64)
    H, W = img.shape
    pad = np.zeros((H + 2, W + 2))
    pad[1:-1, 1:-1] = img

    def px(rr, cc):  # constant-0 border: rr, cc in -1 .. H / W
        return pad[rr + 1, cc + 1]

    r = np.arange(H, dtype=np.float64)[:, None] + np.zeros((1, W))
    c = np.zeros((H, 1)) + np.arange(W, dtype=np.float64)[None, :]
    bits = []
    for i in range(8):
        rf, cf = r + _LBP_R[i], c + _LBP_C[i]
        minr, minc = np.floor(rf), np.floor(cf)
        maxr, maxc = np.ceil(rf), np.ceil(cf)
        dr, dc = rf - minr, cf - minc
        ir0, ir1, ic0, ic1 = (minr.astype(np.int64), maxr.astype(np.int64), minc.astype(np.int64), maxc.astype(np.int64))
        tl, tr, bl, br = px(ir0, ic0), px(ir0, ic1), px(ir1, ic0), px(ir1, ic1)
        top = (1 - dc) * tl + dc * tr
        bottom = (1 - dc) * bl + dc * br
        v = (1 - dr) * top + dr * bottom
        bits.append((v - img >= 0).astype(np.int64))
    bits = np.stack(bits)
    changes = np.sum(bits[:-1] != bits[1:], axis=0)
    return np.where(changes <= 2, bits.sum(axis=0), 9).astype(np.float64)


GLCM_OFFSETS = ((0, 1), (1, 1), (1, 0), (1, -1))  # angles 0, pi/4, pi/2, 3pi/4 at distance 1: (round(sin), round(cos))


def graycomatrix(image, distances, angles, levels=256, symmetric=False, normed=False):
    """skimage.feature.graycomatrix for uint8 images: counts[i, j, d, a] of (image[r, c], image[r + dr, c + dc])."""
    img = np.asarray(image)
    H, W = img.shape
    out = np.zeros((levels, levels, len(distances), len(angles)), np.uint32)
    for di, d in enumerate(distances):
        for ai, ang in enumerate(angles):
            orow, ocol = int(np.round(np.sin(ang) * d)), int(np.round(np.cos(ang) * d))
            r0, r1 = max(0, -orow), min(H, H - orow)
            c0, c1 = max(0, -ocol), min(W, W - ocol)
            if r1 <= r0 or c1 <= c0:
                continue
            i = img[r0:r1, c0:c1].astype(np.int64)
            j = img[r0 + orow:r1 + orow, c0 + ocol:c1 + ocol].astype(np.int64)
            np.add.at(out[:, :, di, ai], (i.ravel(), j.ravel()), 1)
    if symmetric:
        out = out + np.transpose(out, (1, 0, 2, 3))
    if normed:
        out = out.astype(np.float64)
        sums = out.sum(axis=(0, 1), keepdims=True)
        sums[sums == 0] = 1
        out /= sums
    return out


def graycoprops(P, prop="contrast"):
    """skimage.feature.graycoprops: contrast, dissimilarity, homogeneity, energy, correlation, ASM of each matrix."""
    P = np.asarray(P, dtype=np.float64)
    L = P.shape[0]
    sums = P.sum(axis=(0, 1), keepdims=True)
    sums[sums == 0] = 1
    P = P / sums
    I, J = np.ogrid[0:L, 0:L]
    if prop in ("contrast", "dissimilarity", "homogeneity"):
        w = {"contrast": (I - J) ** 2, "dissimilarity": np.abs(I - J), "homogeneity": 1.0 / (1.0 + (I - J) ** 2)}[prop]
        return np.sum(P * w.reshape(L, L, 1, 1), axis=(0, 1))
    if prop == "ASM":
        return np.sum(P ** 2, axis=(0, 1))
    if prop == "energy":
        return np.sqrt(np.sum(P ** 2, axis=(0, 1)))
    if prop == "correlation":
        I4 = np.arange(L).reshape(L, 1, 1, 1)
        J4 = np.arange(L).reshape(1, L, 1, 1)
        di = I4 - np.sum(I4 * P, axis=(0, 1))
        dj = J4 - np.sum(J4 * P, axis=(0, 1))
        si = np.sqrt(np.sum(P * di ** 2, axis=(0, 1)))
        sj = np.sqrt(np.sum(P * dj ** 2, axis=(0, 1)))
        cov = np.sum(P * (di * dj), axis=(0, 1))
        out = np.ones_like(cov)
        ok = ~((si < 1e-15) | (sj < 1e-15))
        out[ok] = cov[ok] / (si[ok] * sj[ok])
        return out
    raise ValueError(prop)


def shannon_entropy(image, base=2):
    """skimage.measure.shannon_entropy: scipy.stats.entropy of the counts of the distinct values."""
    _, counts = np.unique(np.asarray(image), return_counts=True)
    return stats.entropy(counts, base=base)


# ------------------------------------------------------------------------------------------------------- the glue
def _u8(img):
    return (np.asarray(img) * 255).astype(np.uint8)


def _gray(img):
    return orc.cv_rgb2gray_u8(_u8(img))


def extract_color_features(img):
    """feature_extraction.py:17-79 (35 values)."""
    u8 = _u8(img)
    lab = orc.cv_rgb2lab_u8(u8).astype(np.float32)
    f = []
    for c in range(3):
        ch = lab[:, :, c].ravel()
        f += [np.mean(ch), np.std(ch), stats.skew(ch), stats.kurtosis(ch)]
    hsv = orc.cv_rgb2hsv_u8(u8).astype(np.float32)
    for c in range(3):
        ch = hsv[:, :, c].ravel()
        f += [np.mean(ch), np.std(ch)]
    a, b = lab[:, :, 1], lab[:, :, 2]
    ma, mb = np.mean(a), np.mean(b)
    M = np.sqrt(ma ** 2 + mb ** 2)
    D = np.sqrt(np.mean(np.abs(a - ma)) ** 2 + np.mean(np.abs(b - mb)) ** 2)
    f += [M / (D + 1e-10), M, D, ma, mb]
    img = np.asarray(img)
    for c in range(3):
        ch = img[:, :, c].ravel()
        f += [np.mean(ch), np.std(ch), np.min(ch), np.max(ch)]
    return np.array(f)


def extract_texture_features(img):
    """feature_extraction.py:81-126 (22 values)."""
    g = _gray(img)
    lbp = local_binary_pattern_uniform(g)
    hist, _ = np.histogram(lbp.ravel(), bins=10, range=(0, 10), density=True)
    f = list(hist)
    glcm = graycomatrix(resize128(g), [1], [0, np.pi / 4, np.pi / 2, 3 * np.pi / 4], levels=256, symmetric=True, normed=True)
    for prop in ("contrast", "dissimilarity", "homogeneity", "energy", "correlation", "ASM"):
        v = graycoprops(glcm, prop).ravel()
        f += [np.mean(v), np.std(v)]
    return np.array(f)


def extract_frequency_features(img):
    """feature_extraction.py:128-165 (5 values; OddSizeDCT for an odd dimension > 1)."""
    d = dct2(_gray(img).astype(np.float32))
    total = np.sum(d ** 2)
    h, w = d.shape
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.array([np.sum(d[:h // 4, :w // 4] ** 2) / total, np.sum(d[h // 4:h // 2, w // 4:w // 2] ** 2) / total,
                         np.sum(d[h // 2:, w // 2:] ** 2) / total, np.mean(np.abs(d)), np.std(np.abs(d))])


def extract_edge_features(img):
    """feature_extraction.py:167-206 (7 values)."""
    g = _gray(img)
    gx, gy = sobel_int(g)
    sx, sy = (gx / 255.0).astype(np.float32), (gy / 255.0).astype(np.float32)
    mag = np.sqrt(sx ** 2 + sy ** 2)
    edges = canny(g, 50, 150)
    lap = laplacian3(g)
    return np.array([np.mean(mag), np.std(mag), np.max(mag), np.sum(edges > 0) / edges.size, np.mean(np.abs(lap)),
                     np.std(lap), np.var(lap)])


def extract_quality_features(img):
    """feature_extraction.py:208-250 (10 values)."""
    g8 = _gray(img)
    g = g8.astype(np.float32) / 255.0
    s = orc.cv_rgb2hsv_u8(_u8(img)).astype(np.float32)[:, :, 1] / 255.0
    return np.array([np.std(g), shannon_entropy(g), np.mean(g), np.median(g), np.percentile(g, 25), np.percentile(g, 75),
                     np.max(g) - np.min(g), np.mean(s), np.std(s), np.sqrt(np.mean((g - np.mean(g)) ** 2))])


def features79(img):
    """extract_all_features (feature_extraction.py:252-295): 79 values, or 74 when the DCT is dropped."""
    parts = [extract_color_features(img), extract_texture_features(img)]
    try:
        parts.append(extract_frequency_features(img))
    except OddSizeDCT:
        pass
    parts += [extract_edge_features(img), extract_quality_features(img)]
    return np.concatenate(parts).astype(np.float64)


# ------------------------------------------------------------------------------- the same definitions in float64
# features79_f64 states what features79 states with every sum, mean, standard deviation and moment in float64, over the element
# values the reference holds: the integer LAB / HSV / gray / Sobel / Laplacian planes, float32(u8) / 255 lifted to float64 for
# the planes the reference normalises, the float32 values of a general float image.  Unchanged: the order statistics (NumPy's
# float32 'linear' rule), SciPy's NaN rule for skew / kurtosis on float32 planes (m2 <= (eps32 * mean)^2), and the DCT block,
# which takes dct2's values.
F64_GROUPS = ("color", "texture", "frequency", "edge", "quality")
_EPS32 = float(np.finfo(np.float32).eps)


def moments_f64(ch):
    """mean, std, skew, kurtosis (Fisher) of a plane in float64, with SciPy's float32 NaN rule."""
    x = np.asarray(ch, dtype=np.float64).ravel()
    m = x.mean()
    d = x - m
    d2 = d * d
    m2, m3, m4 = d2.mean(), (d2 * d).mean(), (d2 * d2).mean()
    if m2 <= (_EPS32 * m) ** 2:
        return m, np.sqrt(m2), np.nan, np.nan
    return m, np.sqrt(m2), m3 / (m2 * np.sqrt(m2)), m4 / (m2 * m2) - 3.0


def mean_std_f64(ch):
    x = np.asarray(ch, dtype=np.float64).ravel()
    m = x.mean()
    return m, np.sqrt(((x - m) ** 2).mean())


def color_f64(lab, hsv, img_f32):
    """indices 0-34 from the integer LAB / HSV planes and the float32 image."""
    lab = np.asarray(lab, dtype=np.float64)
    f = []
    for c in range(3):
        f += list(moments_f64(lab[:, :, c]))
    for c in range(3):
        f += list(mean_std_f64(hsv[:, :, c]))
    a, b = lab[:, :, 1], lab[:, :, 2]
    ma, mb = a.mean(), b.mean()
    M = np.sqrt(ma ** 2 + mb ** 2)
    D = np.sqrt(np.abs(a - ma).mean() ** 2 + np.abs(b - mb).mean() ** 2)
    f += [M / (D + 1e-10), M, D, ma, mb]
    img_f32 = np.asarray(img_f32, dtype=np.float32)
    for c in range(3):
        ch = img_f32[:, :, c]
        f += list(mean_std_f64(ch)) + [float(ch.min()), float(ch.max())]
    return np.array(f, dtype=np.float64)


def dct_values(d):
    """indices 57-61 from a coefficient plane, sums in float64."""
    d = np.asarray(d, dtype=np.float64)
    h, w = d.shape[-2:]
    e = d * d
    total = e.sum(axis=(-2, -1))
    ad = np.abs(d)
    n = float(h * w)
    ma = ad.sum(axis=(-2, -1)) / n
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.stack([e[..., :h // 4, :w // 4].sum(axis=(-2, -1)) / total,
                         e[..., h // 4:h // 2, w // 4:w // 2].sum(axis=(-2, -1)) / total,
                         e[..., h // 2:, w // 2:].sum(axis=(-2, -1)) / total, ma,
                         np.sqrt(((ad - ma[..., None, None]) ** 2).sum(axis=(-2, -1)) / n)], axis=-1)


def edge_f64(g, with_canny=True):
    gx, gy = sobel_int(g)
    mag = np.sqrt((gx * gx + gy * gy).astype(np.float64)) / 255.0
    lap = laplacian3(g)
    density = np.sum(canny(g, 50, 150) > 0) / g.size if with_canny else np.nan
    mm, ms = mean_std_f64(mag)
    lm, ls = mean_std_f64(lap)
    return np.array([mm, ms, mag.max(), density, np.abs(lap).mean(), ls, ((lap - lm) ** 2).mean()])


def quality_f64(g8, sat_u8):
    g = g8.astype(np.float32) / np.float32(255.0)
    m, s = mean_std_f64(g)
    sm, ss = mean_std_f64(sat_u8.astype(np.float32) / np.float32(255.0))
    return np.array([s, shannon_entropy(g), m, np.median(g), np.percentile(g, 25), np.percentile(g, 75),
                     np.max(g) - np.min(g), sm, ss, s], dtype=np.float64)


def features79_f64(frame, groups=F64_GROUPS, with_canny=True):
    """The row of features79 in float64.  ``frame``: a u8 frame (the float image is then float32(u8) / 255) or a float32
    image in [0, 1].  ``groups``: the blocks to evaluate, in layout order (the cube needs only colour and quality, and the
    Python LBP over it would take minutes); ``with_canny=False`` leaves index 65 NaN."""
    x = np.asarray(frame)
    if x.dtype == np.uint8:
        u8, img = x, x.astype(np.float32) / np.float32(255.0)
    else:
        img = np.asarray(x, dtype=np.float32)
        u8 = _u8(img)
    g = orc.cv_rgb2gray_u8(u8)
    hsv = orc.cv_rgb2hsv_u8(u8)
    parts = []
    for name in F64_GROUPS:
        if name not in groups:
            continue
        if name == "color":
            parts.append(color_f64(orc.cv_rgb2lab_u8(u8), hsv, img))
        elif name == "texture":
            parts.append(extract_texture_features(img).astype(np.float64))  # counts and float64 sums already
        elif name == "frequency":
            try:
                parts.append(dct_values(dct2(g.astype(np.float32))))
            except OddSizeDCT:
                pass
        elif name == "edge":
            parts.append(edge_f64(g, with_canny))
        else:
            parts.append(quality_f64(g, hsv[:, :, 1]))
    return np.concatenate(parts)


def feature_count(H: int, W: int) -> int:
    return 79 if all(n == 1 or n % 2 == 0 for n in (H, W)) else 74


# --------------------------------------------------------------------------------------------------- test frames
def frame(kind: str, H: int, W: int, seed: int = 0) -> np.ndarray:
    """Seeded uint8 test frames: 'underwater' (smooth blue-green field + noise), 'noise' (uniform bytes), 'hazy' (low
    contrast), 'gray' (R = G = B), 'const'."""
    rng = np.random.default_rng(seed)
    if kind == "noise":
        return rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    if kind == "const":
        return np.full((H, W, 3), (37, 140, 201), np.uint8)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    field = 0.5 + 0.3 * np.sin(xx / (7.0 + W / 23.0)) * np.cos(yy / (5.0 + H / 19.0))
    if kind == "gray":
        v = field + rng.normal(0, 0.05, (H, W))
        return np.clip(np.floor(255 * v), 0, 255).astype(np.uint8)[:, :, None].repeat(3, axis=2)
    tint = {"underwater": (0.35, 0.8, 0.75), "hazy": (0.7, 0.75, 0.72)}[kind]
    amp = 0.06 if kind == "hazy" else 1.0
    base = 0.55 if kind == "hazy" else 0.0
    v = (base + amp * field)[:, :, None] * np.array(tint) + rng.normal(0, 0.03, (H, W, 3))
    return np.clip(np.floor(255 * v), 0, 255).astype(np.uint8)
