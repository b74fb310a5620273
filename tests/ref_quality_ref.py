"""The contract of ``uwie_reference_scores_u8`` (include/uwie.h) in NumPy float64, written from the definition: mean absolute
error, mean squared error, PSNR, and SSIM with the 11 x 11 Gaussian window (sigma 1.5) over the windows that lie wholly inside
the frame.  Whole-plane array arithmetic in the header's order of summation (along the row first, the taps in index order,
then down the column); nothing here is shaped like the kernels (no tiles, no bands).  The gray plane is the oracle's
restatement of OpenCV (oracle/cvref.c)."""
import numpy as np

from oracle import uwie_oracle as orc

NAMES = ("mae", "mse", "psnr", "ssim_y", "ssim_r", "ssim_g", "ssim_b", "ssim_rgb")
C1, C2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2


def taps():
    """The 1-D window: exp(-k^2 / 4.5), k = -5 .. 5, divided by the sum taken in index order."""
    e = [float(np.exp(-(k * k) / 4.5)) for k in range(-5, 6)]
    total = 0.0
    for v in e:
        total += v
    return np.array([v / total for v in e], np.float64)


def window_sum(v):
    """The valid 11 x 11 window sums of a float64 plane [H, W] -> [H - 10, W - 10]: along the row first, then down the column,
    taps added in index order."""
    w = taps()
    H, W = v.shape
    rows = w[0] * v[:, 0:W - 10]
    for k in range(1, 11):
        rows = rows + w[k] * v[:, k:W - 10 + k]
    out = w[0] * rows[0:H - 10]
    for k in range(1, 11):
        out = out + w[k] * rows[k:H - 10 + k]
    return out


def ssim_map(px, py):
    """s at every map point of two byte planes [H, W] (H, W >= 11) -> float64 [H - 10, W - 10]."""
    x, y = px.astype(np.float64), py.astype(np.float64)
    mux, muy = window_sum(x), window_sum(y)
    sxx, syy, sxy = window_sum(x * x), window_sum(y * y), window_sum(x * y)
    vx, vy, cov = sxx - mux * mux, syy - muy * muy, sxy - mux * muy
    return ((2 * mux * muy + C1) * (2 * cov + C2)) / ((mux * mux + muy * muy + C1) * (vx + vy + C2))


def ssim(px, py, strip=96):
    """The mean of ssim_map, NaN without a window.  The map is built in strips of rows (every point depends on its own window
    only, so the strips' values are the whole map's, bit for bit): the planes of a strip stay in the cache."""
    H, W = px.shape
    if H < 11 or W < 11:
        return float("nan")
    parts = [ssim_map(px[a:min(a + strip, H - 10) + 10], py[a:min(a + strip, H - 10) + 10]) for a in range(0, H - 10, strip)]
    return float(np.concatenate(parts, axis=0).mean())


def channel_ssims(x, y):
    return [ssim(x[..., c], y[..., c]) for c in range(3)]


def scores(x, y, gray_shift=15, channels=None):
    """The eight numbers of a result x against a reference y, u8 [H, W, 3] each, in NAMES order.  channels: the three
    channel SSIMs if the caller has them already (they do not depend on gray_shift)."""
    x, y = np.ascontiguousarray(x, dtype=np.uint8), np.ascontiguousarray(y, dtype=np.uint8)
    assert x.ndim == 3 and x.shape[2] == 3 and x.shape == y.shape
    d = x.astype(np.int64) - y.astype(np.int64)
    n3 = d.size
    sad, ssd = int(np.abs(d).sum()), int((d * d).sum())
    mae, mse = sad / n3, ssd / n3  # Python's int / int is the correctly rounded quotient
    psnr = float("inf") if ssd == 0 else 10.0 * float(np.log10(65025.0 / mse))
    sy = ssim(orc.cv_rgb2gray_u8(x, gray_shift), orc.cv_rgb2gray_u8(y, gray_shift))
    sr, sg, sb = channel_ssims(x, y) if channels is None else channels
    return np.array([mae, mse, psnr, sy, sr, sg, sb, (sr + sg + sb) / 3], np.float64)
