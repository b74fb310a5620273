"""The contract of ``uwie_underwater_scores_u8`` (include/uwie.h) in NumPy float64, written from the definition: UCIQE and
UIQM in their fixed form (8 x 8 blocks, plain arithmetic).  Order and trimmed statistics come from sorting, the blocks from
sliding_window_view -- nothing here is shaped like the kernels (no histograms, no tiles).  The 8-bit LAB and
gray planes are the oracle's restatement of OpenCV (oracle/cvref.c)."""
import numpy as np

from oracle import uwie_oracle as orc

NAMES = ("sigma_c", "con_l", "mu_s", "uciqe", "uicm", "uism", "uiconm", "uiqm")


def lab_planes(frame):
    lab = orc.cv_rgb2lab_u8(frame).astype(np.int64)
    return lab[..., 0], lab[..., 1] - 128, lab[..., 2] - 128


def uciqe_parts(frame):
    L, da, db = lab_planes(frame)
    n = L.size
    root = np.sqrt((da * da + db * db).astype(np.float64))
    sigma_c = float(np.std(root / 255.0))
    srt = np.sort(L.reshape(-1))
    con_l = float(srt[min(99 * n // 100, n - 1)] - srt[n // 100]) / 255.0
    sat = np.zeros(L.shape, np.float64)
    np.divide(root, L, out=sat, where=L > 0)
    mu_s = float(sat.mean())
    return sigma_c, con_l, mu_s


def trimmed(plane):
    """(mean, population variance) of the plane's values without the n // 10 smallest and the n // 10 largest."""
    v = np.sort(plane.reshape(-1).astype(np.int64))
    t = v.size // 10
    kept = v[t:v.size - t].astype(np.float64)
    mu = float(kept.mean())
    return mu, float(np.mean((kept - mu) ** 2))


def uicm(frame):
    f = frame.astype(np.int64)
    mu_rg, var_rg = trimmed(f[..., 0] - f[..., 1])
    mu_yb2, var_yb2 = trimmed(f[..., 0] + f[..., 1] - 2 * f[..., 2])
    mu_yb, var_yb = mu_yb2 / 2.0, var_yb2 / 4.0
    return -0.0268 * np.sqrt(mu_rg * mu_rg + mu_yb * mu_yb) + 0.1586 * np.sqrt(var_rg + var_yb)


def sobel_q(channel):
    """q = min(gx^2 + gy^2, 65025) * c^2 as exact integers; BORDER_REFLECT_101 (np.pad's 'reflect'; a side of one pixel has
    nothing to reflect and repeats itself, like cv::borderInterpolate)."""
    c = channel.astype(np.int64)
    p = c
    for axis in (0, 1):
        width = [(0, 0), (0, 0)]
        width[axis] = (1, 1)
        p = np.pad(p, width, mode="reflect" if c.shape[axis] > 1 else "edge")
    H, W = c.shape
    w = lambda dy, dx: p[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]  # noqa: E731
    gx = (w(-1, 1) + 2 * w(0, 1) + w(1, 1)) - (w(-1, -1) + 2 * w(0, -1) + w(1, -1))
    gy = (w(1, -1) + 2 * w(1, 0) + w(1, 1)) - (w(-1, -1) + 2 * w(-1, 0) + w(-1, 1))
    return np.minimum(gx * gx + gy * gy, 65025) * c * c


def blocks(plane):
    """The full 8 x 8 blocks from the top left corner as [blocks, 64]; remainder rows and columns dropped."""
    if plane.shape[0] < 8 or plane.shape[1] < 8:
        return np.empty((0, 64), plane.dtype)
    win = np.lib.stride_tricks.sliding_window_view(plane, (8, 8))[::8, ::8]  # windows that start at multiples of 8 and fit
    return win.reshape(-1, 64)


def eme(channel):
    q = blocks(sobel_q(channel))
    if q.shape[0] == 0:
        return 0.0
    qmax, qmin = q.max(axis=1).astype(np.float64), q.min(axis=1).astype(np.float64)
    terms = np.zeros(q.shape[0], np.float64)
    live = qmin > 0
    terms[live] = np.log(qmax[live] / qmin[live])
    return float(np.mean(terms))


def uism(frame):
    return 0.299 * eme(frame[..., 0]) + 0.587 * eme(frame[..., 1]) + 0.114 * eme(frame[..., 2])


def uiconm(frame, gray_shift=15):
    g = blocks(orc.cv_rgb2gray_u8(frame, gray_shift).astype(np.int64))
    if g.shape[0] == 0:
        return 0.0
    M, m = g.max(axis=1).astype(np.float64), g.min(axis=1).astype(np.float64)
    terms = np.zeros(g.shape[0], np.float64)
    live = M > m
    r = (M[live] - m[live]) / (M[live] + m[live])
    terms[live] = r * np.log(r)
    return -float(np.mean(terms))


def scores(frame, gray_shift=15):
    """The eight numbers of one u8 frame [H, W, 3], in NAMES order."""
    frame = np.ascontiguousarray(frame, dtype=np.uint8)
    assert frame.ndim == 3 and frame.shape[2] == 3
    sigma_c, con_l, mu_s = uciqe_parts(frame)
    cm, sm, conm = uicm(frame), uism(frame), uiconm(frame, gray_shift)
    return np.array([sigma_c, con_l, mu_s, 0.4680 * sigma_c + 0.2745 * con_l + 0.2576 * mu_s, cm, sm, conm,
                     0.0282 * cm + 0.2953 * sm + 3.5753 * conm], np.float64)
