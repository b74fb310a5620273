"""The contract of ``uwie_fusion_u8`` (include/uwie.h) in NumPy, written from the comment above the entry point: the multi-scale
fusion of Ancuti et al. 2018 ("Color Balance and Fusion for Underwater Image Enhancement") for a balanced u8 frame, with one
weight pyramid and one pyramid of the difference of the two inputs.  Integer steps are exact int64 arithmetic; every other
step is one NumPy array operation in the contract's order (NumPy never fuses a multiplication with an addition), so a device
that does the same IEEE float64 operations gives the same bits.

``dtype=np.float32`` evaluates the same formula with every non-integer step in float32: what a kernel that worked in float32
would give.  The case table uses it to find a frame on which that changes a byte."""
import numpy as np

from oracle.uwie_oracle import cv_rgb2gray_u8


def table(gamma):
    """G[v] = rint(255 * (v / 255) ** gamma), 256 bytes (always float64: the table is built on the host)."""
    v = np.arange(256, dtype=np.float64)
    return np.rint(np.float64(255) * (v / np.float64(255)) ** np.float64(gamma)).astype(np.uint8)


def shifted(p, d, axis):
    """p[j + d] along ``axis`` with the index clamped to the plane."""
    n = p.shape[axis]
    return np.take(p, np.clip(np.arange(n) + d, 0, n - 1), axis=axis)


def taps(p, axis):
    """The 5-tap rule T along ``axis``: ((v[j-2] + v[j+2]) + 4 (v[j-1] + v[j+1])) + 6 v[j]."""
    return ((shifted(p, -2, axis) + shifted(p, 2, axis)) + 4 * (shifted(p, -1, axis) + shifted(p, 1, axis))) + 6 * p


def blur(p):
    """B(p): T along the row, then T down the column; p [H, W] or [H, W, C]."""
    return taps(taps(p, 1), 0)


def inputs(x, gamma):
    """(I1, I2) of a u8 frame, both uint8 [H, W, 3]."""
    x = np.asarray(x)
    assert x.dtype == np.uint8 and x.ndim == 3 and x.shape[2] == 3
    xi = x.astype(np.int64)
    in2 = np.clip((512 * xi - blur(xi) + 128) >> 8, 0, 255).astype(np.uint8)
    return table(gamma)[x], in2


def weight(img, gray_shift=15, dtype=np.float64):
    """W_k of one input, [H, W] of ``dtype``."""
    F = dtype
    i = img.astype(np.int64)
    Y = cv_rgb2gray_u8(img, gray_shift).astype(np.int64)
    lap = np.abs(4 * Y - shifted(Y, -1, 0) - shifted(Y, 1, 0) - shifted(Y, -1, 1) - shifted(Y, 1, 1))
    wl = lap.astype(F) / F(255)
    n = F(img.shape[0] * img.shape[1])
    B = blur(i)
    sal = np.zeros(img.shape[:2], F)
    for c in range(3):
        mu = F(int(i[..., c].sum())) / n
        d = mu - B[..., c].astype(F) * F(2.0 ** -8)
        sal = sal + d * d
    ws = sal / F(65025)
    q = ((i - Y[..., None]) ** 2).sum(-1)
    wsat = np.sqrt(q.astype(F) / F(3)) / F(255)
    return (wl + ws) + wsat


def normalised(in1, in2, gray_shift=15, dtype=np.float64):
    """Wn, the normalised weight of input 1."""
    a = weight(in1, gray_shift, dtype) + dtype(0.1)
    return a / (a + (weight(in2, gray_shift, dtype) + dtype(0.1)))


def reduce(p):
    """T along the row, T down the column, times 2^-8, at the even indices: [h, w, ...] -> [ceil(h/2), ceil(w/2), ...]."""
    return (taps(taps(p, 1), 0) * p.dtype.type(2.0 ** -8))[::2, ::2]


def expand_axis(p, size, axis):
    i = np.arange(size)
    k = i // 2
    n = p.shape[axis]
    at = lambda j: np.take(p, np.clip(j, 0, n - 1), axis=axis)  # noqa: E731
    F = p.dtype.type
    even = ((at(k - 1) + at(k + 1)) + 6 * at(k)) * F(0.125)
    odd = (at(k) + at(k + 1)) * F(0.5)
    shape = [1] * p.ndim
    shape[axis] = size
    return np.where((i % 2 == 0).reshape(shape), even, odd)


def expand(p, h, w):
    """To the finer size h x w: along the row, then down the column."""
    assert p.shape[0] == (h + 1) // 2 and p.shape[1] == (w + 1) // 2
    return expand_axis(expand_axis(p, w, 1), h, 0)


def fuse(in1, in2, wn, levels):
    """acc_0 [H, W, 3] of wn's dtype from the two inputs and the normalised weight."""
    F = wn.dtype.type
    gw = [wn[..., None]]
    gd = [(in1.astype(np.int64) - in2.astype(np.int64)).astype(F)]
    for _ in range(1, levels):
        gw.append(reduce(gw[-1]))
        gd.append(reduce(gd[-1]))
    acc = gw[-1] * gd[-1]
    for l in range(levels - 2, -1, -1):
        h, w = gd[l].shape[:2]
        acc = gw[l] * (gd[l] - expand(gd[l + 1], h, w)) + expand(acc, h, w)
    return acc


def fusion(x, gamma=2.2, levels=1, gray_shift=15, dtype=np.float64):
    """(out, in1, in2, Wn) of one frame: uint8, uint8, uint8, ``dtype``."""
    in1, in2 = inputs(x, gamma)
    wn = normalised(in1, in2, gray_shift, dtype)
    acc = fuse(in1, in2, wn, levels)
    v = in2.astype(dtype) + acc
    out = np.rint(np.minimum(np.maximum(v, dtype(0)), dtype(255))).astype(np.uint8)
    return out, in1, in2, wn


def default_levels(H, W):
    """What ``levels=None`` means in ``uw.fusion``: min(6, max(1, floor(log2(min(H, W))) - 2))."""
    return min(6, max(1, int(min(H, W)).bit_length() - 1 - 2))
