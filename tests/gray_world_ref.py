"""The contract of ``uwie_gray_world_u8`` (include/uwie.h) in NumPy float64, written from the comment above the entry point:
red-channel compensation (Ancuti et al. 2018 eq. 4-5) followed by gray-world, in byte units.  Every statistic is an exact
Python integer; every float64 step is one NumPy scalar or array operation in the contract's order (NumPy never fuses a
multiplication with an addition), so a device that does the same IEEE operations gives the same bits.

``apply(..., dtype=np.float32)`` evaluates the same formula with the gains rounded to float32: what a kernel that decided
the byte in float32 would give.  The case table uses it to find frames on which that differs."""
import numpy as np

NAMES = ("mean_r", "mean_g", "mean_b", "k_r", "k_b", "m_r", "m_g", "m_b", "gray", "s_r", "s_g", "s_b")
F = np.float64


def sums(frame):
    """S_r, S_g, S_b, S_rg, S_bg as Python integers."""
    f = np.asarray(frame)
    assert f.dtype == np.uint8 and f.ndim == 3 and f.shape[2] == 3
    r, g, b = (f[..., c].astype(np.int64).reshape(-1) for c in range(3))
    return int(r.sum()), int(g.sum()), int(b.sum()), int((r * g).sum()), int((b * g).sum())


def coeffs(frame, red=1.0, blue=0.0, max_gain=0.0):
    """The twelve stats of the contract, a float64 array in ``NAMES`` order."""
    S_r, S_g, S_b, S_rg, S_bg = sums(frame)
    N = F(frame.shape[0] * frame.shape[1])
    mean_r, mean_g, mean_b = F(S_r) / N, F(S_g) / N, F(S_b) / N
    d_r, d_b = mean_g - mean_r, mean_g - mean_b
    k_r = (F(red) * (d_r if d_r > 0 else F(0))) / F(65025)
    k_b = (F(blue) * (d_b if d_b > 0 else F(0))) / F(65025)
    m_r = (F(S_r) + k_r * F(255 * S_g - S_rg)) / N
    m_g = mean_g
    m_b = (F(S_b) + k_b * F(255 * S_g - S_bg)) / N
    gray = ((m_r + m_g) + m_b) / F(3)

    def gain(m):
        s = gray / m if m > 0 else F(1)
        if max_gain > 0:
            s = min(s, F(max_gain))
        return s

    return np.array([mean_r, mean_g, mean_b, k_r, k_b, m_r, m_g, m_b, gray, gain(m_r), gain(m_g), gain(m_b)], dtype=F)


def weighted(frame, st, dtype=np.float64):
    """w_r, w_g, w_b of every pixel, [H, W, 3] of ``dtype`` (before the min and the rounding)."""
    f = np.asarray(frame)
    r, g, b = (f[..., c].astype(np.int64) for c in range(3))
    s_r, s_g, s_b = (dtype(st[NAMES.index(k)]) for k in ("s_r", "s_g", "s_b"))
    k_r, k_b = dtype(st[NAMES.index("k_r")]), dtype(st[NAMES.index("k_b")])
    c_r, c_b = s_r * k_r, s_b * k_b
    w = np.empty(f.shape, dtype)
    w[..., 0] = s_r * r.astype(dtype) + c_r * ((255 - r) * g).astype(dtype)
    w[..., 1] = s_g * g.astype(dtype)
    w[..., 2] = s_b * b.astype(dtype) + c_b * ((255 - b) * g).astype(dtype)
    return w


def apply(frame, st, dtype=np.float64):
    """out_c = rint(min(w_c, 255)) as uint8 (np.rint rounds half to even)."""
    w = weighted(frame, st, dtype)
    return np.rint(np.minimum(w, dtype(255))).astype(np.uint8)


def gray_world(frame, red=1.0, blue=0.0, max_gain=0.0):
    """(balanced frame, stats) of one frame."""
    st = coeffs(frame, red, blue, max_gain)
    return apply(frame, st), st
