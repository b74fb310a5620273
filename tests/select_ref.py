"""NumPy reference of the percentile selection (k_select.hip): what every route must return, bit for bit.

* ``percentiles``: ``np.percentile(plane, q)`` (method "linear") per plane (b, c), in the data's dtype.
* ``percentile_indices`` / ``order_stats``: the two sorted positions NumPy 2.2.6 reads for a percentile (its index
  arithmetic in the data's dtype, "above bounds" clamp included) and the exact values there (``np.partition``).
* ``chain_percentiles``: strategy 3's (lo1, hi1, lo2, hi2) the way the oracle computes them -- the white balance's
  percentiles taken on ``f1(img)``; ``chain_from_order_stats``: the device's form, ``f1`` applied to the order statistics.
* ``stretch_positions`` / ``gated_positions``: the sorted positions of the two DifferentiableEnhancement modules.
"""
from __future__ import annotations

import numpy as np

from diffenh_grad_ref import sorted_positions as stretch_positions  # noqa: F401  int((L/100.0)*n) clamped to [0, n-1]
from dlp_grad_ref import sorted_positions as gated_positions  # noqa: F401  Python's indexing rules


def percentile_indices(n: int, q: float, dtype):
    """NumPy 2.2.6's linear-method index arithmetic for ``n`` values of ``dtype`` at percentile ``q``:
    ``(prev, next, gamma)`` with gamma in ``dtype``.  ``q / dtype(100)`` and ``(n - 1) * q`` round in the data's dtype
    (NEP 50: the Python scalars are weak); at or above ``n - 1`` both neighbours are the maximum."""
    dt = np.dtype(dtype).type
    qd = dt(q) / dt(100)
    vi = dt(n - 1) * qd
    if vi >= dt(n - 1):
        return n - 1, n - 1, dt(0)
    prev = int(np.floor(vi))
    return prev, prev + 1, dt(vi - dt(prev))


def planes(img, planar: bool = False):
    """(B, 3, n) view of a [B, H, W, 3] (or [B, 3, H, W] when planar) batch."""
    a = np.asarray(img)
    if not planar:
        a = np.moveaxis(a, -1, 1)
    return a.reshape(a.shape[0], 3, -1)


def percentiles(img, qs, planar: bool = False) -> np.ndarray:
    """[B, 3, len(qs)] of ``np.percentile(plane, q)`` in the data's dtype."""
    p = planes(img, planar)
    out = np.empty(p.shape[:2] + (len(qs),), p.dtype)
    for b in range(p.shape[0]):
        for c in range(3):
            for j, q in enumerate(qs):
                out[b, c, j] = np.percentile(p[b, c], q)
    return out


def kth(plane, ks) -> np.ndarray:
    """Exact values at the sorted positions ``ks`` of ``plane`` (np.partition)."""
    flat = np.asarray(plane).reshape(-1)
    ks = [int(k) for k in ks]
    part = np.partition(flat, sorted(set(ks)))
    return part[ks]


def order_stats(img, qs, planar: bool = False) -> np.ndarray:
    """[B, 3, len(qs), 2] of the values at NumPy's (prev, next) positions of each percentile."""
    p = planes(img, planar)
    n = p.shape[2]
    ks = []
    for q in qs:
        prev, nxt, _ = percentile_indices(n, q, p.dtype)
        ks += [prev, nxt]
    out = np.empty(p.shape[:2] + (len(qs), 2), p.dtype)
    for b in range(p.shape[0]):
        for c in range(3):
            out[b, c] = kth(p[b, c], ks).reshape(len(qs), 2)
    return out


def lerp(a, b, t):
    """NumPy's _lerp in the dtype of a and b."""
    a, b = np.asarray(a), np.asarray(b)
    t = a.dtype.type(t)
    diff = b - a
    with np.errstate(invalid="ignore", over="ignore"):
        return np.where(t >= 0.5, b - diff * (a.dtype.type(1) - t), a + diff * t).astype(a.dtype)


def stretch_f1(x, lo1, hi1, eps=1e-6):
    """The first stretch of strategy 3 (six_stadigy.py:191-199) in float32: clip((x - lo1) / (hi1 - lo1 + eps), 0, 1)."""
    x = np.asarray(x, np.float32)
    lo1, hi1 = np.float32(lo1), np.float32(hi1)
    return np.clip((x - lo1) / (hi1 - lo1 + np.float32(eps)), np.float32(0), np.float32(1))


def chain_percentiles(img, L_low, L_high, wb, eps=1e-6) -> np.ndarray:
    """[B, 3, 4] = lo1, hi1 of the float32 image, then lo2, hi2 of f1(img) (white_balance's stretch(y, wb, 100 - wb))."""
    p = planes(img)
    out = np.empty(p.shape[:2] + (4,), np.float32)
    for b in range(p.shape[0]):
        for c in range(3):
            lo1, hi1 = np.percentile(p[b, c], L_low), np.percentile(p[b, c], L_high)
            f1 = stretch_f1(p[b, c], lo1, hi1, eps)
            out[b, c] = lo1, hi1, np.percentile(f1, wb), np.percentile(f1, 100 - wb)
    return out


def chain_from_order_stats(img, L_low, L_high, wb, eps=1e-6) -> np.ndarray:
    """The device's chained form (k_pct_finish_chain): f1 applied to the order statistics of the image at the white
    balance's ranks, then lerped; the same as :func:`chain_percentiles` because f1 is monotone non-decreasing."""
    p = planes(img)
    n = p.shape[2]
    qs = (L_low, L_high, wb, 100 - wb)
    os_ = order_stats(img, qs)
    out = np.empty(p.shape[:2] + (4,), np.float32)
    for j, q in enumerate(qs[:2]):
        out[:, :, j] = lerp(os_[:, :, j, 0], os_[:, :, j, 1], percentile_indices(n, q, np.float32)[2])
    for b in range(p.shape[0]):
        for c in range(3):
            m = stretch_f1(os_[b, c, 2:], out[b, c, 0], out[b, c, 1], eps)
            for j in (2, 3):
                out[b, c, j] = lerp(m[j - 2, 0], m[j - 2, 1], percentile_indices(n, qs[j], np.float32)[2])
    return out


def same_bits(got, want) -> np.ndarray:
    """Elementwise bitwise equality (NaN equals NaN; -0.0 differs from +0.0)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    u = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    return (got.view(u) == want.view(u)) | (np.isnan(got) & np.isnan(want))


def describe_mismatch(got, want, what: str = "") -> str:
    """Message for a bitwise comparison: the first differing entries, with signed zeros spelled out."""
    ok = same_bits(got, want)
    bad = np.argwhere(~ok)
    rows = []
    for idx in bad[:6]:
        g, w = np.asarray(got)[tuple(idx)], np.asarray(want)[tuple(idx)]
        zero = " (-0.0 vs +0.0)" if g == w == 0 else ""
        rows.append(f"{tuple(int(i) for i in idx)}: got {g!r} want {w!r}{zero}")
    return f"{what}: {len(bad)} of {ok.size} values differ: " + "; ".join(rows)


def assert_same(got, want, what: str = ""):
    assert same_bits(got, want).all(), describe_mismatch(got, want, what)
