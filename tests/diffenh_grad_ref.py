"""Torch-CPU restatement of DifferentiableEnhancement's forward, for its autograd gradient at any size.

Written from the gradient contract, not from the reference's code: every plane's two order
statistics come from ONE batched ``torch.sort(..., stable=True)`` (the tie rule is stated, not inherited from a default),
so autograd routes their gradient to the element the stable sort took them from.  Pinned against the real module's
gradients by tests/test_diffenh_grad.py (tests/golden/vgg_grads.npz); the GPU tests use it for shapes too large for
fixtures.
"""
from __future__ import annotations

import numpy as np
import torch


def sorted_positions(L, n: int) -> np.ndarray:
    """``int((L / 100.0) * n)`` clamped to ``[0, n - 1]`` per image; ``L`` float32 ``(B,)`` or ``(B, 1)``."""
    pos = (np.asarray(L, dtype=np.float32).reshape(-1).astype(np.float64) / 100.0) * n
    return np.clip(np.trunc(pos), 0, n - 1).astype(np.int64)


def stable_sort_source(plane: np.ndarray, k: int) -> int:
    """Linear index of the element a stable sort puts at position ``k``: among the elements equal to the k-th smallest
    value, the one numbered ``k - #{x < value}`` in linear index order."""
    flat = np.asarray(plane).reshape(-1)
    v = np.sort(flat, kind="stable")[k]
    return int(np.flatnonzero(flat == v)[k - int(np.count_nonzero(flat < v))])


def diff_enhance(img, L_low, L_high, omega=None, gamma=None, planar: bool = True, detach_stats: bool = False):
    """``img``: float32 ``(B, 3, H, W)`` (planar) or ``(B, H, W, 3)``; parameters ``(B, 1)`` tensors (``omega`` /
    ``gamma`` None: stage skipped).  ``detach_stats``: the order statistics get no gradient (only the per-pixel term)."""
    x = img if planar else img.permute(0, 3, 1, 2)
    B, C, H, W = x.shape
    n = H * W
    flat = x.reshape(B, C, n)
    svals = torch.sort(flat, dim=-1, stable=True).values
    idx = lambda L: torch.as_tensor(sorted_positions(L.detach().cpu().numpy(), n), device=flat.device).view(B, 1, 1).expand(B, C, 1)  # noqa: E731
    p_lo = svals.gather(-1, idx(L_low))
    p_hi = svals.gather(-1, idx(L_high))
    if detach_stats:
        p_lo, p_hi = p_lo.detach(), p_hi.detach()
    r = (p_hi - p_lo) + 1e-8
    y = torch.clamp((flat - p_lo) / r, 0, 1).reshape(B, C, H, W)
    if omega is not None:
        dark = torch.min(y, dim=1, keepdim=True).values
        t = torch.clamp(1 - omega.reshape(-1, 1, 1, 1) * dark, 0.1, 1.0)
        y = torch.clamp((y - 0.6) / t + 0.6, 0, 1)
    if gamma is not None:
        y = torch.pow(y + 1e-8, gamma.reshape(-1, 1, 1, 1))
    y = torch.clamp(y, 0, 1)
    return y if planar else y.permute(0, 2, 3, 1)


def grads(img, L_low, L_high, omega=None, gamma=None, grad_out=None, planar: bool = True):
    """Float32 CPU autograd of :func:`diff_enhance` -> (out, grad_img, grad_omega or None, grad_gamma or None)."""
    x = torch.as_tensor(np.asarray(img, dtype=np.float32)).clone().requires_grad_(True)
    tp = lambda v: None if v is None else torch.as_tensor(np.asarray(v, dtype=np.float32)).clone().requires_grad_(True)  # noqa: E731
    om, ga = tp(omega), tp(gamma)
    out = diff_enhance(x, torch.as_tensor(np.asarray(L_low, np.float32)), torch.as_tensor(np.asarray(L_high, np.float32)),
                       om, ga, planar=planar)
    out.backward(torch.as_tensor(np.asarray(grad_out, dtype=np.float32)))
    g = lambda v: None if v is None else v.grad.numpy()  # noqa: E731
    return out.detach().numpy(), x.grad.numpy(), g(om), g(ga)


# ------------------------------------------------------------------ the tolerances of the gradient contract
def ulp32(a) -> np.ndarray:
    a = np.abs(np.asarray(a, dtype=np.float32))
    return np.spacing(a).astype(np.float64)


def scalar_ok(got, want, grad_out_abs_sum) -> np.ndarray:
    """Per-value: relative error <= 1e-4, or absolute <= 1e-4 * sum|grad_out| of the image when the reference is smaller."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return np.abs(got - want) <= 1e-4 * np.maximum(np.abs(want), grad_out_abs_sum)


def check_grads(img, L_low, L_high, grad_out, got, want, planar: bool = True, tag: str = ""):
    """``got`` / ``want``: dicts with ``grad_img`` (or None) and optional ``grad_omega`` / ``grad_gamma`` ``(B, 1)``.

    grad_img: |d| <= 8 ulp(want) + 1e-6 max|want| of the image, except the elements the order statistics' gradients go
    to (stable-sort rule), which take the scalar tolerance.  Returns the worst grad_img error in units of its bound."""
    x = np.asarray(img) if planar else np.moveaxis(np.asarray(img), 3, 1)
    go = np.asarray(grad_out) if planar else np.moveaxis(np.asarray(grad_out), 3, 1)
    B, _, H, W = x.shape
    n = H * W
    gsum = np.abs(go.astype(np.float64)).reshape(B, -1).sum(axis=1)
    for key in ("grad_omega", "grad_gamma"):
        if key in want:
            ok = scalar_ok(np.asarray(got[key]).reshape(B), np.asarray(want[key]).reshape(B), gsum)
            assert ok.all(), f"{tag} {key}: got {np.asarray(got[key]).reshape(-1)}, want {np.asarray(want[key]).reshape(-1)}"
    worst = 0.0
    if want.get("grad_img") is None:
        return worst
    gi = np.asarray(got["grad_img"]) if planar else np.moveaxis(np.asarray(got["grad_img"]), 3, 1)
    wi = np.asarray(want["grad_img"]) if planar else np.moveaxis(np.asarray(want["grad_img"]), 3, 1)
    klo, khi = sorted_positions(L_low, n), sorted_positions(L_high, n)
    for b in range(B):
        bound = 8 * ulp32(wi[b]) + 1e-6 * np.abs(wi[b]).max()
        err = np.abs(gi[b].astype(np.float64) - wi[b])
        for c in range(3):
            for k in {int(klo[b]), int(khi[b])}:
                i = np.unravel_index(stable_sort_source(x[b, c], k), (H, W))
                assert scalar_ok(gi[b, c][i], wi[b, c][i], gsum[b]), \
                    f"{tag} image {b} channel {c}: order-statistic element {i}: got {gi[b, c][i]}, want {wi[b, c][i]}"
                err[c][i] = 0.0
        ratio = float((err / bound).max())
        assert ratio <= 1.0, f"{tag} image {b}: grad_img off by {err.max():.3g} ({ratio:.2f} x the bound)"
        worst = max(worst, ratio)
    return worst
