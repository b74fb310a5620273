"""Torch-CPU restatement of deep_learning_parameters.DifferentiableEnhancement (the gated-gamma module), for its autograd
gradient at any size.

Written from the contract, not from the reference's code: every plane's two order statistics come
from ONE batched ``torch.sort(..., stable=True)``, so autograd routes their gradient to the element the stable sort took
them from; the sorted positions follow Python's indexing rules (no clamp).  Pinned against the real module's gradients by
tests/test_dlp_grad.py (tests/golden/dlp_grads.npz); the GPU tests use it for shapes too large for fixtures.
"""
from __future__ import annotations

import numpy as np
import torch

from diffenh_grad_ref import scalar_ok, stable_sort_source, ulp32  # noqa: F401  (shared tolerances)


def sorted_positions(L, n: int) -> np.ndarray:
    """``int(L / 100.0 * n)`` per image with Python's rules: a negative position counts from the end; one outside
    ``[-n, n - 1]`` raises IndexError, a NaN ``L`` ValueError, an infinite one OverflowError (from ``int()``), one beyond
    int64 ValueError (torch's indexing)."""
    out = []
    for v in np.asarray(L, dtype=np.float32).reshape(-1):
        k = int(float(v) / 100.0 * n)
        if not -2**63 <= k < 2**63:
            raise ValueError("Overflow when unpacking long long")
        if not -n <= k < n:
            raise IndexError(f"index {k} is out of bounds for dimension 0 with size {n}")
        out.append(k + n if k < 0 else k)
    return np.asarray(out, dtype=np.int64)


def gated(img, L_low, L_high, use_gamma, gamma, planar: bool = True, detach_stats: bool = False):
    """``img``: float32 ``(B, 3, H, W)`` (planar) or ``(B, H, W, 3)``; parameters ``(B, 1)`` tensors.  ``detach_stats``:
    the order statistics get no gradient (only the per-pixel term)."""
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
    s = torch.clamp((flat - p_lo) / r, 0, 1).reshape(B, C, H, W)
    u = use_gamma.reshape(-1, 1, 1, 1)
    z = torch.pow(s + 1e-8, 1.0 / gamma.reshape(-1, 1, 1, 1))
    y = torch.clamp(u * z + (1 - u) * s, 0, 1)
    return y if planar else y.permute(0, 2, 3, 1)


def grads(img, L_low, L_high, use_gamma, gamma, grad_out, planar: bool = True):
    """Float32 CPU autograd of :func:`gated` -> (out, grad_img, grad_use_gamma, grad_gamma)."""
    x = torch.as_tensor(np.asarray(img, dtype=np.float32)).clone().requires_grad_(True)
    tp = lambda v: torch.as_tensor(np.asarray(v, dtype=np.float32)).clone().requires_grad_(True)  # noqa: E731
    u, ga = tp(use_gamma), tp(gamma)
    out = gated(x, torch.as_tensor(np.asarray(L_low, np.float32)), torch.as_tensor(np.asarray(L_high, np.float32)), u, ga,
                planar=planar)
    out.backward(torch.as_tensor(np.asarray(grad_out, dtype=np.float32)))
    return out.detach().numpy(), x.grad.numpy(), u.grad.numpy(), ga.grad.numpy()


def check_grads(img, L_low, L_high, grad_out, got, want, planar: bool = True, tag: str = ""):
    """``got`` / ``want``: dicts with ``grad_img`` (or None), ``grad_use_gamma`` and ``grad_gamma`` ``(B, 1)``.

    Parameters: relative 1e-4, or absolute 1e-4 * sum|grad_out| of the image.  grad_img: |d| <= 8 ulp(want) +
    1e-6 max|want| of the image, except the elements the order statistics' gradients go to (stable-sort rule), which take
    the scalar tolerance.  Returns the worst grad_img error in units of its bound."""
    x = np.asarray(img) if planar else np.moveaxis(np.asarray(img), 3, 1)
    go = np.asarray(grad_out) if planar else np.moveaxis(np.asarray(grad_out), 3, 1)
    B, _, H, W = x.shape
    n = H * W
    gsum = np.abs(go.astype(np.float64)).reshape(B, -1).sum(axis=1)
    for key in ("grad_use_gamma", "grad_gamma"):
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
