"""CPU restatement of the byte-domain gated module (uwie_diff_gated_u8): bincount, the sorted positions
by Python's indexing rules, the code at each position, a 256-entry table per (image, channel) by the module's torch
operations, a gather, the quantisation.  tests/test_gated_u8_ref.py pins it to the float-image restatement
(tests/dlp_grad_ref.py gated, itself pinned to the real module)."""
from __future__ import annotations

import numpy as np
import torch

from dlp_grad_ref import sorted_positions


def code_at(hist, k):
    """the byte value at sorted position k of a channel with this 256-bin histogram"""
    return int(np.searchsorted(np.cumsum(hist), k, side="right"))


def order_statistics(u8, cols):
    """float32 [B,3,2] = p_low, p_high per channel"""
    B, H, W, _ = u8.shape
    n = H * W
    klo, khi = sorted_positions(cols[:, 0], n), sorted_positions(cols[:, 1], n)
    out = np.zeros((B, 3, 2), np.float32)
    for b in range(B):
        for c in range(3):
            hist = np.bincount(u8[b, :, :, c].reshape(-1), minlength=256)
            for q, k in enumerate((klo[b], khi[b])):
                out[b, c, q] = np.float32(code_at(hist, int(k))) / np.float32(255.0)
    return out


def tables(u8, cols):
    """float32 [B,3,256]: the module's value for each byte of each channel, by the module's torch operations"""
    os_ = torch.from_numpy(order_statistics(u8, cols))
    x = torch.arange(256, dtype=torch.float32) / 255.0
    out = []
    for b in range(u8.shape[0]):
        u, g = torch.tensor(cols[b, 2]), torch.tensor(cols[b, 3])
        rows = []
        for c in range(3):
            p_lo, p_hi = os_[b, c, 0], os_[b, c, 1]
            s = torch.clamp((x - p_lo) / (p_hi - p_lo + 1e-8), 0, 1)
            z = torch.pow(s + 1e-8, 1.0 / g)
            rows.append(torch.clamp(u * z + (1 - u) * s, 0, 1))
        out.append(torch.stack(rows))
    return torch.stack(out).numpy()


def float_image(u8, cols):
    """float32 [B,H,W,3]"""
    t = tables(u8, cols)
    out = np.empty(u8.shape, np.float32)
    for b in range(u8.shape[0]):
        for c in range(3):
            out[b, :, :, c] = t[b, c][u8[b, :, :, c]]
    return out


def quantise(x):
    return (np.clip(x, 0, 1) * 255).astype(np.uint8)


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.int32), np.ascontiguousarray(b, np.float32).view(np.int32))
