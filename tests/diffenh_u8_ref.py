"""The byte route of DifferentiableEnhancement for uint8 frames, restated on the CPU (NumPy for the counting, torch for the
float32 operations, which are the module's own: one operation per operation of vgg_16_UIE.py:57-128).

    histogram -> code at rank -> v / 255 table -> stretch table -> dehaze, gamma, clamp per pixel -> quantise

x = float32(v) / 255 is strictly increasing in the byte v, so the k-th smallest value of a channel is the image of its k-th
smallest byte, and that byte is the first bin whose cumulative count exceeds k."""
import numpy as np
import torch

F32 = np.float32


def stretch_rank(L, n):
    """int((L / 100.0) * n) clamped to [0, n - 1] (vgg_16_UIE.py:78-82); L is a float32 value"""
    pos = (float(F32(L)) / 100.0) * n
    if not pos > 0.0:
        return 0
    if pos >= n - 1:
        return n - 1
    return int(pos)


def code_at_rank(hist, r):
    """the byte at sorted position r of a channel with this 256-bin histogram"""
    return int(np.searchsorted(np.cumsum(hist.astype(np.int64)), r, side="right"))


def order_statistics(u8, cols):
    """float32 [B,3,2] = p_low, p_high of every channel"""
    B, H, W, _ = u8.shape
    n = H * W
    table = np.arange(256, dtype=F32) / F32(255.0)
    os_ = np.empty((B, 3, 2), F32)
    for b in range(B):
        for c in range(3):
            hist = np.bincount(u8[b, :, :, c].ravel(), minlength=256)
            for q in range(2):
                os_[b, c, q] = table[code_at_rank(hist, stretch_rank(cols[b, q], n))]
    return os_


def float_image(u8, cols, flags=3):
    """The module's float32 output [B,H,W,3] for the frames u8 / 255 (flags: 1 omega, 2 gamma), torch.clamp's NaN rules."""
    u8 = np.asarray(u8)
    cols = np.asarray(cols, dtype=F32)
    B = u8.shape[0]
    os_ = torch.from_numpy(order_statistics(u8, cols))
    x = torch.arange(256, dtype=torch.float32) / 255.0                    # the 256 values a channel can take
    lo, hi = os_[:, :, 0:1], os_[:, :, 1:2]
    table = torch.clamp((x.view(1, 1, 256) - lo) / (hi - lo + 1e-8), 0, 1)  # [B,3,256]
    idx = torch.from_numpy(u8.astype(np.int64))
    # [B,3,H,W] contiguous, the module's layout: torch.pow's vector body and scalar tail differ in the last bit now and then,
    # and which elements fall into the tail depends on the layout
    v = torch.stack([torch.stack([table[b, c][idx[b, :, :, c]] for c in range(3)]) for b in range(B)]).contiguous()
    par = torch.from_numpy(cols.copy())
    if flags & 1:
        omega = par[:, 2].view(-1, 1, 1, 1)
        dark = torch.min(v, dim=1, keepdim=True)[0]
        t = torch.clamp(1 - omega * dark, 0.1, 1.0)
        v = torch.clamp((v - 0.6) / t + 0.6, 0, 1)
    if flags & 2:
        v = torch.pow(v + 1e-8, par[:, 3].view(-1, 1, 1, 1))
    return np.ascontiguousarray(torch.clamp(v, 0, 1).numpy().transpose(0, 2, 3, 1))


def quantise(v):
    """(uint8)(v * 255.0f) with NaN -> 0"""
    v = np.asarray(v, dtype=F32)
    with np.errstate(invalid="ignore"):
        return (np.where(np.isnan(v), F32(0), v) * F32(255.0)).astype(np.uint8)


def same_bits(a, b):
    """float32 arrays equal bit for bit, NaN equal to NaN; -0.0 and 0.0 are one value (clamp(-0.0, 0, 1) may return either:
    IEEE max / min leave the sign of a zero result open)"""
    a = np.asarray(a, dtype=F32) + F32(0.0)
    b = np.asarray(b, dtype=F32) + F32(0.0)
    if a.shape != b.shape:
        return False
    nan = np.isnan(a)
    return bool(np.array_equal(nan, np.isnan(b)) and np.array_equal(a.view(np.int32)[~nan], b.view(np.int32)[~nan]))
