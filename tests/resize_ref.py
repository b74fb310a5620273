"""NumPy restatement of the trainer's per-frame preparation -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.

* ``resize(frame, dsize)``: ``cv2.resize(frame, dsize)`` with the default INTER_LINEAR on 8-bit frames (gray ``[H,W]`` or
  ``[H,W,C]``), OpenCV's fixed-point path:
  - ``dsize == (W, H)``: a copy (cv::resize's early return);
  - exactly 2x smaller on both axes: INTER_AREA's fast path, ``(a + b + c + d + 2) >> 2`` per channel;
  - otherwise the two-tap linear resize: source coordinate ``(float)((d + 0.5) * scale - 0.5)`` with
    ``scale = 1 / (dst / src)`` in double, 11-bit coefficients ``saturate_cast<short>(c * 2048)``; the horizontal pass
    exact in int; the vertical pass with ``VResizeLinearVec_32s8u``'s rounding, and the elements of a row past the vector
    loops with the scalar ``FixedPtCast<int, uchar, 22>`` (the "tail", ``vertical_tail_start``).
  Borders: a column coordinate below 0 or at/after W - 1 is clamped with its fraction set to 0 (resizeGeneric's xmin /
  xmax); a row coordinate keeps its fraction and only the two row indices are clipped to [0, H - 1] (resizeGeneric fills
  ``ibeta`` without a clamp, the invoker clips ``sy``).  Downscaling never reaches either rule on the rows, so
  ``features79_ref.resize128`` (which clamps both) is the same function there.
  The tail rule and the row border are read from OpenCV's source, unpinned: OpenCV is not installed where this was written.
* ``to_chw_f32`` (``u8.astype(float32) / 255.0`` then ``permute(2, 0, 1)``), ``normalize`` (torchvision's float32
  ``sub_(mean).div_(std)``) and ``flip`` (``np.fliplr`` / ``np.flipud`` of the resized frame).
"""
from __future__ import annotations

import numpy as np

COEF_BITS = 11
COEF_SCALE = 1 << COEF_BITS          # INTER_RESIZE_COEF_SCALE
VEC_BYTES = 16                       # OpenCV's baseline SIMD width (v_uint8::nlanes with 128-bit universal intrinsics)
IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)
FLIP_LR, FLIP_UD = 1, 2


def taps(src: int, dst: int, clamp: bool):
    """Two-tap source indices and 11-bit coefficients of each of ``dst`` output coordinates: (s0, s1, c0, c1), int64.
    ``clamp``: the column rule (fraction zeroed at the borders); otherwise the row rule (indices clipped only)."""
    scale = 1.0 / (dst / src)  # resizeGeneric: scale = 1 / inv_scale
    d = np.arange(dst, dtype=np.float64)
    f = ((d + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    f = (f - s.astype(np.float32)).astype(np.float32)
    if clamp:
        lo = s < 0
        f[lo], s[lo] = 0, 0
        hi = s >= src - 1
        f[hi], s[hi] = 0, src - 1
    c0 = np.rint((np.float32(1) - f) * np.float32(COEF_SCALE)).astype(np.int64)
    c1 = np.rint(f * np.float32(COEF_SCALE)).astype(np.int64)
    return np.clip(s, 0, src - 1), np.clip(s + 1, 0, src - 1), c0, c1


def vertical_tail_start(width: int) -> int:
    """First element of a row of ``width`` bytes that VResizeLinear computes with the scalar cast: the vector pass covers
    whole VEC_BYTES chunks while ``x <= width - VEC_BYTES``, then half chunks while ``x < width - VEC_BYTES / 2``."""
    x = (width // VEC_BYTES) * VEC_BYTES
    half = VEC_BYTES // 2
    while x < width - half:
        x += half
    return x


def vresize_vec(S0, S1, b0, b1):
    """VResizeLinearVec_32s8u: v_mul_hi of (S >> 4) with the 16-bit beta, a rounding shift by 2, u8 saturation."""
    v = (((S0 >> 4) * b0) >> 16) + (((S1 >> 4) * b1) >> 16)
    return np.clip((v + 2) >> 2, 0, 255)


def vresize_scalar(S0, S1, b0, b1):
    """FixedPtCast<int, uchar, 22>: (S0 * b0 + S1 * b1 + 2^21) >> 22, u8 saturation."""
    return np.clip((S0 * b0 + S1 * b1 + (1 << (2 * COEF_BITS - 1))) >> (2 * COEF_BITS), 0, 255)


def resize(frame: np.ndarray, dsize) -> np.ndarray:
    """cv2.resize(frame, dsize) for a uint8 ``[H,W]`` or ``[H,W,C]`` frame; ``dsize`` is OpenCV's ``(width, height)``."""
    a = np.ascontiguousarray(frame, dtype=np.uint8)
    gray = a.ndim == 2
    if gray:
        a = a[:, :, None]
    H, W, C = a.shape
    ow, oh = (int(v) for v in dsize)
    if ow <= 0 or oh <= 0 or H <= 0 or W <= 0:
        raise ValueError("empty size")
    if (oh, ow) == (H, W):
        out = a.copy()
    elif H == 2 * oh and W == 2 * ow:  # is_area_fast, iscale 2 -> INTER_AREA
        s = a.astype(np.int32)
        out = ((s[0::2, 0::2] + s[0::2, 1::2] + s[1::2, 0::2] + s[1::2, 1::2] + 2) >> 2).astype(np.uint8)
    else:
        xs0, xs1, a0, a1 = taps(W, ow, clamp=True)
        ys0, ys1, b0, b1 = taps(H, oh, clamp=False)
        gi = a.astype(np.int64)
        D = gi[:, xs0] * a0[None, :, None] + gi[:, xs1] * a1[None, :, None]  # HResizeLinear: int rows [H, ow, C]
        S0, S1 = D[ys0].reshape(oh, ow * C), D[ys1].reshape(oh, ow * C)
        bb0, bb1 = b0[:, None], b1[:, None]
        v = vresize_vec(S0, S1, bb0, bb1)
        t = vertical_tail_start(ow * C)
        v[:, t:] = vresize_scalar(S0[:, t:], S1[:, t:], bb0, bb1)
        out = v.astype(np.uint8).reshape(oh, ow, C)
    return out[:, :, 0] if gray else out


def resize_scalar(frame: np.ndarray, dsize) -> np.ndarray:
    """The same function evaluated one output element at a time in plain Python ints (a check on the vectorised form)."""
    a = np.ascontiguousarray(frame, dtype=np.uint8)
    a = a[:, :, None] if a.ndim == 2 else a
    H, W, C = a.shape
    ow, oh = (int(v) for v in dsize)
    out = np.zeros((oh, ow, C), np.uint8)
    xt, yt = taps(W, ow, True), taps(H, oh, False)
    tail = vertical_tail_start(ow * C)
    for y in range(oh):
        for x in range(ow):
            for c in range(C):
                if (oh, ow) == (H, W):
                    v = int(a[y, x, c])
                elif H == 2 * oh and W == 2 * ow:
                    v = (int(a[2 * y, 2 * x, c]) + int(a[2 * y, 2 * x + 1, c]) + int(a[2 * y + 1, 2 * x, c])
                         + int(a[2 * y + 1, 2 * x + 1, c]) + 2) >> 2
                else:
                    x0, x1, a0, a1 = (int(t[x]) for t in xt)
                    y0, y1, b0, b1 = (int(t[y]) for t in yt)
                    S0 = int(a[y0, x0, c]) * a0 + int(a[y0, x1, c]) * a1
                    S1 = int(a[y1, x0, c]) * a0 + int(a[y1, x1, c]) * a1
                    if x * C + c >= tail:
                        v = (S0 * b0 + S1 * b1 + (1 << 21)) >> 22
                    else:
                        v = ((((S0 >> 4) * b0) >> 16) + (((S1 >> 4) * b1) >> 16) + 2) >> 2
                    v = min(max(v, 0), 255)
                out[y, x, c] = v
    return out[:, :, 0] if np.asarray(frame).ndim == 2 else out


def flip(frame: np.ndarray, flags: int) -> np.ndarray:
    """augment_pair's order: np.fliplr (flag 1), then np.flipud (flag 2)."""
    if flags & FLIP_LR:
        frame = np.fliplr(frame)
    if flags & FLIP_UD:
        frame = np.flipud(frame)
    return np.ascontiguousarray(frame)


def to_chw_f32(u8: np.ndarray) -> np.ndarray:
    """``u8.astype(np.float32) / 255.0`` then ``permute(2, 0, 1)``: [H,W,3] -> [3,H,W] (a [B,H,W,3] batch -> [B,3,H,W])."""
    f = u8.astype(np.float32) / np.float32(255.0)
    return np.ascontiguousarray(np.moveaxis(f, -1, -3))


def normalize(chw: np.ndarray, mean=IMAGENET_MEAN, std=IMAGENET_STD) -> np.ndarray:
    """torchvision Normalize on a float32 [..., 3, H, W] tensor: ``(x - mean) / std`` with float32 mean / std, each
    operation rounded once."""
    m = np.asarray(mean, np.float32)[:, None, None]
    s = np.asarray(std, np.float32)[:, None, None]
    return ((chw.astype(np.float32) - m) / s).astype(np.float32)


def synth_frame(H: int, W: int, seed: int) -> np.ndarray:
    """A seeded uint8 RGB frame from integer arithmetic only (large frames are rebuilt by the tests, not stored): smooth
    ramps with a blue-green tint, plus uniform noise in [0, 4)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.int64)
    ramp = ((xx * 181) // max(W, 1) + (yy * 67) // max(H, 1)) % 256
    wave = np.abs(((xx + 2 * yy) % 96) - 48)
    base = np.stack([ramp // 3 + wave, ramp // 2 + 60 + wave, 255 - ramp // 2 - wave], axis=-1)
    return np.clip(base + rng.integers(0, 4, (H, W, 3)), 0, 255).astype(np.uint8)
