"""The contract of ``uwie_params.dark_patch = k`` (include/uwie.h): the dark channel taken over a k x k patch.  The reference
has no such stage (its dark channel is the minimum over the channels of one pixel), so the definition is stated here in
NumPy and the oracle's own strategies run through it: ``PatchedSix(k)`` / ``PatchedDict(k)`` are the oracle's classes with
the erosion inserted between the channel minimum and ``1 - omega * dark`` and nothing else changed."""
import functools

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

from oracle import uwie_oracle as orc


def erode(plane, k):
    """cv2.erode(plane, ones((k, k))) with its default centre anchor a = k // 2 and its default border: the window of
    (y, x) is rows y - a .. y + k - 1 - a and columns x - a .. x + k - 1 - a, and pixels outside the image never win."""
    plane = np.asarray(plane)
    k = max(int(k), 1)
    a = k // 2
    big = np.inf if plane.dtype.kind == "f" else np.iinfo(plane.dtype).max
    padded = np.pad(plane, ((a, k - 1 - a), (a, k - 1 - a)), constant_values=big)
    return sliding_window_view(padded, (k, k)).min(axis=(2, 3)).astype(plane.dtype)


def erode_bytes(frame_u8, k):
    """The frame whose three channels were eroded as bytes."""
    return np.stack([erode(frame_u8[:, :, c], k) for c in range(3)], axis=2)


@functools.lru_cache(maxsize=None)
def PatchedSix(k):
    def transmission_init(cls, img, A, omega):
        """six_stadigy.py:170-174 with erode between the channel minimum and 1 - omega * dark."""
        dark = erode(np.min(img / (A.reshape(1, 1, 3) + 1e-6), axis=2), k)
        return np.clip(1 - omega * dark, 0.1, 1.0)

    def transmission(cls, img, A, omega, ksize, eps):
        t = orc.guided_filter(cls.guide(img), cls.transmission_init(img, A, omega), ksize, eps)
        return np.clip(t, 0.1, 1.0)

    return type(f"PatchedSix{k}", (orc.SixStrategyOracle,),
                {"transmission_init": classmethod(transmission_init), "transmission": classmethod(transmission)})


@functools.lru_cache(maxsize=None)
def PatchedDict(k):
    def transmission_init(cls, img, A, omega):
        """enhancement_strategies.py:221-225 with the erosion: eps 1e-10, no clip.  ``A``: three values or the tiled HxWx3."""
        dark = erode(np.min(img / (A + 1e-10), axis=2), k)
        return 1 - omega * dark

    def transmission(cls, img, A, omega=0.95, r=15, eps=0.001):
        g = orc.cv_rgb2gray_u8((img * 255).astype(np.uint8), cls.gray_shift).astype(np.float64) / 255.0
        return np.clip(orc.guided_filter(g, cls.transmission_init(img, A, omega), r, eps), 0.1, 1.0)

    return type(f"PatchedDict{k}", (orc.DictStrategyOracle,),
                {"transmission_init": classmethod(transmission_init), "transmission": classmethod(transmission)})


def corrected(frame_u8, kind):
    """The float32 image the SIX surface's transmission sees: u8 / 255, colour-corrected for cast ``kind`` (0 / 1 / 2)."""
    return orc.correct_cast(orc.normalise_u8(frame_u8), ("normal", "greenish", "bluish")[kind])


def six_t0(frame_u8, kind, A, omega, k):
    """float32 t0 plane of the SIX surface for a forced cast kind."""
    return PatchedSix(k).transmission_init(corrected(frame_u8, kind), np.asarray(A, np.float32), omega)


def dict_t0(frame_u8, A, omega, k):
    """float32 t0 plane of the DICT surface (no cast correction, no clip)."""
    return PatchedDict(k).transmission_init(orc.normalise_u8(frame_u8), np.asarray(A, np.float32).reshape(1, 1, 3), omega)


def enhance_u8(frame_u8, strategy, k, cast_correct=True):
    """oracle.enhance_u8 with the patched dark channel: the end-to-end expected bytes."""
    x = orc.normalise_u8(frame_u8)
    if cast_correct:
        x = orc.correct_cast(x, orc.classify_cast(x))
    return orc.quantise_u8(PatchedSix(k).strategy(strategy, x))


def dict_run(frame_u8, name, params, k):
    """DictStrategyOracle.run with the patched dark channel: the float64 image."""
    return PatchedDict(k).run(orc.normalise_u8(frame_u8), name, params)
