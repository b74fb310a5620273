"""Cases for the byte-domain DifferentiableEnhancement (uwie_diff_enhance_u8), shared by the CPU
restatement's test and the GPU tests.  A case is a dict: name, u8 [B,H,W,3] uint8, cols [B,4] float32 = L_low, L_high, omega,
gamma, finite (False where a parameter is NaN / inf: the device's fmax / fmin clamps and torch.clamp part ways there, so
such a case is compared with the device's float32 route only)."""
import functools

import numpy as np

F32 = np.float32


def _cols(rng, B):
    """parameters inside the network's ranges (vgg_16_UIE.py:193-198)"""
    return np.stack([rng.uniform(2.0, 15.0, B), rng.uniform(60.0, 95.0, B), rng.uniform(0.3, 0.9, B), rng.uniform(1.0, 1.5, B)],
                    axis=1).astype(F32)


def _frames(rng, B, H, W):
    """each channel of each image in its own sub-range of the bytes, so that the stretch has something to do"""
    out = np.empty((B, H, W, 3), np.uint8)
    for b in range(B):
        for c in range(3):
            lo = int(rng.integers(0, 100))
            hi = int(rng.integers(lo + 1, 257))
            out[b, :, :, c] = rng.integers(lo, hi, (H, W))
    return out


def _steps(k_per_channel, cols):
    """10x10 frames whose channel c is k zeros, then 255s (in scan order)"""
    u8 = np.full((1, 100, 3), 255, np.uint8)
    for c, k in enumerate(k_per_channel):
        u8[0, :k, c] = 0
    return u8.reshape(1, 10, 10, 3), np.array([cols], F32)


@functools.lru_cache(maxsize=None)
def cases():
    rng = np.random.default_rng(1612)
    out = []

    def add(name, u8, cols, finite=True):
        u8 = np.ascontiguousarray(u8, dtype=np.uint8)
        cols = np.ascontiguousarray(cols, dtype=F32)
        assert u8.ndim == 4 and u8.shape[3] == 3 and cols.shape == (u8.shape[0], 4)
        u8.setflags(write=False)
        cols.setflags(write=False)
        out.append({"name": name, "u8": u8, "cols": cols, "finite": finite})

    # shapes: n = 1 (both ranks 0, range 1e-8); under one 16-pixel group; frame bases at 45 and 90 bytes; groups and a
    # tail in every image; whole groups only; several blocks per image; one bin with two million counts
    for B, H, W in ((1, 1, 1), (1, 1, 7), (3, 5, 3), (5, 33, 95), (1, 64, 64), (2, 257, 511)):
        add(f"shape_{B}x{H}x{W}", _frames(rng, B, H, W), _cols(rng, B))
    const = np.empty((1, 1080, 1920, 3), np.uint8)
    const[...] = (37, 200, 0)
    add("constant_1080p", const, [[5.0, 90.0, 0.7, 1.2]])

    # rank edges, n = 100: L = 29 -> 28 and 57 -> 56 (the double product truncates down); k zeros with k = rank and rank + 1
    # puts sorted position `rank` on either side of the bin boundary, for the low rank (channel 0), the high one (channel 1),
    # and both in one bin (channel 2)
    add("rank_k_eq_rank", *_steps((28, 56, 60), [29.0, 57.0, 0.6, 1.3]))
    add("rank_k_eq_rank_plus_1", *_steps((29, 57, 20), [29.0, 57.0, 0.6, 1.3]))
    edge = _frames(rng, 1, 10, 10)
    add("rank_29_57_random", edge, [[29.0, 57.0, 0.5, 1.1]])
    add("rank_low_above_high", edge, [[80.0, 20.0, 0.5, 1.1]])              # negative range
    add("rank_low_above_high_constant", np.full((1, 10, 10, 3), 9), [[80.0, 20.0, 0.5, 1.1]])  # range = 1e-8
    add("rank_0_100", edge, [[0.0, 100.0, 0.5, 1.1]])
    add("rank_outside", edge, [[-5.0, 150.0, 0.5, 1.1]])
    add("rank_equal", edge, [[40.0, 40.0, 0.5, 1.1]])

    # parameters at the predictor's clip bounds (use_trained_model.py:74-77)
    pb = _frames(rng, 2, 33, 95)
    add("clip_bounds", pb, [[1.0, 65.0, 0.1, 0.5], [30.0, 99.0, 0.9, 3.0]])
    add("clip_bounds_crossed", pb, [[30.0, 65.0, 0.9, 0.5], [1.0, 99.0, 0.1, 3.0]])
    # NaN / inf parameters
    add("gamma_nan_omega_inf", pb, [[5.0, 90.0, 0.7, np.nan], [5.0, 90.0, np.inf, 1.2]], finite=False)
    return tuple(out)


def names(finite_only=False):
    return [c["name"] for c in cases() if c["finite"] or not finite_only]


def case(name):
    return next(c for c in cases() if c["name"] == name)
