"""Cases for the byte-domain gated module (uwie_diff_gated_u8), shared by the CPU restatement's test and
the GPU tests.  A case is a dict: u8 [B,H,W,3] uint8 and cols [B,4] float32 = L_low, L_high, use_gamma, gamma."""
import functools

import numpy as np

SHAPES = {  # name -> (B, H, W): why
    "shape_1x1x1": (1, 1, 1),          # smallest frame
    "shape_1x1x7": (1, 1, 7),          # tail only
    "shape_3x5x3": (3, 5, 3),          # bases at 45 and 90 bytes
    "shape_5x33x95": (5, 33, 95),      # ragged batch
    "shape_1x64x64": (1, 64, 64),      # aligned
    "shape_2x257x511": (2, 257, 511),  # odd sides
    "const_1x1080x1920": (1, 1080, 1920),  # 2 073 600 counts in one bin
}

N = 100  # the rank cases' frames are 10 x 10


def step_frame(k):
    """10 x 10: k zero pixels, then 255s (all three channels)"""
    f = np.full((N, 3), 255, np.uint8)
    f[:k] = 0
    return f.reshape(10, 10, 3)


def _rank_cases():
    f = np.float32
    out = {}
    # sorted position int(37.0 / 100.0 * 100) = 37: with 37 zeros it is the first 255, with 38 the last zero
    out["rank_k_eq_rank"] = (np.stack([step_frame(37)] * 2), np.array([[37.0, 90.0, 0.5, 1.2], [5.0, 37.0, 0.5, 1.2]], f))
    out["rank_k_eq_rank_plus_1"] = (np.stack([step_frame(38)] * 2), np.array([[37.0, 90.0, 0.5, 1.2], [5.0, 37.0, 0.5, 1.2]], f))
    # int(-3.6) = -3 wraps to n - 3 = 97 (a 255: p_low above p_high = sorted[50] ... ); int(-0.5) = 0
    out["rank_negative"] = (np.stack([step_frame(60), step_frame(60), step_frame(99)]),
                            np.array([[-3.6, 50.0, 0.3, 1.4], [-0.5, 90.0, 0.3, 1.4], [-3.6, 99.0, 0.3, 1.4]], f))
    out["rank_low_above_high"] = (np.stack([step_frame(50)] * 2), np.array([[80.0, 20.0, 0.6, 1.3], [80.0, 20.0, 0.0, 1.3]], f))
    out["rank_low_eq_high"] = (np.stack([step_frame(50)] * 2), np.array([[70.0, 70.0, 0.6, 1.3], [30.0, 30.0, 1.0, 0.7]], f))
    g = np.stack([step_frame(40)] * 3)
    g[:, 5:, :, 1] = 128  # a middle value in one channel, so that the gate has something to bend
    g[:, :, 3, 2] = 77
    out["use_gamma_0_1_037"] = (g, np.array([[10.0, 90.0, 0.0, 1.5], [10.0, 90.0, 1.0, 1.5], [10.0, 90.0, 0.37, 1.5]], f))
    out["gamma_1_15_05"] = (g, np.array([[10.0, 90.0, 0.8, 1.0], [10.0, 90.0, 0.8, 1.5], [10.0, 90.0, 0.8, 0.5]], f))
    return out


NAN_GAMMA = ("gamma_nan", np.stack([step_frame(40)] * 2), np.array([[10.0, 90.0, 0.8, np.nan], [10.0, 90.0, 0.0, np.nan]], np.float32))
# L the reference cannot index -> the exception it raises (the flagged image is the middle one of three)
UNINDEXABLE = ((100.0, IndexError), (np.nan, ValueError), (np.inf, OverflowError))


def names(rank_only=False):
    return list(_rank_cases()) if rank_only else list(SHAPES) + list(_rank_cases())


@functools.lru_cache(maxsize=None)
def case(name):
    if name in SHAPES:
        B, H, W = SHAPES[name]
        rng = np.random.default_rng(B * 1000003 + H * 1009 + W)
        if name.startswith("const"):
            u8 = np.full((B, H, W, 3), 131, np.uint8)
        else:
            u8 = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
        cols = np.stack([rng.uniform(1, 30, B), rng.uniform(65, 99, B), rng.uniform(0, 1, B), rng.uniform(0.5, 3, B)], 1).astype(np.float32)
    else:
        u8, cols = _rank_cases()[name]
    u8.setflags(write=False)
    cols.setflags(write=False)
    return {"u8": u8, "cols": cols}
