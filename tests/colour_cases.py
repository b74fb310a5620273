"""The frames that hold every device restatement of OpenCV's 8-bit RGB <-> LAB and RGB -> gray arithmetic to the oracle over the
whole 24-bit colour cube, and the measures of what those frames reach.  NumPy and the oracle only, seeded, no GPU.
tests/test_colour_cases.py asserts on the CPU that every frame is what it claims to be; tests/test_gpu_colour_cube.py compares
the device with the oracle on them.

  cube          all 2^24 byte triples as one 4096 x 4096 frame: pixel i holds (i >> 16, i >> 8 & 255, i & 255)
  shuffled      the same pixels under a seeded permutation: every colour in every position mod 4 of the packed 12-byte stores
  quarters      the shuffled cube as four 2048 x 2048 frames: the channel histograms of each are so close to uniform that
                strategy 2 with omega 0 and percentiles (0, 99.5) hands every pixel's bytes to RGB -> LAB unchanged
  lab_frames    one colour per distinct LAB triple of the cube (2 135 975), alone or with as many gray "ballast" pixels of one
                band, shuffled so that every tile has the same histogram: CLAHE then maps L to a different L' per (ballast,
                clip limit), which spreads the (L', a, b) that LAB -> RGB sees inside the blend kernel

Strategy 2 reaches the device's RGB -> LAB with the frame's own bytes when its dehazing and stretch are the identity on codes:
omega 0 (t0 = 1, so t = 1), percentiles (0, 99.5) on a frame whose channels hold 0 and whose 99.5th percentile is 254 / 255
exactly.  STRATEGY2 holds those parameters, strategy2_before_clahe the oracle's composition of them.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

N = 1 << 24
SIDE = 4096
QUARTER = 2048
LAB_WIDTH = 1464

QUARTER_GRIDS = [((8, 8), 1), ((32, 32), 0)]  # (tile grid, uwie_clahe_plan's wide_lut for a recomputed source) on a quarter

_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        v = make()
        v.setflags(write=False)
        _CACHE[key] = v
    return _CACHE[key]


def cube_pixels():
    """(2^24, 3) u8, pixel i = (i >> 16, i >> 8 & 255, i & 255).  Read-only: copy before handing it to torch."""
    def make():
        i = np.arange(N, dtype=np.uint32)
        return np.stack([(i >> 16).astype(np.uint8), (i >> 8).astype(np.uint8), i.astype(np.uint8)], axis=1)

    return _cached("cube", make)


def cube():
    return cube_pixels().reshape(SIDE, SIDE, 3)


def permutation(n, seed):
    return _cached(("perm", n, seed), lambda: np.random.default_rng([24, seed]).permutation(n).astype(np.uint32))


def shuffled(seed=1):
    """The cube's pixels under a seeded permutation, and the permutation: shuffled.reshape(-1, 3)[k] = cube_pixels()[perm[k]]."""
    perm = permutation(N, seed)
    return _cached(("shuffled", seed), lambda: cube_pixels()[perm].reshape(SIDE, SIDE, 3)), perm


def quarter(i, seed=1):
    """Quarter i (0..3) of the shuffled cube: a 2048 x 2048 frame."""
    s, _ = shuffled(seed)
    n = QUARTER * QUARTER
    return s.reshape(-1, 3)[i * n:(i + 1) * n].reshape(QUARTER, QUARTER, 3)


def colour_index(px):
    """The cube index of every pixel: r << 16 | g << 8 | b."""
    px = np.asarray(px).reshape(-1, 3).astype(np.uint32)
    return (px[:, 0] << 16) | (px[:, 1] << 8) | px[:, 2]


def perturbed_float(u8, dtype, seed=2):
    """A float image in [0, 1] that is NOT u8 / 255 data and truncates (x * 255) to exactly the bytes of u8: the general float
    route of clahe_f32 and of the dict surface sees every colour of u8.  (u8 + d) / 255 with d in [0.25, 0.75), and d = 0 for
    byte 255 (only 1.0 itself truncates to it)."""
    rng = np.random.default_rng([24, seed])
    d = rng.random(u8.shape, dtype=np.float32) * np.float32(0.5) + np.float32(0.25)
    d[u8 == 255] = 0
    return np.ascontiguousarray(((u8.astype(np.float64) + d) / 255.0).astype(dtype))


# --------------------------------------------------------------------------------------------------- LAB triples of the cube
def lab_key(lab):
    lab = np.asarray(lab).reshape(-1, 3).astype(np.uint32)
    return (lab[:, 0] << 16) | (lab[:, 1] << 8) | lab[:, 2]


def gamut(orc):
    """(keys, colours): the distinct LAB byte triples of the cube as sorted keys L << 16 | a << 8 | b, and for each the RGB
    colour of lowest cube index that maps to it, (n, 3) u8."""
    def make():
        keys, first = np.unique(lab_key(orc.cv_rgb2lab_u8(cube())), return_index=True)
        _CACHE["gamut_colours"] = cube_pixels()[first]
        _CACHE["gamut_colours"].setflags(write=False)
        return keys

    keys = _cached("gamut_keys", make)
    return keys, _CACHE["gamut_colours"]


class LabFrame(NamedTuple):
    name: str
    band: tuple | None  # gray ballast values lo..hi inclusive, or None
    weight: int         # ballast pixels per colour pixel
    clip: float
    tiles: tuple

    @property
    def id(self):
        b = "plain" if self.band is None else f"gray{self.band[0]}-{self.band[1]}x{self.weight}"
        return f"{b}-c{self.clip:g}-t{self.tiles[0]}x{self.tiles[1]}"


LAB_FRAMES = [
    LabFrame("plain", None, 0, 2.0, (8, 8)),
    LabFrame("plain", None, 0, 1.0, (8, 8)),
    LabFrame("dark", (0, 40), 1, 40.0, (4, 4)),
    LabFrame("bright", (214, 254), 1, 40.0, (4, 4)),
    LabFrame("bright", (214, 254), 1, 2.0, (8, 8)),
]


def lab_frame(orc, case: LabFrame):
    """The u8 frame of a case: the gamut's colours, the ballast grays (the band's values in turn, equally often) and gray 254
    pins, all shuffled together, LAB_WIDTH to the row."""
    def make():
        _, colours = gamut(orc)
        parts = [colours]
        if case.band is not None:
            lo, hi = case.band
            g = (lo + np.arange(case.weight * len(colours)) % (hi - lo + 1)).astype(np.uint8)
            parts.append(np.repeat(g[:, None], 3, axis=1))
        # gray 254 "pins": the 99.5th percentile of every channel has to be 254 / 255 exactly (more than 0.5 % of the values
        # at 254 or above, fewer than 0.5 % at 255), and the rows have to be whole
        px = np.concatenate(parts)
        top = min(int(np.count_nonzero(px[:, c] >= 254)) for c in range(3))
        n = len(px)
        pins = max(0, int(np.ceil((0.0052 * n - top) / (1 - 0.0052))))
        n += pins
        rows = -(-n // LAB_WIDTH)
        parts.append(np.full((pins + rows * LAB_WIDTH - n, 3), 254, np.uint8))
        px = np.concatenate(parts)
        return px[permutation(len(px), 3)].reshape(rows, LAB_WIDTH, 3)

    return _cached(("lab_frame", case.name), make)


def after_clahe(orc, u8, clip, tiles):
    """The LAB bytes LAB -> RGB is handed for a frame whose bytes reach RGB -> LAB unchanged: (L', a, b)."""
    lab = orc.cv_rgb2lab_u8(u8)
    lab[:, :, 0] = orc.cv_clahe_u8(np.ascontiguousarray(lab[:, :, 0]), clip, tiles)
    return lab


def abxz_arguments(orc, lab):
    """The two arguments LAB -> RGB gives abToXZ for each LAB byte triple, as OpenCV's Lab2RGBinteger computes them:
    ify = LabToYF_b[2 L + 1], adiv = ((5 a 53687 + 2^7) >> 13) - 128 BASE / 500, bdiv = ((b 41943 + 2^4) >> 9) - 128 BASE / 200 + 1,
    x = ify + adiv, z = ify - bdiv (BASE = 2^14).  The table is ify for 116-based L: the oracle's own."""
    t = _cached("ltoyf", lambda: orc.cv_lab_tables()["ltoyf"])
    lab = np.asarray(lab).reshape(-1, 3).astype(np.int64)
    ify = t[2 * lab[:, 0] + 1].astype(np.int64)
    base = 1 << 14
    adiv = ((5 * lab[:, 1] * 53687 + (1 << 7)) >> 13) - 128 * base // 500
    bdiv = ((lab[:, 2] * 41943 + (1 << 4)) >> 9) - 128 * base // 200 + 1
    return ify + adiv, ify - bdiv


LINEAR_BELOW = 3390  # abToXZ's linear branch: argument <= 3390


def branch_shares(orc, lab, width):
    """Of a frame's LAB bytes: the share of pixels with an abToXZ argument on the linear branch, the lowest argument, and the
    numbers of whole 4-pixel groups (along rows of ``width``) that are all-cubic and mixed."""
    x, z = abxz_arguments(orc, lab)
    linear = (x <= LINEAR_BELOW) | (z <= LINEAR_BELOW)
    lowest = int(min(x.min(), z.min()))
    rows = linear.reshape(-1, width)
    wg = width // 4 * 4
    per = rows[:, :wg].reshape(rows.shape[0], wg // 4, 4).sum(axis=2)
    return float(linear.mean()), lowest, int(np.count_nonzero(per == 0)), int(np.count_nonzero((per > 0) & (per < 4)))


# ------------------------------------------------------------------------------------------- strategy 2 as the identity on codes
STRATEGY2 = dict(omega=0.0, L_low=0.0, L_high=99.5, gf_exact=1, cast_correct=0)  # uwie_params overrides


def strategy2_before_clahe(orc, u8):
    """What strategy 2 with STRATEGY2's parameters hands to apply_clahe, composed from the oracle's stages (strategy() fixes the
    parameters): (float32 image, transmission, restored image)."""
    S = orc.SixStrategyOracle
    x = orc.normalise_u8(u8)
    A = orc.atmospheric_light(x, 1, S.gray_shift)
    t = S.transmission(x, A, 0.0, 15, 5e-1)
    r = S.restore(x, A, t)
    return S.stretch(r, 0, 99.5), t, r


def strategy2(orc, before, clip, tiles):
    """(bytes, float32 image) of strategy 2 from strategy2_before_clahe's image."""
    y = orc.SixStrategyOracle.clahe(before, clip, tiles)
    return orc.quantise_u8(y), y


DICT_IDENTITY = dict(L_low=0, L_high=100, apply_gamma=False)  # dict clahe_enhancement: no table before LAB, v -> v - 1 behind it


def dict_clahe(orc, u8, clip, tiles):
    """(bytes, float32 image, float64 image) of dict clahe_enhancement with DICT_IDENTITY on u8 / 255."""
    want = orc.DictStrategyOracle.run(orc.normalise_u8(u8), "clahe_enhancement", dict(DICT_IDENTITY, clip_limit=clip, tile_grid_size=tiles))
    return (want * 255).astype(np.uint8), want.astype(np.float32), want
