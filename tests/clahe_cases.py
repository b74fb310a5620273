"""The (shape, tile grid, clip limit, content) cases that hold CLAHE's three device implementations to the oracle: the stage
kernels (k_clahe.hip), the fused tail of strategies 1-2 and the code-domain tail of strategies 4-6 / dict
clahe_enhancement (k_fused.hip).  Pure NumPy, seeded, no GPU.  tests/test_clahe_cases.py asserts on the CPU that every
case is what it claims to be and that tests/clahe_ref.py and the oracle agree on every plane of it;
tests/test_gpu_clahe_tail.py compares the device with the oracle.

What the groups are for (k_fused.hip):
  grid    tile grids away from 8 x 8: fewer than four tiles per direction (the clamp of the 4 x 4 LUT window), tx != ty
          (a swapped unpacking of tile_grid_size), more tiles than pixels (pads wider than the frame: repeated reflection)
  ragged  one direction divides evenly, the other does not: OpenCV pads both
  clip    no clipping at all, a limit raised from 0 to 1, a limit nothing exceeds, every count over the limit
  ties    tile area 510: lutScale is exactly 0.5, so every odd cumulative count is a rounding tie, and so are blends
  flat    a cell 360 px wide: k_clahe_apply_out's flat group loop next to column-walking cells of 180 px
  wide    few, large tiles: the 1024-thread LUT kernel, with and without a reflected overhang
  abxz    dark and dark-yellow pixels among bright ones: abToXZ's linear branch inside mixed 4-pixel groups
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

GRIDS = [(1, 1), (1, 8), (8, 1), (2, 3), (3, 2), (3, 3), (4, 4), (5, 4), (12, 12), (16, 8), (64, 64)]
CONTENTS = ("noise", "underwater", "constant")
CLIPS = (0.0, 0.01, 1.0, 40.0, 1e6)
CONSTANT = (77, 120, 96)


class Case(NamedTuple):
    group: str
    H: int
    W: int
    tiles: tuple   # (tiles_x, tiles_y), as cv2.createCLAHE(tileGridSize=) and the dict's tile_grid_size take them
    clip: float
    content: str

    @property
    def id(self):
        return f"{self.group}-{self.H}x{self.W}-t{self.tiles[0]}x{self.tiles[1]}-c{self.clip:g}-{self.content}"


def _cases():
    out = []
    for H, W in ((96, 120), (97, 131)):
        out += [Case("grid", H, W, g, 2.0, c) for g in GRIDS for c in CONTENTS]
    for H, W, g in ((16, 16, (64, 64)), (5, 7, (3, 2)), (1, 1, (2, 2))):
        out += [Case("grid", H, W, g, 2.0, c) for c in CONTENTS]
    out.append(Case("ragged", 64, 100, (8, 8), 2.0, "noise"))
    out += [Case("clip", 64, 100, (8, 8), clip, c) for clip in CLIPS for c in ("noise", "constant")]
    out += [Case("ties", 136, 240, (8, 8), clip, "noise") for clip in (0.0, 2.0)]
    out.append(Case("flat", 32, 720, (2, 1), 2.0, "noise"))
    out += [Case("wide", 96, 96, (1, 1), 2.0, "underwater"), Case("wide", 181, 183, (2, 2), 2.0, "underwater")]
    out.append(Case("abxz", 61, 83, (8, 8), 2.0, "darkmix"))
    return out


CASES = _cases()
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)


def of_group(*groups):
    return [c for c in CASES if c.group in groups]


def _seed(H, W, content):
    return [H, W, CONTENTS.index(content) if content in CONTENTS else 7]


_FRAMES = {}


def frame(H, W, content):
    """The u8 RGB frame of a content at a shape: the same bytes every time (a copy of the cached frame: torch wants writable
    arrays, and no caller can spoil another's)."""
    key = (H, W, content)
    if key not in _FRAMES:
        rng = np.random.default_rng(_seed(H, W, content))
        if content == "noise":
            f = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        elif content == "underwater":
            from test_gpu_configs import underwater

            f = underwater(rng, H, W, (0.45, 0.85, 0.80))
        elif content == "constant":
            f = np.empty((H, W, 3), np.uint8)
            f[:] = CONSTANT
        elif content == "darkmix":
            kind = rng.integers(0, 3, (H, W))
            dark = rng.integers(0, 13, (H, W, 3))
            yellow = np.array([60, 60, 0]) + rng.integers(-6, 7, (H, W, 3))
            bright = rng.integers(128, 256, (H, W, 3))
            f = np.where(kind[:, :, None] == 0, dark, np.where(kind[:, :, None] == 1, yellow, bright))
            f = np.clip(f, 0, 255).astype(np.uint8)
        else:
            raise KeyError(content)
        _FRAMES[key] = f
    return _FRAMES[key].copy()


def case_frame(case: Case):
    return frame(case.H, case.W, case.content)


def batch_frames(H=96, W=120):
    """Three frames of different content for the batch tests."""
    return np.stack([frame(H, W, c) for c in CONTENTS])


def general_float(case: Case, dtype):
    """A float image in [0, 1] that is NOT u8 / 255 data (the general float path of the dict surface), from the case's frame."""
    rng = np.random.default_rng(_seed(case.H, case.W, case.content) + [1])
    f = (case_frame(case).astype(np.float64) + rng.random((case.H, case.W, 3)) * 0.999) / 256.0
    return np.ascontiguousarray(f.astype(dtype))
