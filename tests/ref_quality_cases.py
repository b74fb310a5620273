"""Case table of the full-reference scores (uwie_reference_scores_u8: MAE, MSE, PSNR, SSIM), built from the tile of map
points that uwie_reference_plan reports.  The SSIM pass stages a (tile_h + 10) x (tile_w + 10) patch per workgroup and uses
valid windows only, so the places where it can go wrong are the seams between tiles (a lost or doubled halo row or column),
the frame's border (a pixel nearer than 10 to it is covered by fewer windows), the ragged last tiles, and the frame's
neighbours in a batch.

Shared by tests/test_ref_quality_cases.py (no device: the table's preconditions on the restatement alone) and
tests/test_gpu_ref_quality.py (the kernels against the definition)."""
import dataclasses

import numpy as np

SEAM_OFFSETS = (0, -1, 1, -5, 5, -6, 6)
BORDER_DISTANCES = (0, 4, 5, 6)


@dataclasses.dataclass
class Case:
    name: str
    x: np.ndarray  # the result [H, W, 3] uint8
    y: np.ndarray  # the reference [H, W, 3] uint8

    @property
    def shape(self):
        return self.x.shape[:2]

    @property
    def has_window(self):
        return self.x.shape[0] >= 11 and self.x.shape[1] >= 11


def plan(H, W):
    from underwater_image_enhancement_amd import _lib

    return _lib.reference_plan(H, W)


def shapes(tile):
    tw, th = tile
    return ((1, 1), (10, 40), (40, 10), (11, 11), (11, 12), (12, 11), (th + 10, tw + 10), (th + 11, tw + 11), (2 * th + 15, 2 * tw + 21))


def noise_pair(rng, H, W, amplitude=24):
    """Noise, and the same noise with a perturbation bounded by amplitude."""
    y = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    x = np.clip(y.astype(np.int64) + rng.integers(-amplitude, amplitude + 1, (H, W, 3)), 0, 255).astype(np.uint8)
    return x, y


def flat_pair(H, W, a=(70, 120, 200), b=(90, 100, 20)):
    return np.broadcast_to(np.array(a, np.uint8), (H, W, 3)).copy(), np.broadcast_to(np.array(b, np.uint8), (H, W, 3)).copy()


def opposite_pair(rng, H, W):
    """Every byte 0 or 255, the reference its complement: cov < 0 wherever a window holds both levels."""
    x = (rng.integers(0, 2, (H, W, 3)) * 255).astype(np.uint8)
    return x, (255 - x).astype(np.uint8)


def shape_cases(tile):
    """Per shape: an identical pair, two flat frames, noise with a bounded perturbation, exact opposites."""
    rng = np.random.default_rng(2025)
    out = []
    for H, W in shapes(tile):
        x, y = noise_pair(rng, H, W)
        out.append(Case(f"identical_{H}x{W}", y.copy(), y))
        out.append(Case(f"flat_{H}x{W}", *flat_pair(H, W)))
        out.append(Case(f"noise_{H}x{W}", x, y))
        out.append(Case(f"opposite_{H}x{W}", *opposite_pair(rng, H, W)))
    return out


def full_hd_case():
    """One 1080p pair, for the width of the integer sums and the tile grid: noise over a slow gradient against the same scene
    with another noise and a gain."""
    rng = np.random.default_rng(1080)
    yy, xx = np.mgrid[0:1080, 0:1920]
    base = np.stack([60 + xx // 16, 200 - yy // 8, 90 + (xx + yy) // 32], axis=-1)
    y = np.clip(base + rng.integers(-40, 41, (1080, 1920, 3)), 0, 255).astype(np.uint8)
    x = np.clip(base * 0.9 + rng.integers(-30, 31, (1080, 1920, 3)), 0, 255).astype(np.uint8)
    return Case("full_hd", x, y)


def impulse_shape(tile):
    return tile[1] + 22, tile[0] + 22  # map (tile_h + 12) x (tile_w + 12): two tiles in each direction, the second ragged


def impulse_base(tile):
    """A fixed textured frame: two crossed waves and noise."""
    H, W = impulse_shape(tile)
    rng = np.random.default_rng(31)
    yy, xx = np.mgrid[0:H, 0:W]
    f = np.stack([128 + 60 * np.sin(xx / 5.0 + c) * np.cos(yy / 7.0 - c) for c in range(3)], axis=-1) + rng.integers(-20, 21, (H, W, 3))
    return np.clip(f, 0, 255).astype(np.uint8)


def seam_points(tile):
    """Pixels at the seam between the first and the second tile of map points (map row tile_h, map column tile_w: the pixel
    there is the first one that the first tile's windows no longer reach from the top / left side), and at distances 1, 5 and 6
    on both sides: along the horizontal seam, along the vertical one, and on the diagonal through their crossing."""
    tw, th = tile
    H, W = impulse_shape(tile)
    return ([(th + d, W // 2) for d in SEAM_OFFSETS] + [(H // 2, tw + d) for d in SEAM_OFFSETS] + [(th + d, tw + d) for d in SEAM_OFFSETS])


def border_points(tile):
    """Pixels at distances 0, 4, 5 and 6 from each of the frame's four borders: at distance d < 10 only d + 1 rows (or columns)
    of windows cover a pixel, so a window too many or too few at the border changes the score."""
    H, W = impulse_shape(tile)
    pts = []
    for d in BORDER_DISTANCES:
        pts += [(d, W // 3), (H - 1 - d, W // 3), (H // 3, d), (H // 3, W - 1 - d)]
    return pts


def impulse_points(tile):
    return seam_points(tile) + border_points(tile)


def impulse_cases(tile):
    """The base as the reference; the result differs from it in one pixel."""
    base = impulse_base(tile)
    out = []
    for yy, xx in impulse_points(tile):
        x = base.copy()
        x[yy, xx] = 255 - x[yy, xx]
        out.append(Case(f"impulse_{yy}_{xx}", x, base))
    return out


def batch_pairs(tile):
    """Three pairs of one shape that score very differently: bright noise with a strong perturbation, a smooth dark scene
    with a weak one, and exact opposites.  Returns (results [3, H, W, 3], references [3, H, W, 3])."""
    H, W = tile[1] + 19, tile[0] + 23
    rng = np.random.default_rng(404)
    yy, xx = np.mgrid[0:H, 0:W]
    x0, y0 = noise_pair(rng, H, W, amplitude=90)
    y1 = np.stack([40 + (xx + 2 * yy) % 50, 30 + (2 * xx + yy) % 60, 70 - (xx + yy) % 40], axis=-1).astype(np.uint8)
    x1 = np.clip(y1.astype(np.int64) + rng.integers(-2, 3, (H, W, 3)), 0, 255).astype(np.uint8)
    x2, y2 = opposite_pair(rng, H, W)
    return np.stack([x0 | 128, x1, x2]), np.stack([y0 | 128, y1, y2])


def selection_frames():
    """Two frames for select_best_reference (a hazy greenish scene and a dim bluish one) and their references: the clean scene
    they were degraded from, which is no strategy's output.  tests/test_ref_quality_cases.py checks, through the oracle's
    strategies, that the two best sets are more than 1e-3 apart on both frames by every metric."""
    rng = np.random.default_rng(77)
    yy, xx = np.mgrid[0:72, 0:96]
    field = 0.5 + 0.3 * np.sin(xx / 9.0) * np.cos(yy / 7.0)
    scene = field[:, :, None] * np.array((0.95, 0.85, 0.75)) + 0.1 * np.sin(xx / 3.0)[:, :, None] * np.array((0.5, -0.3, 0.4))
    frames, refs = [], []
    for tint, gain, noise in (((0.45, 0.85, 0.80), 0.9, 0.03), ((0.35, 0.55, 0.95), 0.6, 0.06)):
        f = gain * scene * np.array(tint) + 0.1 + rng.normal(0, noise, (72, 96, 3))
        frames.append(np.clip(np.floor(255 * f), 0, 255).astype(np.uint8))
        refs.append(np.clip(np.floor(255 * scene), 0, 255).astype(np.uint8))
    return np.stack(frames), np.stack(refs)
