"""Case table of the multi-scale fusion (uwie_fusion_u8).  The level-0 passes work on ``tile_w`` x ``tile_h`` tiles staged with a
halo (uwie_fusion_plan: the launchers run on these numbers), every stencil clamps its indices to the plane, and the pyramid's
levels are odd and even in turn, so the places where the kernels can go wrong are the sizes around the tile seams, planes of
one row or one column or one point, impulses next to the borders and the seams, both ends of the byte range, and the float64
decisions of the contract: the half-to-even tie of the last rounding and steps that float32 would decide otherwise.

Shared by tests/test_fusion_cases.py (no device: the claims below, proven on tests/fusion_ref.py alone) and
tests/test_gpu_fusion.py (the kernels against the reference).  References are computed once per (case, gamma, levels)."""
import dataclasses
import functools

import numpy as np

import fusion_ref as ref

# (gamma, levels) of the device comparison
PARAMS = ((2.2, 1), (2.2, 3), (0.8, 4), (1.5, 8))
TABLE_GAMMAS = (0.5, 0.8, 1.5, 2.0, 2.2, 2.5)
TINY_SHAPES = ((1, 1), (1, 5), (5, 1), (2, 3), (3, 2))
# levels odd and even in turn: 33 x 47 -> 17 x 24 -> 9 x 12 -> 5 x 6 -> 3 x 3 -> 2 x 2 -> 1 x 1; 37 x 21 at L = 6 ends 2 x 1, 1 x 1
PARITY_SHAPES = ((33, 47), (37, 21))
IMPULSE_SHAPE_TILES = (2, 2)  # the impulse frames are 2 * tile + 3 in each direction


@dataclasses.dataclass(eq=False)  # hashed by identity: all_cases() hands out the same objects, reference() is keyed by them
class Case:
    name: str
    frame: np.ndarray  # [H, W, 3] uint8

    @property
    def shape(self):
        return self.frame.shape[:2]


def plan():
    from underwater_image_enhancement_amd import _lib

    return _lib.fusion_plan(64, 64)  # one tile for every frame


def scene(rng, H, W):
    """A balanced-looking frame with structure at several scales: a smooth field, an edge, and noise."""
    yy, xx = np.mgrid[0:H, 0:W]
    field = 110 + 60 * np.sin(xx / 7.0) * np.cos(yy / 5.0) + 50 * (xx > W // 2)
    f = field[..., None] * np.array([0.8, 1.0, 0.9]) + rng.integers(-40, 41, (H, W, 3))
    return f.clip(0, 255).astype(np.uint8)


def shape_cases(tile_w, tile_h):
    """The smallest shapes at which the kernels can still go wrong, every one a scene of its own."""
    rng = np.random.default_rng(2018)
    shapes = list(TINY_SHAPES) + list(PARITY_SHAPES)
    shapes += [(19, w) for w in (tile_w - 1, tile_w, tile_w + 1, 2 * tile_w + 3)]
    shapes += [(h, 21) for h in (tile_h - 1, tile_h, tile_h + 1, 2 * tile_h + 3)]
    seen, out = set(), []
    for h, w in shapes:
        if (h, w) not in seen:
            seen.add((h, w))
            out.append(Case(f"scene_{h}x{w}", scene(rng, h, w)))
    return out


def impulse_positions(tile_w, tile_h):
    """(y, x) of the raised pixel: every distance 0 .. 5 from each border (two borders per frame), and each side of each tile
    seam, in a frame of (2 tile_h + 3) x (2 tile_w + 3)."""
    H, W = IMPULSE_SHAPE_TILES[0] * tile_h + 3, IMPULSE_SHAPE_TILES[1] * tile_w + 3
    pos = []
    for d in range(6):
        pos += [(d, d), (H - 1 - d, W - 1 - d)]
    for k in range(1, 3):
        sy, sx = k * tile_h, k * tile_w
        pos += [(sy - 1, sx - 1), (sy, sx), (sy - 1, sx), (sy, sx - 1)]
    return (H, W), pos


def impulse_cases(tile_w, tile_h):
    (H, W), pos = impulse_positions(tile_w, tile_h)
    out = []
    for i, (y, x) in enumerate(pos):
        f = np.full((H, W, 3), (90, 120, 100), np.uint8)
        f[y, x] = ((250, 20, 180), (0, 255, 60))[i % 2]  # raised and lowered, coloured: every weight term moves
        out.append(Case(f"impulse_{y}_{x}", f))
    return out


def clipping_frame():
    """Black and white blocks side by side: the unsharp mask overshoots on both sides of every edge, so I2 clamps at 0 and at
    255, and at gamma < 1 the fused value reaches both ends."""
    f = np.zeros((24, 40, 3), np.uint8)
    f[:, 10:20] = 255
    f[8:16, 20:30] = 255
    f[:, 30:] = (3, 250, 128)
    return f


def f32_sensitive_frame():
    """A frame on which the contract evaluated in float32 gives another byte at gamma 2.2, L = 4 (found by search over seeds:
    about one random frame of this size in ten has one)."""
    f = np.random.default_rng(7).integers(0, 256, (70, 131, 3)).astype(np.uint8)
    f[..., 0] //= 3
    return f


F32_PARAMS = (2.2, 4)


def purpose_cases():
    """Frames with a purpose; what each is for is proven in tests/test_fusion_cases.py."""
    return [
        Case("flat_77_9x13", np.full((9, 13, 3), 77, np.uint8)),
        Case("black_5x9", np.zeros((5, 9, 3), np.uint8)),
        Case("white_6x7", np.full((6, 7, 3), 255, np.uint8)),
        Case("clipping_24x40", clipping_frame()),
        Case("f32_sensitive_70x131", f32_sensitive_frame()),
    ]


@functools.lru_cache(maxsize=None)
def all_cases():
    tile = plan()
    return tuple(shape_cases(*tile) + impulse_cases(*tile) + purpose_cases())


def case(name):
    return next(c for c in all_cases() if c.name.startswith(name))


@functools.lru_cache(maxsize=None)
def reference(c, gamma, levels, gray_shift=15):
    """(out, in1, in2, Wn) of the reference for one case; computed once, never written to."""
    res = ref.fusion(c.frame, gamma, levels, gray_shift)
    for a in res:
        a.setflags(write=False)
    return res


def batch_cases():
    """Batches whose frames differ: 3 frames of 5 x 7 and 4 of 33 x 31 (3 * 1023 bytes per frame: the second and fourth frame
    start at addresses that are not 4-byte aligned)."""
    rng = np.random.default_rng(99)
    out = []
    for B, H, W in ((3, 5, 7), (4, 33, 31)):
        frames = rng.integers(0, 256, (B, H, W, 3)).astype(np.float64)
        for i in range(B):
            frames[i] *= np.array([0.5 + 0.15 * i, 0.9 - 0.1 * i, 0.6 + 0.1 * i])
        out.append(frames.astype(np.uint8))
    return out


def seeded_270x480():
    """One 270 x 480 frame: a slow gradient with texture, as a balanced underwater frame looks."""
    rng = np.random.default_rng(270)
    yy, xx = np.mgrid[0:270, 0:480]
    base = np.stack([70 + xx // 8, 90 + yy // 4, 80 + (xx + yy) // 12], -1) + rng.integers(0, 70, (270, 480, 3))
    return Case("scene_270x480", base.clip(0, 255).astype(np.uint8))


def green_cast_batch():
    """The (2, 48, 64) batch of the composition test: a smooth scene with noise under a green cast, each frame its own."""
    rng = np.random.default_rng(3)
    yy, xx = np.mgrid[0:48, 0:64]
    field = 0.5 + 0.25 * np.sin(xx / 9.0) * np.cos(yy / 7.0)
    frames = []
    for tint in ((0.30, 0.85, 0.60), (0.40, 0.90, 0.50)):
        f = field[:, :, None] * np.array(tint) + rng.normal(0, 0.03, (48, 64, 3))
        frames.append(np.clip(np.floor(255 * f), 0, 255).astype(np.uint8))
    return np.stack(frames)
