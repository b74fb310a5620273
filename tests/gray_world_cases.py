"""Case table of the gray-world pre-pass (uwie_gray_world_u8).  The sum pass adds ``block_px`` pixels per workgroup into 32-bit
integers and the apply pass takes ``thread_px`` pixels per thread, the rest of a frame byte by byte (uwie_gray_world_plan:
the launchers run on these numbers), so the places where the kernels can go wrong are the pixel counts around those two
seams, frame starts that are not 4-byte aligned, the width of the integer sums, and the float64 decisions of the contract:
exact halves, the clip at 255, the gain bound, channels whose mean is zero.

Shared by tests/test_gray_world_cases.py (no device: the claims below, proven on tests/gray_world_ref.py alone) and
tests/test_gpu_gray_world.py (the kernels against the reference).  References are computed once per (case, parameters)."""
import dataclasses
import functools

import numpy as np

import gray_world_ref as ref

# (red, blue, max_gain)
PARAMS = ((1.0, 0.0, 0.0), (1.0, 1.0, 0.0), (0.0, 0.0, 0.0), (0.7, 0.3, 0.0), (1.0, 0.0, 1.25), (0.0, 0.0, 1.0))
SMALL_SHAPES = ((1, 1), (1, 2), (1, 5), (5, 7), (1, 15), (1, 16), (1, 17), (17, 1), (3, 21))


@dataclasses.dataclass(eq=False)  # hashed by identity: all_cases() hands out the same objects, reference() is keyed by them
class Case:
    name: str
    frame: np.ndarray  # [H, W, 3] uint8

    @property
    def shape(self):
        return self.frame.shape[:2]


def plan():
    from underwater_image_enhancement_amd import _lib

    return _lib.gray_world_plan(64, 64)  # one pair for every frame


def cast_frame(rng, H, W):
    """Seeded noise under a green-blue cast: red a quarter of its range, green lifted."""
    base = rng.integers(0, 256, (H, W, 3)).astype(np.float64)
    f = np.stack([base[..., 0] * 0.25, base[..., 1] * 0.8 + 30, base[..., 2] * 0.7 + 20], -1)
    return f.clip(0, 255).astype(np.uint8)


def rectangle(npx):
    """(H, W) with H * W = npx and H the largest divisor below the square root: rows that do not end on a seam.  A prime count
    has no such rectangle: three rows of ceil(npx / 3) pixels then, up to two pixels more."""
    h = max(d for d in range(1, int(npx ** 0.5) + 1) if npx % d == 0)
    return (h, npx // h) if h > 1 else (3, -(-npx // 3))


def shape_cases(block_px, thread_px):
    """The smallest shapes at which the kernels can still go wrong, every one a cast frame of its own."""
    rng = np.random.default_rng(20181)
    shapes = list(SMALL_SHAPES) + [(1, thread_px - 1), (1, thread_px + 1)]
    for npx in (block_px - 1, block_px, block_px + 1, 2 * block_px + 3):
        shapes += [(1, npx), rectangle(npx)]
    shapes.append((270, 480))
    seen, out = set(), []
    for h, w in shapes:
        if (h, w) not in seen:
            seen.add((h, w))
            out.append(Case(f"cast_{h}x{w}", cast_frame(rng, h, w)))
    return out


def tie_frame(H=6, W=34):
    """Channel means 40 / 60 / 80, so plain gray-world has gray = 60 and gains exactly 1.5 / 1 / 0.75; columns alternate
    r = 39 / 41, g = 57 / 63, b = 78 / 82, so every w_r and w_b is 58.5 or 61.5 and must come out 58 or 62 (half to even)."""
    assert W % 2 == 0
    f = np.empty((H, W, 3), np.uint8)
    f[:, 0::2] = (39, 57, 78)
    f[:, 1::2] = (41, 63, 82)
    return f


TIE_PARAMS = (0.0, 0.0, 0.0)


def max_gain_frame():
    """Deep green, no compensation asked for: plain gray-world wants a red gain of about 10, the bound 1.25 binds."""
    rng = np.random.default_rng(7)
    f = np.empty((24, 40, 3), np.uint8)
    f[..., 0] = rng.integers(0, 21, (24, 40))
    f[..., 1] = rng.integers(150, 251, (24, 40))
    f[..., 2] = rng.integers(60, 121, (24, 40))
    return f


MAX_GAIN_PARAMS = (0.0, 0.0, 1.25)


def clipping_frame():
    """Low red with 40 bright red highlights: the red gain is well above 1, so the highlights' w_r exceeds 255 and saturates."""
    rng = np.random.default_rng(11)
    f = np.empty((32, 48, 3), np.uint8)
    f[..., 0] = rng.integers(4, 17, (32, 48))
    f[..., 1] = rng.integers(120, 181, (32, 48))
    f[..., 2] = rng.integers(90, 151, (32, 48))
    f[10:12, 8:28, 0] = rng.integers(240, 256, (2, 20))
    return f


CLIPPING_PARAMS = (1.0, 0.0, 0.0)


def f32_sensitive_frame(k=7):
    """A frame on which the same formula evaluated in float32 gives other bytes (for red = 1): the 256 x 256 frame r = row >> 1,
    g = column, b = (7 row + 13 column) mod 256, and k + 1 ballast rows of one colour that move the gains."""
    yy, xx = np.mgrid[0:256, 0:256]
    base = np.stack([yy >> 1, xx, (7 * yy + 13 * xx) % 256], -1).astype(np.uint8)
    ballast = np.empty((k + 1, 256, 3), np.uint8)
    ballast[:] = ((3 * k) % 256, (200 - k) % 256, (5 * k + 17) % 256)
    return np.concatenate([base, ballast], 0)


F32_PARAMS = (1.0, 0.0, 0.0)


def purpose_cases():
    """Frames with a purpose; what each is for is proven in tests/test_gray_world_cases.py."""
    rng = np.random.default_rng(5)
    red_zero = cast_frame(rng, 9, 13)
    red_zero[..., 0] = 0
    red_green_zero = cast_frame(rng, 9, 13)
    red_green_zero[..., :2] = 0
    yellow = np.empty((4, 5, 3), np.uint8)
    yellow[:] = (255, 255, 0)
    return [
        Case("black_5x9", np.zeros((5, 9, 3), np.uint8)),
        Case("one_gray_level_7x11", np.full((7, 11, 3), 77, np.uint8)),
        Case("red_zero_9x13", red_zero),
        Case("red_green_zero_9x13", red_green_zero),
        Case("yellow_4x5", yellow),
        Case("all_255_1024x1024", np.full((1024, 1024, 3), 255, np.uint8)),
        Case("tie_6x34", tie_frame()),
        Case("max_gain_24x40", max_gain_frame()),
        Case("clipping_32x48", clipping_frame()),
        Case("f32_sensitive_264x256", f32_sensitive_frame()),
    ]


@functools.lru_cache(maxsize=None)
def all_cases():
    return tuple(shape_cases(*plan()) + purpose_cases())


def case(name):
    return next(c for c in all_cases() if c.name.startswith(name))


@functools.lru_cache(maxsize=None)
def reference(c, params):
    """(bytes, stats, whether any w exceeds 255) of the reference for one case and one parameter set; computed once, never
    written to."""
    st = ref.coeffs(c.frame, *params)
    w = ref.weighted(c.frame, st)
    out = np.rint(np.minimum(w, 255.0)).astype(np.uint8)
    for a in (out, st):
        a.setflags(write=False)
    return out, st, bool((w > 255.0).any())


def balanced_channels(c, params):
    """The channels on which gray-world's own property holds for this case: mean(w_c) = s_c * m_c = gray when the channel's gain
    is gray / m_c -- m_c > 0 and the gain not cut by max_gain -- and no value of the frame is clipped at 255; rounding moves a
    byte by at most 1/2, so the output's byte mean lies within 1/2 of gray.  Empty when a value is clipped."""
    _, st, clipped = reference(c, params)
    if clipped:
        return []
    free = ref.coeffs(c.frame, params[0], params[1], 0.0)  # the gains without the bound
    return [ch for ch in range(3) if st[5 + ch] > 0 and st[9 + ch] == free[9 + ch]]


def batch_cases():
    """Batches whose frames each have a cast of their own: 3 frames of 5 x 7 and 4 of 33 x 31 (3 * 1023 bytes per frame: the
    second and fourth frame start at addresses that are not 4-byte aligned)."""
    rng = np.random.default_rng(99)
    out = []
    for B, H, W in ((3, 5, 7), (4, 33, 31)):
        frames = rng.integers(0, 256, (B, H, W, 3)).astype(np.float64)
        for i in range(B):
            frames[i] *= np.array([0.2 + 0.15 * i, 0.9 - 0.1 * i, 0.5 + 0.1 * i])
        out.append(frames.astype(np.uint8))
    return out


def seeded_1080p():
    """One 1080p frame with an underwater cast over a slow gradient."""
    rng = np.random.default_rng(1080)
    yy, xx = np.mgrid[0:1080, 0:1920]
    base = np.stack([20 + xx // 64, 120 + yy // 16, 90 + (xx + yy) // 48], -1) + rng.integers(0, 60, (1080, 1920, 3))
    return Case("cast_1080x1920", base.clip(0, 255).astype(np.uint8))


def green_cast_batch():
    """The (2, 96, 128) batch of the composition tests: a smooth scene with noise under a green cast, each frame its own."""
    rng = np.random.default_rng(3)
    yy, xx = np.mgrid[0:96, 0:128]
    field = 0.5 + 0.25 * np.sin(xx / 19.0) * np.cos(yy / 13.0)
    frames = []
    for tint in ((0.30, 0.85, 0.60), (0.40, 0.90, 0.50)):
        f = field[:, :, None] * np.array(tint) + rng.normal(0, 0.03, (96, 128, 3))
        frames.append(np.clip(np.floor(255 * f), 0, 255).astype(np.uint8))
    return np.stack(frames)
