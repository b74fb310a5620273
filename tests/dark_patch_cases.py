"""Case table of the patched dark channel (uwie_params.dark_patch, k_trans_patch) and an analyser that says what each case
reaches.  The kernel works on output tiles (uwie_dark_patch_plan) with a halo of a = k // 2 pixels before and k - 1 - a
pixels behind each tile, so the places where it can go wrong are the frame's borders and the seams between tiles: an
impulse (one dark pixel in a white frame) at distance d before or after a seam shows in the neighbouring tile exactly when
d <= a resp. d <= k - 1 - a, and a halo one pixel short or a swapped anchor moves that limit by one.

Shared by tests/test_dark_patch_cases.py (no device: the definition, the byte-domain identity, the coverage claims) and
tests/test_gpu_dark_patch.py (the kernel against the definition)."""
import dataclasses

import numpy as np

PATCHES = (2, 3, 4, 15, 16, 31)
# two impulse shapes: a width the kernel loads in 4-pixel groups and a ragged one (W % 4 != 0), each with a second tile in x
# that is wider than the largest halo and three tiles in y
IMPULSE_SHAPES = ((72, 152), (70, 150))
OMEGA = 0.5
A_PLAIN = (0.8, 0.78, 0.82)


@dataclasses.dataclass
class Case:
    name: str
    frame: np.ndarray          # [H, W, 3] uint8
    k: int
    kind: int = 0              # forced cast kind (SIX surface)
    A: tuple = A_PLAIN
    omega: float = OMEGA
    impulses: tuple = ()       # ((y, x), ...)

    @property
    def shape(self):
        return self.frame.shape[:2]


def plan(H, W, k):
    from underwater_image_enhancement_amd import _lib

    return _lib.dark_patch_plan(H, W, k)


def seams(n, tile):
    """First pixels of every tile but the first along an axis of n pixels."""
    return list(range(tile, n, tile))


def seam_distances(k):
    """The distances from a seam at which the halo decides: the last one that still reaches the neighbour and the first one
    that does not, for the halo before a tile (a) and the one behind it (k - 1 - a); and 1, the pixel next to the seam."""
    a = k // 2
    return sorted({d for d in (1, a, a + 1, k - 1 - a, k - a) if d >= 1})


def impulse_frame(shape, points):
    """All 255 with one dark pixel per point; every impulse has its own value, so the minimum says which one it saw."""
    f = np.full(shape + (3,), 255, np.uint8)
    for i, (y, x) in enumerate(points):
        f[y, x] = (3 * i + 1, 3 * i + 2, 3 * i + 3)
    return f


def _inside(points, shape):
    return tuple(dict.fromkeys((y, x) for y, x in points if 0 <= y < shape[0] and 0 <= x < shape[1]))


def impulse_cases():
    out = []
    for k in PATCHES:
        a = k // 2
        for H, W in IMPULSE_SHAPES:
            tw, th = plan(H, W, k)
            sx, sy = seams(W, tw), seams(H, th)
            assert sx and sy, "the impulse shapes must span a seam in both directions"
            # corners, and a / a + 1 pixels from each border
            pts = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)]
            for d in (a, a + 1):
                pts += [(d, W // 3), (H - 1 - d, W // 3), (H // 2, d), (H // 2, W - 1 - d)]
            out.append(Case(f"borders_k{k}_{H}x{W}", impulse_frame((H, W), _inside(pts, (H, W))), k, impulses=_inside(pts, (H, W))))
            # next to and at the deciding distances from every seam: along x (rows in the middle of a tile), along y, and at the crossing
            for d in seam_distances(k):
                for side in ("before", "after"):
                    off = (lambda s: s - d) if side == "before" else (lambda s: s - 1 + d)
                    pts = [(th // 2, off(x)) for x in sx] + [(off(y), tw // 2) for y in sy] + [(off(y), off(x)) for y in sy for x in sx]
                    pts = _inside(pts, (H, W))
                    out.append(Case(f"seam_{side}{d}_k{k}_{H}x{W}", impulse_frame((H, W), pts), k, impulses=pts))
    return out


def shape_cases():
    """Noise frames: frames smaller than the patch (every output is the global minimum), one pixel more than a tile in both
    directions, ragged widths and pixel counts, and the frame of the end-to-end tests."""
    rng = np.random.default_rng(20260115)
    out = []
    for H, W in ((1, 1), (1, 40), (40, 1), (3, 5)):
        out.append(Case(f"small_{H}x{W}_k15", rng.integers(0, 256, (H, W, 3), dtype=np.uint8), 15))
    tw, th = plan(64, 64, 15)
    shapes = [(th + 1, tw + 1),  # one row and one column in the second tiles
              (44, 130),          # W % 4 != 0 with npx % 4 == 0
              (61, 83),           # npx % 4 != 0
              (96, 136)]
    for H, W in shapes:
        frame = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        for k in PATCHES:
            out.append(Case(f"noise_{H}x{W}_k{k}", frame, k))
    return out


A_CHANNELS = (0.85, 0.8, 0.8)  # red wins most often as it stands; the 0.85 of a cast correction hands that to green resp. blue


def channel_cases():
    rng = np.random.default_rng(77)
    frame = rng.integers(60, 256, (40, 56, 3), dtype=np.uint8)
    return [Case(f"channels_kind{kind}_k{k}", frame, k, kind=kind, A=A_CHANNELS) for kind in (0, 1, 2) for k in (3, 15)]


def batch_cases():
    """(frames [3, H, W, 3], kinds, A [3][3], k): all 255, all 0, noise -- neighbours in memory that must not see each other."""
    rng = np.random.default_rng(5)
    out = []
    for H, W in ((40, 72), (37, 50)):
        frames = np.stack([np.full((H, W, 3), 255, np.uint8), np.zeros((H, W, 3), np.uint8),
                           rng.integers(0, 256, (H, W, 3), dtype=np.uint8)])
        out.append((frames, (0, 1, 2), ((0.8, 0.78, 0.82), (0.6, 0.9, 0.7), (0.95, 0.5, 0.66)), 15))
    return out


def all_cases():
    return impulse_cases() + shape_cases() + channel_cases()


# ------------------------------------------------------------------ the analyser
def reach(case):
    """What a case reaches: {('x' | 'y' | 'cross', 'before' | 'after', d)} for every impulse at distance d <= k from a seam
    (before: the impulse is the d-th pixel in front of the seam; after: the d-th behind it), ('corner',), ('border', d) for
    d = a, a + 1 from a border, ('ragged',) / ('groups',) for the two load paths, ('tiles', nx, ny)."""
    H, W = case.shape
    k = case.k
    a = k // 2
    tw, th = plan(H, W, k)
    sx, sy = seams(W, tw), seams(H, th)
    got = {("ragged",) if W % 4 else ("groups",), ("tiles", len(sx) + 1, len(sy) + 1)}
    if H < k and W < k:
        got.add(("global",))

    def rel(p, ss):
        return {("before", s - p) for s in ss if s - k <= p < s} | {("after", p - (s - 1)) for s in ss if s <= p < s + k}

    for y, x in case.impulses:
        rx, ry = rel(x, sx), rel(y, sy)
        got |= {("x",) + r for r in rx} | {("y",) + r for r in ry} | {("cross",) + r for r in rx & ry}
        if (y in (0, H - 1)) and (x in (0, W - 1)):
            got.add(("corner",))
        for d in (a, a + 1):
            if y in (d, H - 1 - d) or x in (d, W - 1 - d):
                got.add(("border", d))
    return got


def required(k):
    """Every class the impulse cases of patch k must reach, per load path."""
    a = k // 2
    need = {("corner",), ("border", a), ("border", a + 1)}
    for axis in ("x", "y", "cross"):
        for side in ("before", "after"):
            for d in seam_distances(k):
                need.add((axis, side, d))
    return need


def winners(case):
    """How often each channel holds the per-pixel minimum of img / (A + eps) for the case's cast kind."""
    import dark_patch_ref as ref

    q = ref.corrected(case.frame, case.kind) / (np.asarray(case.A, np.float32).reshape(1, 1, 3) + 1e-6)
    return np.bincount(np.argmin(q, axis=2).ravel(), minlength=3)
