"""Gray planes that make Canny's hysteresis depend on the parts of k_canny.hip that plain noise never singles out: links
across tile seams and tile corners, list walkers beyond the first wavefront and the first block, the per-tile candidate
switch, the halo load on either side of its condition.  Pure NumPy, seeded, no GPU; tests/test_canny_cases.py asserts on
the oracle alone that every pattern is what it claims to be, tests/test_gpu_canny.py compares the device with the oracle.

Geometry the patterns are laid out for (k_canny.hip): tiles of 32 rows x 64 columns, a list walker wavefront takes 16
tiles, a walker block four wavefronts (64 tiles).  Amplitudes: over a flat 100 a step of +20 / +25 gives Sobel magnitudes
of 80 / 100 on a straight edge -- weak at the thresholds (50, 150) -- and a patch of 250 gives strong ones.
"""
import numpy as np

TILE_H, TILE_W = 32, 64
FLAT, SEED_VALUE = 100, 250


def tile_counts(edges):
    """Nonzero pixels of an H x W map per 32 x 64 tile -> [tiles_y, tiles_x]."""
    H, W = edges.shape
    ty, tx = -(-H // TILE_H), -(-W // TILE_W)
    padded = np.zeros((ty * TILE_H, tx * TILE_W), bool)
    padded[:H, :W] = edges != 0
    return padded.reshape(ty, TILE_H, tx, TILE_W).sum(axis=(1, 3))


def noise(H, W, seed):
    return np.random.default_rng(seed).integers(0, 256, (H, W), dtype=np.uint8)


# ------------------------------------------------------------------------------------------------------- serpentine
SERP_BAND, SERP_PITCH, SERP_MARGIN = 6, 16, 5


def serpentine_bands(H):
    """First rows of the serpentine's horizontal runs in a plane of H rows."""
    return list(range(SERP_MARGIN, H - SERP_MARGIN - SERP_BAND + 1, SERP_PITCH))


def serpentine(H=133, W=770, amplitude=20, seed=None):
    """A boustrophedon band, 6 px wide, `amplitude` over a flat 100: horizontal runs every 16 rows, joined alternately at
    the right and the left end, so its outline is one closed weak contour that visits nearly every tile.  `seed`: None (no
    strong pixel anywhere: no edge at all), "last" (a 250-valued patch inside the last run, at the end where the outline
    finishes) or "first" (the same plane rotated by 180 degrees: the seed at the lowest pixel indices)."""
    if seed == "first":
        return np.ascontiguousarray(serpentine(H, W, amplitude, "last")[::-1, ::-1])
    assert seed in (None, "last")
    p = np.full((H, W), FLAT, np.uint8)
    x0, x1 = SERP_MARGIN, W - SERP_MARGIN
    ys = serpentine_bands(H)
    for k, y in enumerate(ys):
        p[y:y + SERP_BAND, x0:x1] = FLAT + amplitude
        if k + 1 < len(ys):
            xs = x1 - SERP_BAND if k % 2 == 0 else x0
            p[y:ys[k + 1] + SERP_BAND, xs:xs + SERP_BAND] = FLAT + amplitude
    if seed == "last":  # near the free end of the last run, across its whole width: the outline itself turns strong there
        last = len(ys) - 1
        xs = x0 + 8 if last % 2 == 0 else x1 - 8 - 4
        p[ys[-1]:ys[-1] + SERP_BAND, xs:xs + 4] = SEED_VALUE
    return p


def serpentine_transposed(amplitude=20, seed="last"):
    """The 133 x 770 serpentine as a 770 x 133 plane: the contour runs down tile columns instead of along tile rows."""
    return np.ascontiguousarray(serpentine(133, 770, amplitude, seed).T)


# ----------------------------------------------------------------------------------------- seam and corner crossers
# 64 x 128 planes = 2 x 2 tiles: the vertical seam is x = 63|64, the horizontal one y = 31|32, the corner (32, 64).
CROSS_H, CROSS_W = 64, 128


def _seed_patch(p, y, x):
    """A 3 x 3 patch of 250 centred on (y, x), a pixel on the DARK side that touches the step: the patch's strong outline
    joins the weak edge on both sides.  (Found on the oracle: a patch centred on the bright side, or inside a band without
    touching its outline, starts a contour of its own that non-maximum suppression cuts off from the weak edge.)"""
    assert p[y, x] == FLAT
    p[y - 1:y + 2, x - 1:x + 2] = SEED_VALUE


def crosser(kind, seed_side):
    """A weak step edge (+20) that crosses one seam, or the tile corner, exactly once.  `kind`:
      "vseam"   a horizontal edge between rows 15|16, from the left border to the right one: crosses x = 63|64
      "hseam"   a vertical edge between columns 31|32, from the top border to the bottom one: crosses y = 31|32
      "diag_se_hi" / "diag_se_lo"   the diagonal y - 32 = x - 64 (tile (0,0) -> tile (1,1)), bright side above / below it
      "diag_sw_hi" / "diag_sw_lo"   the diagonal y - 32 = 64 - x (tile (0,1) -> tile (1,0)), bright side above / below it
    `seed_side`: 0 / 1 puts a 250-valued 3 x 3 patch against the edge near its first / last end, None leaves the edge unseeded.
    Returns (plane, near, far): boolean masks of the tiles on the seed's side of the crossing and beyond it (for an
    unseeded plane: as for seed_side = 0)."""
    yy, xx = np.mgrid[0:CROSS_H, 0:CROSS_W]
    p = np.full((CROSS_H, CROSS_W), FLAT, np.uint8)
    if kind == "vseam":
        p[yy >= 16] = FLAT + 20
        ends = ((15, 12), (15, 116))
        sides = (xx < 64, xx >= 64)
    elif kind == "hseam":
        p[xx >= 32] = FLAT + 20
        ends = ((8, 31), (56, 31))
        sides = (yy < 32, yy >= 32)
    elif kind.startswith("diag_se"):
        d = (yy - 32) - (xx - 64)  # 0 on the diagonal, < 0 above it
        p[(d < 0) if kind.endswith("hi") else (d >= 0)] = FLAT + 20
        ends = ((8, 40), (56, 88)) if kind.endswith("hi") else ((7, 40), (55, 88))
        sides = ((yy < 32) & (xx < 64), (yy >= 32) & (xx >= 64))
    elif kind.startswith("diag_sw"):
        d = (yy - 32) + (xx - 64)  # 0 on the anti-diagonal through (32, 64), < 0 above it
        p[(d < 0) if kind.endswith("hi") else (d >= 0)] = FLAT + 20
        ends = ((8, 88), (56, 40)) if kind.endswith("hi") else ((7, 88), (55, 40))
        sides = ((yy < 32) & (xx >= 64), (yy >= 32) & (xx < 64))
    else:
        raise KeyError(kind)
    if seed_side is not None:
        _seed_patch(p, *ends[seed_side])
    near, far = (sides[0], sides[1]) if seed_side in (None, 0) else (sides[1], sides[0])
    return p, near, far


CROSSER_KINDS = ("vseam", "hseam", "diag_se_hi", "diag_se_lo", "diag_sw_hi", "diag_sw_lo")


# A purely diagonal link through the corner: the staircases above put a third pixel next to the corner, so the diagonal
# pair (31,63)-(32,64) (or (31,64)-(32,63)) is never the ONLY connection.  A bounded, seeded search on the oracle (at most
# 6000 tries per kind: the step pattern with 1..8 pixels of the 8 x 8 window around the corner redrawn from
# {100, 105, ..., 130}) found, for every kind, edits after which the oracle's map is set on one diagonal pair of the corner,
# clear on the other, and the two halves of the edge hang together by that pair alone.  The edits are kept, not the search.
PURE_DIAGONAL_EDITS = {
    "diag_se_hi": ((28, 62, 115), (29, 66, 110), (30, 67, 125), (32, 64, 125), (33, 66, 115)),
    "diag_se_lo": ((28, 62, 120), (30, 62, 100), (32, 64, 100)),
    "diag_sw_hi": ((31, 64, 100),),
    "diag_sw_lo": ((33, 64, 100), (34, 61, 130)),
}


def pure_diagonal(kind, seed_side):
    """crosser(kind, seed_side) with the corner redrawn so that the link across it is one diagonal pixel pair.  Returns
    (plane, near, far, pair, others): `pair` = the two corner pixels that carry the link, the seed's side first; `others`
    = the two corner pixels that must stay clear."""
    p, near, far = crosser(kind, seed_side)
    for y, x, v in PURE_DIAGONAL_EDITS[kind]:
        p[y, x] = v
    pair, others = (((31, 63), (32, 64)), ((31, 64), (32, 63)))
    if kind.startswith("diag_sw"):
        pair, others = others, pair
    if seed_side == 1:
        pair = pair[::-1]
    return p, near, far, pair, others


def reach(edges, start, blocked=None):
    """Mask of the pixels of an edge map that are 8-connected to `start` without stepping on `blocked`."""
    e = np.asarray(edges) != 0
    seen = np.zeros_like(e)
    if not e[start]:
        return seen
    seen[start] = True
    stack = [start]
    while stack:
        y, x = stack.pop()
        for ny in range(max(y - 1, 0), min(y + 2, e.shape[0])):
            for nx in range(max(x - 1, 0), min(x + 2, e.shape[1])):
                if e[ny, nx] and not seen[ny, nx] and (ny, nx) != blocked:
                    seen[ny, nx] = True
                    stack.append((ny, nx))
    return seen


# ------------------------------------------------------------------------------------------------------ density sweep
DENSITY_FRACTIONS = (0.004, 0.01, 0.02, 0.04, 0.07, 0.11, 0.16, 0.24, 0.4, 1.0)


def density_plane(fraction, seed):
    """64 x 128 (2 x 2 tiles) of masked noise: a `fraction` of the pixels carries a uniform random byte, the rest is flat
    128.  From a few dozen edge pixels per tile to more than 512: the gathered-roots switch of k_canny_gradnms (more than
    256 candidates in the tile) lies inside the sweep."""
    rng = np.random.default_rng(seed)
    p = np.full((64, 128), 128, np.uint8)
    mask = rng.random((64, 128)) < fraction
    p[mask] = rng.integers(0, 256, int(mask.sum()), dtype=np.uint8)
    return p


def density_sweep():
    return {f"density_{f:g}": density_plane(f, 1000 + i) for i, f in enumerate(DENSITY_FRACTIONS)}


# ------------------------------------------------------------------------------------------------------ halo boundary
def halo_cases():
    """Noise at the sizes where k_canny_gradnms's plain-load halo path (tx0 >= 2 and tx0 + 66 <= cols) switches for the
    last full tile column, where the last tile row is 0, 1, 2 rows high, exactly one tile, and one-pixel slivers."""
    out = {}
    for W in (128, 129, 130, 131):
        out[f"halo_40x{W}"] = noise(40, W, 2000 + W)
    for H in (32, 33, 34):
        out[f"halo_{H}x70"] = noise(H, 70, 2100 + H)
    out["halo_32x64"] = noise(32, 64, 2200)
    out["halo_33x65"] = noise(33, 65, 2201)
    return out


# ------------------------------------------------------------------------------------------------------ walker groups
def walker_cases():
    """64 x 1088 = 2 x 17 = 34 tiles: the third walker wavefront starts inside the second tile row."""
    return {"walk_noise_64x1088": noise(64, 1088, 3000),
            "walk_serp_64x1088": serpentine(64, 1088, 20, "last"),
            "walk_serp_first_64x1088": serpentine(64, 1088, 25, "first")}


def batch3():
    """{noise, flat 77, serpentine B} at 133 x 770: 65 tiles per frame -- two walker blocks per frame, the second holding one
    tile -- so a walker that mixes up frames (regions) reads the neighbour's lists."""
    return np.stack([noise(133, 770, 3100), np.full((133, 770), 77, np.uint8), serpentine(133, 770, 20, "last")])


# ------------------------------------------------------------------------------------------------- the whole catalogue
def serpentine_cases():
    out = {}
    for amp in (20, 25):
        out[f"serp_A_{amp}"] = serpentine(133, 770, amp, None)
        out[f"serp_B_{amp}"] = serpentine(133, 770, amp, "last")
        out[f"serp_B_first_{amp}"] = serpentine(133, 770, amp, "first")
        out[f"serp_B_T_{amp}"] = serpentine_transposed(amp, "last")
    return out


def crosser_cases():
    out = {}
    for kind in CROSSER_KINDS:
        for side in (None, 0, 1):
            out[f"cross_{kind}_{'none' if side is None else side}"] = crosser(kind, side)[0]
    for kind in PURE_DIAGONAL_EDITS:
        for side in (None, 0, 1):
            out[f"purediag_{kind}_{'none' if side is None else side}"] = pure_diagonal(kind, side)[0]
    return out


def all_cases():
    """name -> plane, every pattern of this module (the 3-frame batch as three planes)."""
    out = {}
    out.update(serpentine_cases())
    out.update(crosser_cases())
    out.update(density_sweep())
    out.update(halo_cases())
    out.update(walker_cases())
    for i, p in enumerate(batch3()):
        out[f"batch3_{i}"] = p
    return out


def gray_rgb(plane):
    """The plane as an RGB frame with R = G = B."""
    return np.ascontiguousarray(np.repeat(np.asarray(plane)[..., None], 3, axis=-1))
