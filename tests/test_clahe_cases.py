"""Preconditions of tests/test_gpu_clahe_tail.py, on the CPU (no GPU): on every plane of tests/clahe_cases.py the NumPy
restatement of OpenCV's CLAHE (tests/clahe_ref.py) and the oracle's C restatement (oracle/cvref.c) give the same bytes -- the
oracle's only pin away from 8 x 8 tiles -- and every case is what it claims to be: the clip limits clip (or do not) as
stated, the tie case holds rounding ties, the route cases take their routes.  Routes are asked of the library's own launch
plan (uwie_clahe_plan, which needs no device), not recomputed here."""
import numpy as np
import pytest

import clahe_cases as C
import clahe_ref as R


@pytest.fixture(scope="module")
def orc():
    from oracle import uwie_oracle

    return uwie_oracle


@pytest.fixture(scope="module")
def plan():
    import underwater_image_enhancement_amd as uw
    from underwater_image_enhancement_amd import _lib

    uw.load()
    return lambda case, recomputed, batch=1: _lib.clahe_plan(batch, case.H, case.W, case.tiles, case.clip, recomputed)


def planes(orc, case):
    """The planes the device meets in a case: a raw channel of the frame (the stage kernels) and the frame's L (CLAHE of
    strategy 4 and of dict clahe_enhancement)."""
    f = C.case_frame(case)
    return {"red": np.ascontiguousarray(f[:, :, 0]), "L": np.ascontiguousarray(orc.cv_rgb2lab_u8(f)[:, :, 0])}


def ids(cases):
    return [c.id for c in cases]


def test_table():
    assert len(C.CASES) == 92
    groups = {g: len(C.of_group(g)) for g in ("grid", "ragged", "clip", "ties", "flat", "wide", "abxz")}
    assert groups == dict(grid=75, ragged=1, clip=10, ties=2, flat=1, wide=2, abxz=1)
    for c in C.CASES:
        f = C.case_frame(c)
        assert f.shape == (c.H, c.W, 3) and f.dtype == np.uint8 and np.array_equal(f, C.case_frame(c))
        assert c.H * c.W <= 181 * 183
    noise, const = C.frame(96, 120, "noise"), C.frame(96, 120, "constant")
    assert len(np.unique(noise)) == 256 and len(np.unique(const.reshape(-1, 3), axis=0)) == 1
    g32, g64 = C.general_float(C.CASES[0], np.float32), C.general_float(C.CASES[0], np.float64)
    for g in (g32, g64):  # not u8 / 255 data, and the same bytes when truncated
        assert g.min() >= 0 and g.max() < 1 and not np.array_equal(np.floor(g * 255) / 255, g)


@pytest.mark.parametrize("case", C.CASES, ids=ids(C.CASES))
def test_restatement_equals_oracle(orc, plan, case):
    """Two independently written restatements of OpenCV's CLAHE, byte for byte; the library's plan has their geometry."""
    for name, p in planes(orc, case).items():
        ref = R.clahe(p, case.clip, case.tiles)
        want = orc.cv_clahe_u8(p, case.clip, case.tiles)
        bad = np.flatnonzero(ref.out != want)
        assert bad.size == 0, f"{case.id} {name}: {bad.size} bytes differ, first at {np.unravel_index(bad[0], p.shape)}"
        assert ref.luts.shape == (case.tiles[1], case.tiles[0], 256)
    g = R.geometry(case.H, case.W, case.tiles, case.clip)
    for recomputed in (False, True):
        q = plan(case, recomputed)
        assert (q.tile_w, q.tile_h, bool(q.padded), q.clip_limit) == (g["tw"], g["th"], g["padded"], g["limit"]), case.id
        # every interpolation cell that can hold a pixel is on one of the two loops
        nx = sum(1 for i in range(case.tiles[0] + 1) if max(i * g["tw"] - g["tw"] // 2, 0) < min((i + 1) * g["tw"] - g["tw"] // 2, case.W))
        ny = sum(1 for i in range(case.tiles[1] + 1) if max(i * g["th"] - g["th"] // 2, 0) < min((i + 1) * g["th"] - g["th"] // 2, case.H))
        assert q.cells_walk + q.cells_flat == nx * ny and q.nchunk >= 1, case.id


def test_grids_cover_the_window_clamp_and_the_long_pads():
    grids = {c.tiles for c in C.of_group("grid")}
    assert any(tx < 4 and ty < 4 for tx, ty in grids) and any(tx < 4 <= ty for tx, ty in grids) and any(ty < 4 <= tx for tx, ty in grids)
    assert sum(tx != ty for tx, ty in grids) >= 6
    for H, W, tiles in ((16, 16, (64, 64)), (1, 1, (2, 2))):
        g = R.geometry(H, W, tiles)
        assert g["padded"] and g["We"] - W >= W and g["He"] - H >= H, (H, W, tiles)  # the reflection has to repeat
    g = R.geometry(5, 7, (3, 2))  # pads by a third of the frame: tiles of 3 x 3 on 5 x 7, no repeat
    assert g["padded"] and (g["tw"], g["th"], g["We"], g["He"]) == (3, 3, 9, 6)
    # 97 x 131 is ragged under every grid but (1, 1); 96 x 120 under (64, 64), (16, 8) and (5, 4) only... both kinds occur
    assert R.geometry(96, 120, (12, 12))["padded"] is False and R.geometry(97, 131, (12, 12))["padded"] is True


def test_one_ragged_direction_pads_both(plan):
    (case,) = C.of_group("ragged")
    assert case.H % case.tiles[1] == 0 and case.W % case.tiles[0] != 0
    g = R.geometry(case.H, case.W, case.tiles, case.clip)
    assert (g["He"], g["We"]) == (72, 104)
    q = plan(case, True)
    assert q.padded == 1 and q.tile_h * case.tiles[1] == 72 and q.tile_w * case.tiles[0] == 104


@pytest.mark.parametrize("case", C.of_group("clip"), ids=ids(C.of_group("clip")))
def test_clip_limits_do_what_they_claim(orc, plan, case):
    g = R.geometry(case.H, case.W, case.tiles, case.clip)
    assert plan(case, True).clip_limit == g["limit"]
    if case.clip == 0.0:
        assert g["limit"] == 0
    if case.clip == 0.01:
        assert g["limit"] == 1 and int(case.clip * g["area"] / 256) == 0  # truncates to 0, raised to 1
    for name, p in planes(orc, case).items():
        ref = R.clahe(p, case.clip, case.tiles)
        if case.clip == 1e6:
            assert ref.info["hist_max"] < g["limit"] and not ref.info["cut"].any(), name  # exceeded by no bin
        if case.clip == 0.0:
            assert not ref.info["cut"].any()
        if case.content == "constant" and 0 < case.clip < 1e6:
            assert g["limit"] < g["area"]
            assert ref.info["hist_max"] == g["area"] and (ref.info["cut"] == g["area"] - g["limit"]).all(), name
        if case.content == "noise" and case.clip in (0.01, 1.0):
            assert (ref.info["cut"] > 0).all(), name


def test_constant_tiles_leave_a_stepped_residual():
    """Every count of a one-value tile is over the limit; for at least one grid the cut total is no multiple of 256, so the
    stepped redistribution runs, with several different steps."""
    residuals = {}
    for c in C.CASES:
        if c.content == "constant" and c.clip > 0:
            g = R.geometry(c.H, c.W, c.tiles, c.clip)
            if g["limit"] < g["area"]:
                residuals[c.id] = (g["area"] - g["limit"]) % 256
    assert len(residuals) >= 25
    assert sum(r != 0 for r in residuals.values()) >= 10, residuals
    assert len({256 // r for r in residuals.values() if r}) >= 4, residuals  # several different steps


@pytest.mark.parametrize("case", C.of_group("ties"), ids=ids(C.of_group("ties")))
def test_tie_case_holds_ties(orc, case):
    g = R.geometry(case.H, case.W, case.tiles, case.clip)
    assert g["area"] == 510 and np.float32(255) / np.float32(510) == np.float32(0.5)
    for name, p in planes(orc, case).items():
        ref = R.clahe(p, case.clip, case.tiles)
        print(f"{case.id} {name}: {ref.lut_ties} LUT ties ({ref.info['lut_ties_up']} that half-up would round differently), "
              f"{ref.blend_ties} blend ties")
        assert ref.lut_ties > 1000 and ref.info["lut_ties_up"] > 100 and ref.blend_ties > 50, name


def test_flat_case_takes_both_loops(plan):
    (case,) = C.of_group("flat")
    for recomputed in (True, False):
        q = plan(case, recomputed)
        assert q.cells_flat >= 1 and q.cells_walk >= 1, (q.cells_flat, q.cells_walk)
    # no other case does: without this one the flat loop never runs
    assert all(plan(c, True).cells_flat == 0 for c in C.CASES if c.group != "flat")


def test_wide_cases_take_the_wide_kernel(plan):
    small, big = C.of_group("wide")
    for case in (small, big):
        assert plan(case, True).wide_lut == 1 and plan(case, False).wide_lut == 0, case.id
        assert plan(case, True, batch=512).wide_lut == 0  # many tiles in the call: the 256-thread form
    q = plan(big, True)
    assert (q.tile_w, q.tile_h, q.padded) == (92, 91, 1) and q.nchunk > 1
    assert 2 * q.tile_w - big.W == 1 and 2 * q.tile_h - big.H == 1  # one reflected column, one reflected row
    assert plan(small, True).padded == 0


def test_abxz_case_mixes_linear_and_cubic_pixels(orc):
    (case,) = C.of_group("abxz")
    lab = orc.cv_rgb2lab_u8(C.case_frame(case))
    lab[:, :, 0] = orc.cv_clahe_u8(lab[:, :, 0], case.clip, case.tiles)
    L, a, b = lab[:, :, 0] * (100.0 / 255.0), lab[:, :, 1] - 128.0, lab[:, :, 2] - 128.0
    fy = (L + 16.0) / 116.0
    linear = (fy - b / 200.0 < 6.0 / 29.0) | (fy + a / 500.0 < 6.0 / 29.0)
    frac = linear.mean()
    print(f"{case.id}: {frac:.3f} of the pixels take abToXZ's linear branch")
    assert 0.10 < frac < 0.90
    # ... inside 4-pixel groups that hold both kinds
    Wg = case.W // 4 * 4
    per_group = linear[:, :Wg].reshape(case.H, Wg // 4, 4).sum(axis=2)
    assert np.count_nonzero((per_group > 0) & (per_group < 4)) > 0.5 * per_group.size
