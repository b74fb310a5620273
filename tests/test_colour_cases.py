"""Preconditions of tests/test_gpu_colour_cube.py, on the CPU (no GPU), from the oracle alone: the frames of
tests/colour_cases.py hold what they claim, the parameter sets that are meant to hand a frame's own bytes to the device's
RGB -> LAB do so on the oracle, a wrong LAB byte shows in the RGB bytes behind it, and the frames built for the blend kernel's
LAB -> RGB reach the stated share of its domain.  Every measure is printed (pytest -s): README.md and DESIGN.md quote them."""
import numpy as np
import pytest

import colour_cases as K


@pytest.fixture(scope="module")
def orc():
    from oracle import uwie_oracle

    return uwie_oracle


def counts(px):
    return np.bincount(K.colour_index(px), minlength=K.N)


def test_cube_holds_every_colour_once_and_the_shuffle_moves_them_across_the_store_positions():
    px = K.cube_pixels()
    assert px.shape == (K.N, 3) and px.dtype == np.uint8
    assert np.array_equal(K.colour_index(px), np.arange(K.N, dtype=np.uint32))
    s, perm = K.shuffled()
    assert s.shape == (K.SIDE, K.SIDE, 3) and (counts(s) == 1).all()
    assert np.array_equal(K.colour_index(s), perm)
    # position mod 4 inside a packed 12-byte group: natural order gives colour i position i & 3, the shuffle an independent one
    table = np.bincount((perm & 3) * 4 + (np.arange(K.N, dtype=np.uint32) & 3), minlength=16)
    print("colours by (natural position, shuffled position) mod 4:", table.tolist())
    assert (np.abs(table - K.N / 16) < 0.01 * K.N / 16).all()
    assert np.array_equal(np.concatenate([K.quarter(i).reshape(-1, 3) for i in range(4)]), s.reshape(-1, 3))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_perturbed_float_keeps_the_bytes_and_is_refused_as_u8_data(orc, dtype):
    import underwater_image_enhancement_amd as uw

    u8 = K.cube()
    x = K.perturbed_float(u8, dtype)
    assert x.dtype == dtype and x.min() >= 0 and x.max() == 1
    assert np.array_equal((x * 255).astype(np.uint8), u8)  # what both surfaces' apply_clahe quantises
    with pytest.raises(uw.UnsupportedInputError):  # a slice that is refused refuses the frame
        uw.api._recover_u8(x[:4])


def test_one_step_in_lab_shows_in_the_rgb_bytes(orc):
    """k_stretch_lab_lut's LAB plane is not exposed: a wrong L, a or b has to show behind LAB -> RGB.  Of the distinct LAB
    triples of the cube, the share whose RGB bytes change when one component moves by one step (a step that leaves 0..255
    counts as no change)."""
    keys, colours = K.gamut(orc)
    assert len(keys) == 2135975 and len(colours) == len(keys)
    lab = np.stack([keys >> 16, (keys >> 8) & 255, keys & 255], axis=1).astype(np.uint8)
    assert np.array_equal(orc.cv_rgb2lab_u8(colours[None])[0], lab)
    ab = np.unique(keys & 0xFFFF)
    print(f"{len(keys)} distinct LAB triples, {len(ab)} distinct (a, b) pairs")
    assert len(ab) == 22684
    base = orc.cv_lab2rgb_u8(lab[None])[0]
    for c, name in enumerate("Lab"):
        for step in (-1, 1):
            moved = lab.astype(np.int16)
            moved[:, c] = np.clip(moved[:, c] + step, 0, 255)
            share = float((orc.cv_lab2rgb_u8(moved.astype(np.uint8)[None])[0] != base).any(axis=1).mean())
            print(f"{name}{step:+d}: RGB changes for {share:.4f} of the triples")
            assert share >= 0.99, (name, step, share)


@pytest.mark.parametrize("order", ["cube", "shuffled"])
def test_dict_identity_hands_the_bytes_to_lab_and_trails_by_one(orc, order):
    """dict clahe_enhancement with L_low 0, L_high 100 and no gamma: nothing before LAB, and behind LAB -> RGB the stretch is
    v -> max(v - 1, 0) on bytes: injective except 0 / 1, so a wrong byte out of LAB -> RGB stays visible."""
    u8 = K.cube() if order == "cube" else K.shuffled()[0]
    x = orc.normalise_u8(u8)
    assert orc.classify_cast(x) == "normal"  # strategy 6 rides on the cube with cast detection on
    assert np.array_equal((x * 255).astype(np.uint8), u8)
    after = orc.cv_lab2rgb_u8(K.after_clahe(orc, u8, 2.0, (8, 8)))
    got, _, _ = K.dict_clahe(orc, u8, 2.0, (8, 8))
    assert np.array_equal(got, np.maximum(after.astype(np.int16) - 1, 0).astype(np.uint8))
    assert len(np.unique(after)) == 256


@pytest.mark.parametrize("i", range(4))
def test_quarter_reaches_lab_with_its_own_bytes(orc, i):
    q = K.quarter(i)
    before, t, r = K.strategy2_before_clahe(orc, q)
    x = orc.normalise_u8(q)
    print(f"quarter {i}: t in [{t.min()!r}, {t.max()!r}], restore returns x for {float((r == x).mean()):.4f} of the values")
    assert (t == 1.0).all()
    assert not np.array_equal(r, x)  # the restore arithmetic is live
    for c in range(3):  # lo is 0, hi is 254 / 255 (to the last place of the restore), so the divisor is inside StretchDiv's fast range
        assert np.percentile(r[:, :, c], 0) == 0 and abs(float(np.percentile(r[:, :, c], 99.5)) - 254 / 255) < 1e-7
    assert np.array_equal((before * 255).astype(np.uint8), q)  # code == input byte, 255 included


def test_quarters_take_both_forms_of_the_lut_kernel():
    import underwater_image_enhancement_amd as uw
    from underwater_image_enhancement_amd import _lib

    uw.load()
    for tiles, wide in K.QUARTER_GRIDS:
        assert _lib.clahe_plan(1, K.QUARTER, K.QUARTER, tiles, 2.0, recomputed=True).wide_lut == wide, tiles
        assert _lib.clahe_plan(1, K.QUARTER, K.QUARTER, tiles, 2.0, recomputed=False).wide_lut == 0
        assert K.QUARTER % (4 * tiles[0]) == 0  # whole 4-pixel groups only: every pixel on lab_of's fast path


def test_lab_frames_reach_the_blend_kernels_domain(orc):
    """The frames of LAB_FRAMES hand LAB -> RGB inside k_clahe_apply_out at least 3.5 M distinct (L', a, b) -- of at most
    2 135 975 distinct (L, a, b) x whatever L' CLAHE makes of them, 22 684 (a, b) pairs -- with arguments of abToXZ below zero,
    at least 5 % of the pixels on its linear branch, and 4-pixel groups of both kinds."""
    seen = np.zeros(K.N, bool)
    lowest = 0
    checked = set()
    for case in K.LAB_FRAMES:
        f = K.lab_frame(orc, case)
        if case.name not in checked:
            checked.add(case.name)
            assert f.shape[1] == K.LAB_WIDTH and f.shape[0] * f.shape[1] <= 8 << 20
            before, t, _ = K.strategy2_before_clahe(orc, f)
            assert (t == 1.0).all() and np.array_equal((before * 255).astype(np.uint8), f), case.id  # strategy 2: code == byte
        lab = K.after_clahe(orc, f, case.clip, case.tiles)
        seen[K.lab_key(lab)] = True
        linear, low, cubic_groups, mixed_groups = K.branch_shares(orc, lab, K.LAB_WIDTH)
        lowest = min(lowest, low)
        print(f"{case.id}: {f.shape[0]} x {f.shape[1]}, {int(seen.sum())} distinct (L', a, b) so far, {linear:.4f} of the pixels "
              f"on the linear branch, lowest abToXZ argument {low}, {cubic_groups} all-cubic and {mixed_groups} mixed groups")
        assert linear >= 0.05 and cubic_groups > 0 and mixed_groups > 0, case.id
    assert int(seen.sum()) >= 3_500_000
    assert lowest < 0
