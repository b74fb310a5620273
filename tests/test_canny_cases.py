"""Preconditions of tests/test_gpu_canny.py, on the oracle alone (no GPU): every pattern of tests/canny_cases.py is what it
claims to be.  Without these a GPU comparison could pass vacuously -- a serpentine whose seed does not reach the contour
compares two nearly empty maps, whatever the walkers do."""
import numpy as np
import pytest

import canny_cases as C


@pytest.fixture(scope="module")
def canny():
    from oracle import uwie_oracle

    return lambda plane, low=50, high=150: uwie_oracle.cv_canny_u8(plane, low, high)


def test_every_plane_is_small_gray_u8():
    cases = C.all_cases()
    assert len(set(cases)) == len(cases) >= 60
    for name, p in cases.items():
        assert p.dtype == np.uint8 and p.ndim == 2 and p.flags.c_contiguous, name
        assert p.shape[0] * p.shape[1] <= 300 * 1100 and max(p.shape) <= 1100, (name, p.shape)
    again = C.all_cases()  # seeded: the same bytes every time
    assert all(np.array_equal(cases[k], again[k]) for k in cases)


@pytest.mark.parametrize("amp", [20, 25])
def test_serpentine_hangs_on_its_seed(canny, amp):
    a = canny(C.serpentine(133, 770, amp, None))
    assert not a.any()  # weak everywhere: no edge at all
    first_band = C.serpentine_bands(133)[0]
    for name, plane, tiles in (("B", C.serpentine(133, 770, amp, "last"), 65), ("B first", C.serpentine(133, 770, amp, "first"), 65),
                               ("B transposed", C.serpentine_transposed(amp, "last"), 75)):
        e = canny(plane)
        tc = C.tile_counts(e)
        assert tc.size == tiles
        assert np.count_nonzero(tc) >= 40, (name, np.count_nonzero(tc))
        assert np.count_nonzero(e) > 10000, (name, np.count_nonzero(e))
        # the far end of the contour: the first run for a seed in the last one (and the other way round, and transposed)
        if name == "B":
            far = e[:first_band + C.SERP_BAND + 2]
        elif name == "B first":
            far = e[-(first_band + C.SERP_BAND + 2):]
        else:
            far = e[:, :first_band + C.SERP_BAND + 2]
        assert np.count_nonzero(far) > 1000, (name, np.count_nonzero(far))
    # the seed sits at the highest indices in B, at the lowest in its rotation
    b = C.serpentine(133, 770, amp, "last")
    ys, xs = np.nonzero(b == C.SEED_VALUE)
    assert ys.min() >= 96 and np.array_equal(C.serpentine(133, 770, amp, "first"), b[::-1, ::-1])


def test_serpentine_tiles_span_five_walker_wavefronts_and_two_blocks():
    tiles = -(-133 // C.TILE_H) * -(-770 // C.TILE_W)
    assert tiles == 65 and -(-tiles // 16) == 5 and -(-(-(-tiles // 16)) // 4) == 2 and tiles - 64 == 1


@pytest.mark.parametrize("kind", C.CROSSER_KINDS)
def test_crossers_cross(canny, kind):
    plane, near, far = C.crosser(kind, None)
    assert not canny(plane).any()
    assert not (near & far).any()
    for side in (0, 1):
        plane, near, far = C.crosser(kind, side)
        e = canny(plane) != 0
        assert np.count_nonzero(e & near) >= 30 and np.count_nonzero(e & far) >= 30, (kind, side)
        if kind.startswith("diag"):  # through the corner: a staircase, at least two of the four corner pixels
            assert np.count_nonzero(e[31:33, 63:65]) >= 2, (kind, side)
        elif kind == "vseam":
            assert e[:, 63].any() and e[:, 64].any()
        else:
            assert e[31, :].any() and e[32, :].any()
        # everything beyond the crossing is an edge only through the crossing: it is one component with the seed
        ys, xs = np.nonzero(plane == C.SEED_VALUE)
        seed_px = next((y, x) for y in range(ys.min() - 1, ys.max() + 2) for x in range(xs.min() - 1, xs.max() + 2) if e[y, x])
        assert np.array_equal(C.reach(e, seed_px), e), (kind, side)


@pytest.mark.parametrize("kind", sorted(C.PURE_DIAGONAL_EDITS))
def test_pure_diagonal_links(canny, kind):
    assert not canny(C.pure_diagonal(kind, None)[0]).any()
    for side in (0, 1):
        plane, near, far, pair, others = C.pure_diagonal(kind, side)
        e = canny(plane) != 0
        assert e[pair[0]] and e[pair[1]] and not e[others[0]] and not e[others[1]], (kind, side)
        # the far half hangs on the diagonal pair alone: without stepping on the near pixel of the pair, a walk from the far
        # one stays inside the far tile -- and it is not a stub
        beyond = C.reach(e, pair[1], blocked=pair[0])
        assert np.count_nonzero(beyond) >= 20 and not (beyond & ~far).any(), (kind, side)
        assert np.count_nonzero(e & near) >= 20


def test_density_sweep_brackets_the_candidate_switch(canny):
    sweep = C.density_sweep()
    assert len(sweep) >= 8
    counts = np.stack([C.tile_counts(canny(p)).ravel() for p in sweep.values()])
    assert counts.shape[1] == 4
    assert (counts.max(axis=1) < 64).any(), counts.tolist()      # a plane with every tile below 64
    assert (counts.min(axis=1) > 512).any(), counts.tolist()     # a plane with every tile above 512
    assert ((counts > 128) & (counts <= 256)).any() and ((counts > 256) & (counts < 512)).any(), counts.tolist()  # around 256
    assert ((counts.min(axis=1) <= 256) & (counts.max(axis=1) > 256)).any()  # both kinds of tile in one launch


def test_halo_and_walker_shapes(canny):
    halo = C.halo_cases()
    assert sorted(p.shape for p in halo.values()) == sorted([(40, 128), (40, 129), (40, 130), (40, 131), (32, 70), (33, 70),
                                                             (34, 70), (32, 64), (33, 65)])
    assert all(canny(p).any() for p in halo.values())
    for name, p in C.walker_cases().items():
        assert p.shape == (64, 1088)
        tc = C.tile_counts(canny(p))
        assert tc.shape == (2, 17) and np.count_nonzero(tc) == 34, name  # the third walker wavefront (tiles 32, 33) has work
    b = C.batch3()
    assert b.shape == (3, 133, 770) and (b[1] == 77).all()
    assert canny(b[0]).any() and not canny(b[1]).any() and np.count_nonzero(C.tile_counts(canny(b[2]))) >= 40


def test_magnitude_tops_out_at_2040(canny):
    """Each Sobel term of a byte plane is at most 4 * 255 = 1020 in magnitude, so |dx| + |dy| <= 2040: a high threshold of
    2040 or more leaves no strong pixel and the map is empty, whatever the low one is.  A diagonal step from 0 to 255 comes
    within one weight of the bound (3 * 255 per term) -- the thresholds are not out of reach by a wide margin."""
    tri = np.triu(np.full((16, 16), 255, np.uint8))
    gp = np.pad(tri.astype(np.int64), 1, mode="edge")
    dx = (gp[:-2, 2:] + 2 * gp[1:-1, 2:] + gp[2:, 2:]) - (gp[:-2, :-2] + 2 * gp[1:-1, :-2] + gp[2:, :-2])
    dy = (gp[2:, :-2] + 2 * gp[2:, 1:-1] + gp[2:, 2:]) - (gp[:-2, :-2] + 2 * gp[:-2, 1:-1] + gp[:-2, 2:])
    assert int((np.abs(dx) + np.abs(dy)).max()) == 1530
    assert canny(tri, 1000, 1529).any() and not canny(tri, 1000, 1530).any()
    for plane in (C.noise(133, 770, 3100), C.serpentine(133, 770, 20, "last"), tri):
        for low, high in ((0, 2040), (2039, 2040), (1, 5000)):
            assert not canny(plane, low, high).any(), (low, high)
        assert canny(plane, 0, 0).any()
