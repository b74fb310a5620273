"""Canny's hysteresis on the device against the oracle's flood fill (oracle/cvref.c), byte for byte, on the patterns of
tests/canny_cases.py: contours that are edges only through one strong pixel many tiles away, links across tile seams and
through a tile corner (staircases and single diagonal pairs), tiles on both sides of the gathered-roots switch, the halo
load on both sides of its condition, list walkers in a third wavefront and a second block, regions of a batch.  Both routes:
the edge map (uwie_canny_u8: every candidate labelled) and the weak-only counts (FeatureExtractor's Canny density, the
quadtree's per-quadrant counts).  tests/test_canny_cases.py holds the preconditions that keep these from passing vacuously.
No tolerances anywhere: integers and bytes, and float64 quotients of the same integers.
"""
import numpy as np
import pytest

import canny_cases as C

pytestmark = pytest.mark.gpu

THRESHOLD_PAIRS = [(150, 50), (100, 100), (0, 0), (0, 2040), (2039, 2040), (1, 5000), (20, 60)]


@pytest.fixture(scope="module")
def dev():
    import underwater_image_enhancement_amd as uw

    return uw.get_device(0)


@pytest.fixture(scope="module")
def uw():
    import underwater_image_enhancement_amd as uw

    return uw


@pytest.fixture(scope="module")
def orc():
    from oracle import uwie_oracle

    return uwie_oracle


@pytest.fixture(scope="module")
def cases():
    return C.all_cases()


@pytest.fixture(scope="module")
def want(orc, cases):
    """The oracle's edge map of every case at (50, 150), computed once and left alone."""
    out = {name: orc.cv_canny_u8(p, 50, 150) for name, p in cases.items()}
    for e in out.values():
        e.setflags(write=False)
    return out


def same(got, want, tag=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype, (tag, got.dtype, want.dtype)
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got.ravel() != want.ravel())
        y, x = np.unravel_index(bad[0], got.shape)[-2:]
        raise AssertionError(f"{tag}: {bad.size} of {got.size} differ; first at {bad[0]} (row {y}, column {x}: tile row {y // C.TILE_H}, "
                             f"tile column {x // C.TILE_W}): got {got.ravel()[bad[0]]!r} want {want.ravel()[bad[0]]!r}")


def by_shape(names, cases):
    groups = {}
    for n in names:
        groups.setdefault(cases[n].shape, []).append(n)
    return groups


GROUPS = {
    "serpentine": lambda n: n.startswith("serp_"),
    "crossers": lambda n: n.startswith("cross_") or n.startswith("purediag_"),
    "density": lambda n: n.startswith("density_"),
    "halo": lambda n: n.startswith("halo_"),
    "walkers": lambda n: n.startswith("walk_") or n.startswith("batch3_"),
}


# ------------------------------------------------------------------------------------------------------------ edge map
@pytest.mark.parametrize("group", sorted(GROUPS))
def test_edge_map_matches_oracle(dev, cases, want, group):
    """uwie_canny_u8 at (50, 150): every case alone and in a batch with the cases of its shape -- the same bytes, the
    oracle's."""
    names = [n for n in cases if GROUPS[group](n)]
    assert names
    for shape, members in by_shape(names, cases).items():
        batch = dev.canny_u8(dev.tensor(np.stack([cases[n] for n in members])), 50, 150).cpu().numpy()
        for i, n in enumerate(members):
            same(batch[i], want[n], f"{n} (frame {i} of a batch of {len(members)})")
            single = dev.canny_u8(dev.tensor(cases[n][None]), 50, 150).cpu().numpy()[0]
            same(single, want[n], n)
    dev.check_status()


def test_edge_map_twice(dev, cases, want):
    """The union-find is racy by design (lock-free links, relaxed loads); its result must not be: serpentines and noise, twice
    more, in the other batch order."""
    names = [n for n in cases if n.startswith("serp_") or n.startswith("walk_") or n.startswith("batch3_") or n == "density_1"]
    for shape, members in by_shape(names, cases).items():
        members = members[::-1]
        planes = dev.tensor(np.stack([cases[n] for n in members]))
        for run in range(2):
            got = dev.canny_u8(planes, 50, 150).cpu().numpy()
            for i, n in enumerate(members):
                same(got[i], want[n], f"{n} (run {run})")
    dev.check_status()


def test_thresholds(dev, orc):
    """Other thresholds than (50, 150): low > high is swapped (as cv2.Canny does), low == high, zero, and pairs at and above
    the largest magnitude |dx| + |dy| = 2040 that bytes can give -- an empty map, on the oracle too."""
    planes = np.stack([C.noise(133, 770, 3100), C.serpentine(133, 770, 20, "last")])
    for low, high in THRESHOLD_PAIRS:
        wanted = np.stack([orc.cv_canny_u8(p, low, high) for p in planes])
        if high >= 2040:
            assert not wanted.any(), (low, high)
        else:
            assert wanted[0].any(), (low, high)
        got = dev.canny_u8(dev.tensor(planes), low, high).cpu().numpy()
        same(got, wanted, f"thresholds ({low}, {high})")
        same(dev.canny_u8(dev.tensor(planes[1:]), low, high).cpu().numpy(), wanted[1:], f"thresholds ({low}, {high}), single")
    swapped = dev.canny_u8(dev.tensor(planes), 150, 50).cpu().numpy()
    same(swapped, dev.canny_u8(dev.tensor(planes), 50, 150).cpu().numpy(), "swap")
    assert swapped[1].any()
    # (20, 60): the serpentine's straight runs (magnitude 80) are strong themselves now
    assert np.count_nonzero(orc.cv_canny_u8(C.serpentine(133, 770, 20, None), 20, 60)) > 10000
    dev.check_status()


# ------------------------------------------------------------------------------------------------ weak-only counts
def test_weak_only_counts_on_the_same_content(dev, uw, cases, want):
    """The counting route (only weak candidates are labelled; strong pixels are counted where they are found) on the same
    planes, as gray RGB frames: FeatureExtractor's Canny density must be the oracle's count / (H W), and the count of the
    device's own edge map.  For R = G = B the gray byte is the byte itself (the coefficients add up to one)."""
    names = [n for n in cases if n.startswith(("serp_", "cross_", "purediag_", "batch3_", "walk_"))]
    assert any(not want[n].any() for n in names) and any(np.count_nonzero(want[n]) > 10000 for n in names)
    for (H, W), members in by_shape(names, cases).items():
        planes = np.stack([cases[n] for n in members])
        rgb = C.gray_rgb(planes)
        same(dev.rgb2gray_u8(dev.tensor(rgb)).cpu().numpy(), planes, f"gray of R = G = B at {H}x{W}")
        col = uw.feature_extractor_keys(H, W).index("canny_density")
        rows = uw.feature_extractor_rows(rgb)
        own = dev.canny_u8(dev.tensor(planes), 50, 150).cpu().numpy()
        for i, n in enumerate(members):
            count = int(np.count_nonzero(want[n]))
            assert rows[i, col] == count / (H * W), (n, rows[i, col] * H * W, count)
            assert int(np.count_nonzero(own[i])) == count, n
            one = uw.feature_extractor_rows(rgb[i])
            assert one[col] == count / (H * W), (n, "single", one[col] * H * W, count)
        dev.check_status()


# ------------------------------------------------------------------------------------------------------- quadrants
def quadrant_frame(quads):
    """A gray RGB frame from four equal planes, in the quadtree's order: top-left, top-right, bottom-left, bottom-right."""
    return C.gray_rgb(np.block([[quads[0], quads[1]], [quads[2], quads[3]]]))


def quadrant_planes(H, W):
    return {"B": C.serpentine(H, W, 20, "last"), "A": C.serpentine(H, W, 20, None), "flat": np.full((H, W), C.FLAT, np.uint8),
            "dark": np.full((H, W), 40, np.uint8), "noise": C.noise(H, W, 4000 + W)}


@pytest.mark.parametrize("order,qw,prepass", [(("B", "A", "flat", "noise"), 770, 1), (("noise", "flat", "A", "B"), 770, 1),
                                              (("B", "A", "flat", "noise"), 771, 1), (("B", "A", "flat", "noise"), 770, 0),
                                              (("dark", "noise", "dark", "B"), 770, 1), (("B", "dark", "noise", "dark"), 771, 0)])
def test_quadrant_counts(dev, orc, order, qw, prepass):
    """The quadtree's per-quadrant Canny (four regions per frame in one launch, each its own image) on a 266 x 2 qw frame
    whose quadrants are {serpentine B, serpentine A, flat, noise}: the trace against the oracle's, level by level, bit for
    bit.  qw = 771: W % 8 != 0, the pre-pass is k_canny_strong instead of the fused gray / histogram sweeps; prepass = 0: no
    pre-pass at all, the unseeded serpentine goes through the component kernels and must still count nothing.  The last two
    orders make serpentine B the brightest quadrant, so the walk goes on INTO it: sub-quadrants whose tile grid starts at an
    odd offset of the frame and whose contour is cut from its seed by the quadrant border."""
    import torch

    planes = quadrant_planes(133, qw)
    u8 = quadrant_frame([planes[k] for k in order])
    assert u8.shape == (266, 2 * qw, 3) and (2 * qw) % 8 == (4 if qw == 770 else 6)
    x = orc.normalise_u8(u8)
    assert orc.classify_cast(x) == "normal"
    assert np.array_equal(orc.quantise_u8(x), u8)  # the quadtree's own gray plane is these bytes
    trace = []
    want_A = orc.atmospheric_light(x, 1, trace=trace)
    # what the oracle's level 0 must show: nothing in the unseeded quadrant, the whole contour in the seeded one
    n = 133 * qw
    terms = [orc.quality_score(x[qy:qy + 133, qx:qx + qw])[1] for qy in (0, 133) for qx in (0, qw)]
    for k, t in zip(order, terms):
        count = int(np.count_nonzero(orc.cv_canny_u8(planes[k], 50, 150)))
        assert t[3] == count / n, (k, t[3] * n, count)
        assert (count == 0) == (k in ("A", "flat", "dark")) and (k != "B" or count > 10000), (k, count)
    assert trace[0][:4] == (0, 0, 266, 2 * qw) and trace[0][4] == [float(t[0] + t[1] - t[2] - t[3]) for t in terms]
    if "dark" in order:  # the walk enters serpentine B and meets edges again below
        assert trace[1][:4] == (133 * (order.index("B") // 2), qw * (order.index("B") % 2), 133, qw)
    kk = torch.zeros(1, dtype=torch.int32, device=dev.torch_device)
    with dev.tuning(canny_prepass=prepass):
        A, tr = dev.atmospheric_light(dev.tensor(u8[None]), kk, trace=True)
        A2 = dev.atmospheric_light(dev.tensor(u8[None]), kk)  # the untraced route (histogram decisions where they separate)
    for lvl, (y0, x0, rows, cols, scores) in enumerate(trace):
        rec = tr[0, lvl]
        assert (rec["y0"], rec["x0"], rec["rows"], rec["cols"]) == (y0, x0, rows, cols), (order, lvl)
        same(rec["score"], np.array(scores, np.float64), f"{order} level {lvl}")
    assert tr[0, len(trace)]["rows"] == 0
    same(A[0].cpu().numpy(), np.asarray(want_A))
    same(A2[0].cpu().numpy(), np.asarray(want_A))
    dev.check_status()
