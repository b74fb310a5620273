"""The preconditions of tests/fx_cases.py, on the CPU: the float64 statement agrees with the float32 reference to the old bounds,
every frame resolves a single pixel, a single histogram count and a single DCT term at ten times the tolerance it is held to,
the cube sets hold every colour once, and the mutations the cases are there for are caught by the cases' own checkers."""
import numpy as np
import pytest

import features79_ref as R
import fx_cases as F
from oracle import uwie_oracle as orc


@pytest.fixture(scope="module")
def batches():
    return F.dct_batches()


@pytest.fixture(scope="module")
def references(batches):
    return {s: F.dct_reference(fr) for s, (_, fr) in batches.items()}


# ---------------------------------------------------------------------------------------------------------------- A
def test_f64_statement_agrees_with_the_reference_on_the_golden_frames():
    with np.load(F.GOLDEN, allow_pickle=False) as z:
        rows = {k[4:]: z[k] for k in z.files if k.startswith("row_")}
    for tag, u8 in F.golden_frames():
        got = R.features79_f64(u8)
        F.assert_row_f32(got, rows[tag], tag + " (fixture)")
        F.assert_row_f32(got, R.features79(u8.astype(np.float32) / 255.0), tag)
    img = F.float_image()
    assert not np.array_equal((img * 255).astype(np.uint8).astype(np.float32) / np.float32(255), img)
    F.assert_row_f32(R.features79_f64(img), R.features79(img), "float image")


def test_groups_are_slices_of_the_f64_row():
    u8 = R.frame("underwater", 24, 40, seed=2)
    row = R.features79_f64(u8)
    assert row.shape == (79,)
    assert np.array_equal(R.features79_f64(u8, groups=("color", "quality")), np.r_[row[:35], row[69:]])
    lab, hsv, img = F.planes(u8)
    assert np.array_equal(F.colour_block(lab, hsv, img), row[list(F.COLOUR_BLOCK)])


def a_frames():
    frames = F.row_frames() + [(f"batch3[{i}]", f) for i, f in enumerate(F.batch3())] + [("float image", F.float_image())]
    tags, sparse = F.sparse_frames()
    return frames + [("sparse " + t, f) for t, f in zip(tags, sparse)]


def test_every_row_frame_resolves_one_pixel_and_one_histogram_count():
    """one pixel raised by one gray level, and one count moved to the neighbouring bin of each of the nine colour
    histograms, each move some compared value by more than ten tolerances."""
    rng = np.random.default_rng(41)
    seen_shapes = set()
    for tag, frame in a_frames():
        seen_shapes.add(frame.shape[:2])
        lab, hsv, img = F.planes(frame)
        base = F.colour_block(lab, hsv, img)
        for name, l2, h2, i2 in F.histogram_moves(lab, hsv, img, rng):
            assert F.moved(base, F.colour_block(l2, h2, i2)) > 10.0, (tag, name)
        u8 = frame if frame.dtype == np.uint8 else (frame * 255).astype(np.uint8)
        g = orc.cv_rgb2gray_u8(u8)
        y, x = int(rng.integers(g.shape[0])), int(rng.integers(g.shape[1]))
        g2 = g.copy()
        g2[y, x] += 1 if g2[y, x] < 255 else -1
        s = hsv[:, :, 1].astype(np.uint8)
        a = np.r_[R.edge_f64(g, with_canny=False), R.quality_f64(g, s)]
        b = np.r_[R.edge_f64(g2, with_canny=False), R.quality_f64(g2, s)]
        assert F.moved(a, b) > 10.0, tag
    assert {(512, 514), (1026, 256), F.SPARSE_SHAPE} <= seen_shapes


def test_sparse_frames_are_what_they_claim():
    tags, frames = F.sparse_frames()
    H, W = F.SPARSE_SHAPE
    assert (H * W) % 256 and H % 2 == 0 and W % 2 == 0
    where = set()
    for f in frames:
        raised = np.argwhere(np.any(f != np.array(F.SPARSE_FLAT, np.uint8), axis=2))
        assert raised.shape == (1, 2)
        where.add(tuple(raised[0]))
    assert {(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)} <= where
    assert {y * W + x for y, x in where} >= {255, 256, 257, H * W - 1}
    assert {y for y, _ in where} >= {0, 1, H - 2, H - 1} and {x for _, x in where} >= {0, 1, W - 2, W - 1}
    # a gray frame goes through RGB2GRAY unchanged (part C relies on it)
    g = np.arange(256, dtype=np.uint8).reshape(16, 16)
    assert np.array_equal(orc.cv_rgb2gray_u8(F.gray_rgb(g)), g)


# ---------------------------------------------------------------------------------------------------------------- B
@pytest.mark.parametrize("shuffled", [False, True])
def test_slab_sets_hold_every_colour_once(shuffled):
    s = F.slabs(shuffled)
    assert s.shape == (256, 256, 256, 3) and s.dtype == np.uint8
    idx = F.cc.colour_index(s)
    assert np.array_equal(np.bincount(idx, minlength=1 << 24), np.ones(1 << 24, np.int64))
    if not shuffled:
        assert np.all(s[:, :, :, 0] == np.arange(256, dtype=np.uint8)[:, None, None])
        assert np.all(s[7, :, :, 1] == np.arange(256, dtype=np.uint8)[:, None]) and np.all(s[7, :, :, 2] == np.arange(256, dtype=np.uint8))
    else:
        assert not np.array_equal(s, F.slabs(False))


def test_one_byte_of_a_slab_moves_the_colour_block():
    rng = np.random.default_rng(42)
    for shuffled in (False, True):
        s = F.slabs(shuffled)
        for r in rng.integers(0, 256, 6):
            lab, hsv, img = F.planes(s[r])
            base = F.colour_block(lab, hsv, img)
            moves = [m for m in F.histogram_moves(lab, hsv, img, rng) if m[0] in "LabHSV"]
            assert len(moves) == 6
            for name, l2, h2, i2 in moves:
                assert F.moved(base, F.colour_block(l2, h2, i2)) > 10.0, (shuffled, int(r), name)


def test_hsv_restatement_is_the_oracle_and_an_off_by_one_constant_is_caught():
    """The NumPy statement of RGB2HSV equals the oracle on the whole cube; with one constant off by one, the colour block of
    some slab leaves the bound (the mutation the cube case is there for)."""
    px = F.cc.cube_pixels()
    want = orc.cv_rgb2hsv_u8(px.reshape(4096, 4096, 3)).reshape(-1, 3)
    assert np.array_equal(F.hsv_numpy(px), want)
    for kw in ({"half": (1 << 11) - 1}, {"sat_scale": 254}, {"hrange": 179}):
        for r in (255, 128, 37):
            s = F.slabs(False)[r]
            lab, hsv, img = F.planes(s)
            wrong = F.hsv_numpy(s, **kw)
            if np.array_equal(wrong, hsv):
                continue
            bad, _ = F.row_failures(_as_row(F.colour_block(lab, wrong, img)), _as_row(F.colour_block(lab, hsv, img)), indices=F.COLOUR_BLOCK)
            assert bad, (kw, r)
            break
        else:
            raise AssertionError(f"{kw} changes no byte of the sampled slabs")


def _as_row(block):
    row = np.zeros(79)
    row[list(F.COLOUR_BLOCK)] = block
    return row


def test_a_clamped_border_is_caught_by_the_sparse_frames(monkeypatch):
    """reflect101 replaced by a clamp, stated in NumPy: the Sobel / Laplacian values of the border cases leave the bound."""
    tags, frames = F.sparse_frames()
    g = [orc.cv_rgb2gray_u8(f) for f in frames]
    good = [R.edge_f64(x, with_canny=False) for x in g]
    monkeypatch.setattr(R, "_reflect101", lambda i, n: np.clip(i, 0, n - 1))
    caught = [t for t, x, w in zip(tags, g, good) if F.moved(w, R.edge_f64(x, with_canny=False)) > 1.0]
    assert any(t.startswith("corner") for t in caught) and any(t.startswith("border") for t in caught), caught
    assert not any(t.startswith("seam") for t in caught)


# ---------------------------------------------------------------------------------------------------------------- C
def test_dct_batches_cover_the_lengths_and_positions(batches):
    for N in F.DCT_LENGTHS:
        for shape, axis in (((N, 6), 0), ((6, N), 1)):
            cases = [c for c in batches[shape][0] if c.kind == "basis"]
            along = {(c.a, c.b)[axis] for c in cases}
            across = {(c.b, c.a)[axis] for c in cases}
            assert along == set(range(N)) and across >= {0, 1, 5}, shape
    assert {(N + 1) // 2 for N in F.DCT_LENGTHS} >= {63, 64, 65, 127, 128, 129}
    assert {(N // 2) % 4 for N in F.DCT_LENGTHS} == {0, 1, 2, 3}
    for shape in F.DCT_SQUARES + F.IMPULSE_SHAPES:
        assert shape in batches
    for (H, W), (cases, frames) in batches.items():
        assert frames.shape == (len(cases), H, W) and frames.dtype == np.uint8
        for c, g in zip(cases, frames):
            if c.kind == "impulse":
                assert np.count_nonzero(g) == 1 and g[c.a, c.b] == 255
            elif c.kind == "mirror":
                assert np.count_nonzero(g) == 2 and g[c.a, c.b] == 255
                assert g[(H - 1 - c.a, c.b) if c.axis == 0 else (c.a, W - 1 - c.b)] == 100
    assert any(c.kind == "impulse" for c in batches[(1, 130)][0]) and any(c.kind == "impulse" for c in batches[(130, 1)][0])
    assert sum(len(c) for c, _ in batches.values()) < 8000 and max(f[0].size for _, f in batches.values()) <= 258 * 130


def test_the_split_statement_is_the_dct(batches, references):
    """the even / odd split with the 4N-entry table, in float64, is the transform: the model the mutations are stated in."""
    for shape, (_, frames) in batches.items():
        want, tolerance, _ = references[shape]
        assert F.dct_units(R.dct_values(F.dct_split(frames)), want, tolerance).max() < 0.1, shape


def test_basis_cases_resolve_their_coefficient(batches, references):
    """condition 1: the reference's coefficient (k, c) scaled by 1 + 1e-3 moves one of the five values by more than 10 of
    the tolerances it is held to, and that value is not one the raised floor applies to."""
    lowest = np.inf
    for shape, (cases, frames) in batches.items():
        sel = [i for i, c in enumerate(cases) if c.kind == "basis" and (c.a, c.b) != (0, 0)]
        if not sel:
            continue
        want, tolerance, raised = (x[sel] for x in references[shape])
        d = F.dct_planes(frames[sel])
        b = np.arange(len(sel))
        d[b, [cases[i].a for i in sel], [cases[i].b for i in sel]] *= 1.0 + 1e-3
        u = np.where(raised, 0.0, F.dct_units(R.dct_values(d), want, tolerance)).max(axis=1)
        lowest = min(lowest, u.min())
        assert u.min() > 10.0, (shape, cases[sel[int(u.argmin())]], u.min())
    print(f"basis cases: the scaled coefficient moves a value by at least {lowest:.3g} tolerances")


def sampled_lines(N):
    K = N // 2
    return sorted({k for k in (0, 1, 2, K - 1, K, N - 2, N - 1, 63, 64, 65) if 0 <= k < N})


def test_impulse_cases_resolve_an_output_line(batches, references):
    """condition 2.  The five values are even in d, so a negated output row moves none of them whatever the frame; what an
    impulse frame resolves is an output row (column) that is LOST (a padding lane or a mask that drops it) and, on a mirror
    pair, an output row computed from the sum where the difference belongs (the partner's term negated).  Every sampled row
    and column on which the impulse's basis function is at least 1 / 4 of its peak moves a value by more than 10 tolerances
    when zeroed; so does every such line of a mirror pair when the partner's sign is turned."""
    lowest = np.inf
    for shape in F.IMPULSE_SHAPES:
        cases, frames = batches[shape]
        H, W = shape
        want, tolerance, raised = references[shape]
        d0 = F.dct_planes(frames)
        CH, CW = F.cos_matrix(H), F.cos_matrix(W)
        for i, c in enumerate(cases):
            if c.kind == "basis":
                continue
            n_checked = 0
            for axis, N, C, p in ((0, H, CH, c.a), (1, W, CW, c.b)):
                if N == 1:
                    continue
                for k in sampled_lines(N):
                    if abs(C[k, p]) < 0.25 * np.sqrt(2.0 / N):
                        continue
                    d = d0[i].copy()
                    if axis == 0:
                        d[k, :] = 0.0
                    else:
                        d[:, k] = 0.0
                    u = np.where(raised[i], 0.0, F.dct_units(R.dct_values(d), want[i], tolerance[i])).max()
                    lowest = min(lowest, u)
                    assert u > 10.0, (shape, c, axis, k, u)
                    n_checked += 1
                    if c.kind == "mirror" and c.axis == axis and k % 2 == 1:
                        g = frames[i].astype(np.float64)
                        wrong = np.where(g == 100, -g, g)  # the difference x_n - x_{N-1-n} taken as the sum, in line k
                        dw = CH @ wrong @ CW.T
                        d = d0[i].copy()
                        if axis == 0:
                            d[k, :] = dw[k, :]
                        else:
                            d[:, k] = dw[:, k]
                        u = np.where(raised[i], 0.0, F.dct_units(R.dct_values(d), want[i], tolerance[i])).max()
                        assert u > 10.0, (shape, c, axis, k, "sum for difference", u)
            assert n_checked >= 3, (shape, c)
    print(f"impulse cases: a lost output line moves a value by at least {lowest:.3g} tolerances")


def test_the_raised_floor_is_rare(references):
    """condition 3: the raised floor applies to at most 1 % of the compared values."""
    n = sum(r[0].size for r in references.values())
    k = sum(int(r[2].sum()) for r in references.values())
    worst = max(float((r[1] / (F.DCT_RTOL * np.abs(r[0]) + F.DCT_FLOOR))[r[2]].max()) for r in references.values() if r[2].any())
    print(f"raised floor on {k} of {n} values, at most {worst:.3g} plain tolerances")
    assert k <= 0.01 * n


def dct_failures(batches, references, values_of, only=None):
    out = []
    for shape, (cases, frames) in batches.items():
        if only is not None and shape not in only:
            continue
        want, tolerance, _ = references[shape]
        u = F.dct_units(values_of(frames), want, tolerance)
        out += [(shape, cases[i]) for i in np.flatnonzero(u.max(axis=1) > 1.0)]
    return out


def test_dct_mutations_are_caught(batches, references):
    """A table index stepped once too often for one ni, and k < h4 turned into k <= h4, stated in NumPy: cases fail."""
    for ni in range(4):
        for ax in (1, 2):
            def step(axis, m, k, n, ni=ni, ax=ax):  # outputs at positions 16 ni .. 16 ni + 15 of their 64-wide block: one more 8k
                h = k // 2
                return np.where((axis == ax) & ((h % 64) // 16 == ni) & (n >= 4), m + 8 * k, m)

            bad = dct_failures(batches, references, lambda fr: R.dct_values(F.dct_split(fr, step)), only=F.DCT_SQUARES + F.IMPULSE_SHAPES)
            assert any(c.kind == "basis" for _, c in bad) and any(c.kind != "basis" for _, c in bad), (ni, ax)

    def regions_le(frames):
        d = F.dct_planes(frames)
        v = R.dct_values(d)
        h, w = d.shape[1:]
        e = d * d
        v[:, 0] = e[:, :h // 4 + 1, :w // 4].sum(axis=(1, 2)) / e.sum(axis=(1, 2))  # k <= h4
        return v

    bad = dct_failures(batches, references, regions_le)
    assert {s for s, c in bad if c.kind == "basis"} >= {(N, 6) for N in F.DCT_LENGTHS if N >= 4}
    for N in F.DCT_LENGTHS[1:]:
        assert ((N, 6), F.DctCase("basis", N // 4, 0, -1)) in bad, N
