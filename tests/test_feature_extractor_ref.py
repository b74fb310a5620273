"""CPU checks of tests/features79_ref.py, the restatement the device FeatureExtractor is tested against: it reproduces the
real reference's rows (tests/golden/features79.npz) and its primitives pass known-answer tests.  No GPU needed."""
import math
import os

import numpy as np
import pytest

import features79_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def golden79():
    with np.load(os.path.join(HERE, "golden", "features79.npz")) as z:
        return {k[6:]: (z[k], z["row_" + k[6:]]) for k in z.files if k.startswith("frame_")}


def test_restatement_reproduces_the_reference_rows(golden79):
    assert len(golden79) == 8
    for tag, (u8, row) in golden79.items():
        got = R.features79(u8.astype(np.float32) / 255.0)
        assert got.shape == row.shape == (R.feature_count(*u8.shape[:2]),), tag
        nan = np.isnan(row)
        assert np.array_equal(np.isnan(got), nan), tag
        np.testing.assert_allclose(got[~nan], row[~nan], rtol=1e-6, atol=1e-9, err_msg=tag)


def test_golden_covers_the_named_cases(golden79):
    rows = {t: r for t, (_, r) in golden79.items()}
    assert rows["odd_37x53"].size == 74
    assert np.flatnonzero(np.isnan(rows["gray_48x64"])).tolist() == [6, 7, 10, 11]  # a, b planes constant (128)
    assert np.flatnonzero(np.isnan(rows["const_32x48"])).tolist() == [2, 3, 6, 7, 10, 11]
    assert rows["gray_48x64"][18] > 1e10  # CCF = M / (0 + 1e-10)
    assert golden79["area2x_256x256"][0].shape[:2] == (256, 256)


def _lbp_scalar(g, r, c):
    """skimage's per-pixel loop, scalar Python floats (IEEE double, no fusing)."""
    H, W = g.shape
    centre = float(g[r, c])
    bits = []
    for i in range(8):
        rp = round(-math.sin(2 * math.pi * i / 8), 5)
        cp = round(math.cos(2 * math.pi * i / 8), 5)
        rr, cc = r + rp, c + cp
        minr, minc, maxr, maxc = math.floor(rr), math.floor(cc), math.ceil(rr), math.ceil(cc)
        dr, dc = rr - minr, cc - minc

        def px(y, x):
            return float(g[y, x]) if 0 <= y < H and 0 <= x < W else 0.0

        top = (1 - dc) * px(minr, minc) + dc * px(minr, maxc)
        bottom = (1 - dc) * px(maxr, minc) + dc * px(maxr, maxc)
        bits.append(1 if (1 - dr) * top + dr * bottom - centre >= 0 else 0)
    changes = sum(bits[i] != bits[i + 1] for i in range(7))
    return sum(bits) if changes <= 2 else 9


@pytest.mark.parametrize("shape", [(3, 3), (4, 4)])
def test_lbp_known_answers(shape):
    rng = np.random.default_rng(11)
    patterns = [np.full(shape, 7, np.uint8), np.zeros(shape, np.uint8), rng.integers(0, 4, shape).astype(np.uint8),
                rng.integers(0, 256, shape).astype(np.uint8)]
    peak = np.zeros(shape, np.uint8)
    peak[1, 1] = 200
    pit = np.full(shape, 10, np.uint8)
    pit[1, 1] = 0
    patterns += [peak, pit]
    for g in patterns:
        got = R.local_binary_pattern_uniform(g)
        want = np.array([[_lbp_scalar(g, r, c) for c in range(shape[1])] for r in range(shape[0])], np.float64)
        assert np.array_equal(got, want), g
    assert R.local_binary_pattern_uniform(peak)[1, 1] == 0  # every sample below the centre
    assert R.local_binary_pattern_uniform(pit)[1, 1] == 8  # every sample at or above it (interior pixel of the 3x3 / 4x4)
    # a flat patch's border pixels see the constant-0 outside: never all 8 bits
    assert R.local_binary_pattern_uniform(np.full(shape, 7, np.uint8))[0, 0] != 8


def test_glcm_props_of_a_four_level_image_against_direct_sums():
    rng = np.random.default_rng(3)
    img = rng.integers(0, 4, (6, 7)).astype(np.uint8)
    angles = [0, np.pi / 4, np.pi / 2, 3 * np.pi / 4]
    P = R.graycomatrix(img, [1], angles, levels=4, symmetric=True, normed=True)
    for a, (dr, dc) in enumerate(R.GLCM_OFFSETS):
        C = np.zeros((4, 4))
        for r in range(6):
            for c in range(7):
                if 0 <= r + dr < 6 and 0 <= c + dc < 7:
                    C[img[r, c], img[r + dr, c + dc]] += 1
        C = C + C.T
        C /= C.sum()
        assert np.allclose(P[:, :, 0, a], C, rtol=0, atol=1e-15)
        ii, jj = np.meshgrid(np.arange(4), np.arange(4), indexing="ij")
        mu = (C * ii).sum()
        var = (C * (ii - mu) ** 2).sum()
        want = {"contrast": (C * (ii - jj) ** 2).sum(), "dissimilarity": (C * abs(ii - jj)).sum(),
                "homogeneity": (C / (1 + (ii - jj) ** 2)).sum(), "ASM": (C ** 2).sum(), "energy": math.sqrt((C ** 2).sum()),
                "correlation": (C * (ii - mu) * (jj - mu)).sum() / var}
        for prop, v in want.items():
            assert R.graycoprops(P, prop)[0, a] == pytest.approx(v, rel=1e-12), prop
    assert R.graycoprops(R.graycomatrix(np.full((5, 5), 2, np.uint8), [1], angles, 4, True, True), "correlation").tolist() == [[1.0] * 4]


def test_dct_region_sums_against_a_direct_cosine_sum():
    rng = np.random.default_rng(5)
    H, W = 8, 12
    g = rng.integers(0, 256, (H, W)).astype(np.float32)

    def C(N):
        k, n = np.arange(N)[:, None], np.arange(N)[None, :]
        return np.where(k == 0, math.sqrt(1 / N), math.sqrt(2 / N)) * np.cos(np.pi * k * (2 * n + 1) / (2 * N))

    d = C(H) @ g.astype(np.float64) @ C(W).T
    got = R.dct2(g)
    assert np.allclose(got, d, rtol=1e-6, atol=1e-3)
    assert np.sum(got[:2, :3].astype(np.float64) ** 2) == pytest.approx(np.sum(d[:2, :3] ** 2), rel=1e-6)
    assert np.sum(got[4:, 6:].astype(np.float64) ** 2) == pytest.approx(np.sum(d[4:, 6:] ** 2), rel=1e-5)
    with pytest.raises(R.OddSizeDCT):
        R.dct2(np.zeros((5, 4), np.float32))
    assert np.array_equal(R.dct2(np.arange(6, dtype=np.float32)[None]).shape, (1, 6))  # a length-1 axis is the identity
    assert R.dct2(np.full((1, 1), 9, np.float32))[0, 0] == 9


def _resize_scalar(g, dy, dx):
    H, W = g.shape

    def tap(d, src):
        f = np.float32((d + 0.5) * (1.0 / (128.0 / src)) - 0.5)
        s = math.floor(f)
        f = np.float32(f - np.float32(s))
        if s < 0:
            f, s = np.float32(0), 0
        if s >= src - 1:
            f, s = np.float32(0), src - 1
        return s, min(s + 1, src - 1), int(np.rint((np.float32(1) - f) * np.float32(2048))), int(np.rint(f * np.float32(2048)))

    x0, x1, a0, a1 = tap(dx, W)
    y0, y1, b0, b1 = tap(dy, H)
    S0 = int(g[y0, x0]) * a0 + int(g[y0, x1]) * a1
    S1 = int(g[y1, x0]) * a0 + int(g[y1, x1]) * a1
    return min(max((((S0 >> 4) * b0 >> 16) + ((S1 >> 4) * b1 >> 16) + 2) >> 2, 0), 255)


def test_resize_known_answers():
    rng = np.random.default_rng(9)
    g = rng.integers(0, 256, (256, 256)).astype(np.uint8)
    got = R.resize128(g)
    s = g.astype(int)
    assert got[5, 7] == (s[10, 14] + s[10, 15] + s[11, 14] + s[11, 15] + 2) >> 2  # INTER_AREA fast path
    assert np.array_equal(R.resize128(g[:128, :128]), g[:128, :128])
    for shape in [(200, 300), (90, 120), (37, 53), (1, 96)]:
        g = rng.integers(0, 256, shape).astype(np.uint8)
        got = R.resize128(g)
        for dy, dx in [(0, 0), (127, 127), (5, 77), (64, 3), (100, 64)]:
            assert got[dy, dx] == _resize_scalar(g, dy, dx), (shape, dy, dx)
    assert np.array_equal(R.resize128(np.full((77, 300), 93, np.uint8)), np.full((128, 128), 93, np.uint8))
    # coefficient check of one upscale tap: scale 37 / 128, dx = 10 -> fx = float32(10.5 * scale - 0.5)
    f = np.float32(10.5 * (1.0 / (128.0 / 37)) - 0.5)
    assert math.floor(f) == 2 and int(np.rint((np.float32(1) - (f - np.float32(2))) * 2048)) == 952  # (1 - 0.53515625) * 2048


def test_odd_sizes_give_74_values_and_the_library_agrees():
    from underwater_image_enhancement_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    lib = _lib.load()
    for H, W in [(1, 1), (2, 2), (3, 5), (7, 128), (5, 7), (37, 53), (1, 96), (96, 1), (1080, 1920), (3, 4), (4, 3)]:
        assert lib.uwie_feature_extractor_count(H, W) == R.feature_count(H, W), (H, W)
    assert R.feature_count(3, 5) == 74 and R.feature_count(1, 1) == 79
    assert R.features79(R.frame("noise", 3, 5).astype(np.float32) / 255).size == 74
    assert lib.uwie_workspace_bytes_feature_extractor(0, 8, 8) == 0
    assert lib.uwie_feature_extractor_u8(None, None, None, 1, 8, 8, 15, None, None, 0, None) != 0


def test_feature_keys_name_the_79_values():
    import underwater_image_enhancement_amd as uw

    keys = uw.FEATURE_EXTRACTOR_KEYS
    assert len(keys) == 79 == len(set(keys))
    assert keys[35] == "lbp_0" and keys[57] == "dct_low" and keys[62] == "sobel_mean" and keys[78] == "rms_contrast"
