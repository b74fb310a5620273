"""uwie_feature_extractor_u8 held to float64 (tests/fx_cases.py):

  A  every index outside 57-61 against features79_ref.features79_f64 at 1e-9 relative + 1e-12, on frames where one pixel or one
     histogram count moves a value by ten tolerances (tests/test_fx_cases.py)
  B  k_fx_maps's own RGB -> LAB and RGB -> HSV on all 2^24 colours, twice (slabs by red byte, and shuffled), through the colour
     block; and k_quality.hip's HSV copy through the saturation score
  C  the DCT through indices 57-61 on basis frames (one coefficient) and impulse frames (one input position), at
     max(2e-5 |w| + 1e-9, 4 |NumPy float32 evaluation - float64|)

Each test prints the largest distance it measured, in tolerance units, before it asserts.
"""
import numpy as np
import pytest

import features79_ref as R
import fx_cases as F
import quality_ref as qr
from oracle import uwie_oracle as orc

pytestmark = pytest.mark.gpu

GROUPS = {"colour": range(0, 35), "texture": range(35, 57), "edge": range(62, 69), "quality": range(69, 79)}


@pytest.fixture(scope="module")
def uw():
    import underwater_image_enhancement_amd as uw

    return uw


@pytest.fixture(scope="module")
def dev(uw):
    return uw.get_device(0)


def same_bits(a, b, what):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    assert a.shape == b.shape and a.tobytes() == b.tobytes(), what


def hold(got, want, tag, worst, indices=None):
    bad = []
    for name, idx in GROUPS.items():
        sel = set(idx) if indices is None else set(idx) & set(indices)
        b, w = F.row_failures(got, want, indices=sel, tag=tag)
        bad += b
        worst[name] = max(worst.get(name, 0.0), w)
    return bad


def report(what, worst):
    print(f"{what}: largest |device - float64| in tolerance units (1e-9 |w| + 1e-12): "
          + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))


# ---------------------------------------------------------------------------------------------------------------- A
def test_rows_against_the_float64_statement(uw, dev):
    worst, bad = {}, []
    for tag, u8 in F.row_frames():
        got = uw.feature_extractor_rows(u8)
        assert got.size == R.feature_count(*u8.shape[:2])
        bad += hold(got, R.features79_f64(u8), tag, worst)
    report("row frames", worst)
    assert not bad, "; ".join(bad)
    dev.check_status()


def test_a_batch_of_three_and_a_float_image(uw, dev):
    worst, bad = {}, []
    frames = F.batch3()
    rows = uw.feature_extractor_rows(frames)
    for i, u8 in enumerate(frames):
        bad += hold(rows[i], R.features79_f64(u8), f"batch3[{i}]", worst)
        same_bits(uw.feature_extractor_rows(u8), rows[i], f"batch3[{i}] alone")
    img = F.float_image()
    got = uw.FeatureExtractor.extract_all_features(img)
    bad += hold(got, R.features79_f64(img), "float image", worst)
    assert got[[25, 26, 33, 34]].tolist() == [float(img[:, :, 0].min()), float(img[:, :, 0].max()), float(img[:, :, 2].min()),
                                               float(img[:, :, 2].max())]
    report("batch of three, float image", worst)
    assert not bad, "; ".join(bad)
    dev.check_status()


def test_sparse_frames(uw, dev):
    """a flat frame with one pixel raised: the Sobel, Laplacian and LBP values rest on that pixel's neighbourhood alone."""
    worst, bad = {}, []
    tags, frames = F.sparse_frames()
    rows = uw.feature_extractor_rows(frames)
    for i, tag in enumerate(tags):
        bad += hold(rows[i], R.features79_f64(frames[i]), "sparse " + tag, worst)
    for i in (0, len(tags) // 2, len(tags) - 1):
        same_bits(uw.feature_extractor_rows(frames[i]), rows[i], "sparse " + tags[i] + " alone")
    report("sparse frames", worst)
    assert not bad, "; ".join(bad)
    dev.check_status()


# ---------------------------------------------------------------------------------------------------------------- B
@pytest.mark.parametrize("shuffled", [False, True], ids=["by red byte", "shuffled"])
def test_colour_block_on_all_colours(uw, dev, shuffled):
    slabs = F.slabs(shuffled).copy()  # (the cases are read-only)
    rows = uw.feature_extractor_rows(slabs)
    assert rows.shape == (256, 79)
    worst, bad = {}, []
    lift = (np.arange(256, dtype=np.float32) / np.float32(255.0)).astype(np.float64)
    sat = np.empty(256)
    for r in range(256):
        lab, hsv, img = F.planes(slabs[r])
        want = np.full(79, np.nan)
        want[list(F.COLOUR_BLOCK)] = F.colour_block(lab, hsv, img)
        bad += hold(rows[r], want, f"slab {r}", worst, indices=F.COLOUR_BLOCK)
        sat[r] = np.clip(lift[hsv[:, :, 1]].mean() * 100.0, 0.0, 100.0)
    for r in (0, 77, 255):
        same_bits(uw.feature_extractor_rows(slabs[r]), rows[r], f"slab {r} alone")
    report("cube " + ("shuffled" if shuffled else "by red byte"), {k: v for k, v in worst.items() if k in ("colour", "quality")})
    assert not bad, "; ".join(bad[:20])
    if shuffled:  # k_quality.hip's copy of RGB -> HSV, through the saturation score and the bound test_gpu_quality holds it to
        q = uw.quality_scores(slabs)
        d = np.abs(q[:, 3] - sat)
        print(f"quality saturation score on the shuffled slabs: largest |device - float64| = {d.max():.3g} (bound {qr.bound('saturation'):g})")
        assert d.max() <= qr.bound("saturation"), int(d.argmax())
    dev.check_status()


# ---------------------------------------------------------------------------------------------------------------- C
@pytest.fixture(scope="module")
def dct_cases():
    batches = F.dct_batches()
    return {s: (cases, frames, F.dct_reference(frames)) for s, (cases, frames) in batches.items()}


def test_dct_one_output_and_one_input_at_a_time(uw, dev, dct_cases):
    worst, bad = {"basis": 0.0, "impulse": 0.0, "mirror": 0.0}, []
    for (H, W), (cases, frames, (want, tolerance, _)) in dct_cases.items():
        rgb = F.gray_rgb(frames)
        rows = uw.feature_extractor_rows(rgb)
        assert rows.shape == (len(cases), 79)
        u = F.dct_units(rows[:, 57:62], want, tolerance)
        for i, c in enumerate(cases):
            worst[c.kind] = max(worst[c.kind], u[i].max())
            if u[i].max() > 1.0:
                bad.append(f"{H}x{W} {c}: got {rows[i, 57:62]!r} want {want[i]!r} ({u[i].max():.3g} tolerances)")
        for i in (0, len(cases) // 3, len(cases) - 1):
            same_bits(uw.feature_extractor_rows(rgb[i]), rows[i], f"{H}x{W} {cases[i]} alone")
    print("DCT: largest |device - float64| in tolerance units: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    assert not bad, f"{len(bad)} cases: " + "; ".join(bad[:10])
    dev.check_status()
