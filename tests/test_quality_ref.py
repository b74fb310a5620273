"""tests/quality_ref.py (the float64 reference of the quality scores that tests/test_gpu_quality.py holds the device to)
pinned on the CPU: against ``oracle.quality_assessment`` on the frames of test_gpu_stages.py::test_quality_scores_match_oracle
within that test's 2e-3, and on frames whose scores are known in closed form."""
import numpy as np

import quality_ref as qr
from oracle import uwie_oracle as orc


def small_images():
    rng = np.random.default_rng(2025)
    yy, xx = np.mgrid[0:96, 0:130]
    smooth = 0.5 + 0.3 * np.sin(xx / 17.0) * np.cos(yy / 11.0)
    return {
        "random": rng.random((96, 130, 3)),
        "dark": rng.random((96, 130, 3)) * 0.3,
        "bright": 0.7 + rng.random((96, 130, 3)) * 0.3,
        "flat": np.full((64, 64, 3), 0.5),
        "binary": rng.choice([0.0, 1.0], size=(70, 90, 3)),
        "smooth": np.clip(smooth[:, :, None] * np.array([0.5, 0.8, 0.9]) + rng.normal(0, 0.01, (96, 130, 3)), 0, 1),
    }


def test_quality_ref_matches_the_float32_oracle():
    for name, img in small_images().items():
        img = img.astype(np.float32)
        u8 = (img * 255).astype(np.uint8)
        for weights in (None, {"contrast": 0.5, "entropy": 0.5}):
            # the float image given (comprehensive_assessment), and the frame as u8 / 255 (the batch form)
            for kind, got, want in (("f32", qr.scores(u8, img=img, weights=weights), qr.oracle_scores(u8, img=img, weights=weights)),
                                    ("u8", qr.scores(u8, weights=weights), qr.oracle_scores(u8, weights=weights))):
                d = np.abs(got - want)
                assert d.max() <= 2e-3, (name, kind, d)
                for i in (2, 5, 7):  # entropy, edge_density, naturalness: counts only, float64 in the oracle too
                    assert d[i] <= 1e-9, (name, kind, qr.KEYS[i], got[i], want[i])


def test_quality_ref_closed_forms():
    flat = np.full((12, 20, 3), 128, np.uint8)  # gray 128, S 0, LAB L of a mid gray, no edges, rg = yb = 0
    sc = qr.scores(flat)
    L = float(orc.cv_rgb2lab_u8(flat)[0, 0, 0])
    assert list(sc[:4]) == [0.0, 0.0, 0.0, 0.0] and sc[4] == 100 - abs(L - 128) / 128 * 100 and list(sc[5:8]) == [0.0, 0.0, 100.0]
    red = np.zeros((8, 8, 3), np.uint8)
    red[:, :, 0] = 255  # rg = 1, yb = 0.5 everywhere: 0.3 * sqrt(1.25) / 0.5 * 100; S = 255 everywhere: 100 and "over-saturated"
    sc = qr.scores(red)
    assert abs(sc[6] - 0.3 * np.sqrt(1.25) / 0.5 * 100) <= 1e-12 and sc[3] == 100.0 and sc[7] == 0.0
    yy, xx = np.mgrid[0:16, 0:16]
    checker = np.repeat((((yy + xx) & 1) * 255).astype(np.uint8)[:, :, None], 3, axis=2)
    sc = qr.scores(checker)  # two gray levels, half each: std 0.5, entropy 1 bit; |l| = 4 everywhere: var 16, clipped
    assert abs(sc[0] - 100.0) <= 1e-12 and sc[1] == 100.0 and sc[2] == 0.0
    assert np.array_equal(qr.laplacian_i64(checker[:, :, 0]), np.where((yy + xx) & 1, -1020, 1020))
    one = np.array([[[10, 200, 30]]], np.uint8)  # 1 x 1: every statistic of one value
    sc = qr.scores(one)
    assert np.isfinite(sc).all() and sc[0] == 0.0 and sc[1] == 0.0 and sc[2] == 0.0 and sc[5] == 0.0
    w = {"contrast": 0.5, "colorfulness": 2.0}
    assert qr.scores(red, weights=w)[8] == 0.5 * qr.scores(red)[0] + 2.0 * qr.scores(red)[6]


def test_bounds_come_from_the_recorded_distances():
    assert qr.bound("colorfulness", "f32") == 2 * qr.DISTANCE["f32"]["colorfulness"] <= 2e-3
    assert all(qr.bound(k) == 1e-9 for k in qr.KEYS) and all(qr.bound(k, "f32") == 1e-9 for k in qr.KEYS if k != "colorfulness")
    assert abs(qr.total_bound() - 1e-9) <= 1e-24 and max(max(v.values()) for v in qr.DISTANCE.values()) <= 2e-3
