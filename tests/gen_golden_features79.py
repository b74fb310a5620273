"""Generate tests/golden/features79.npz: rows of the REAL feature_extraction.FeatureExtractor.extract_all_features.

TEST INFRASTRUCTURE, run by hand where the reference project is importable (its location: oracle/gen_golden.py's REF).
The module is imported with ``cv2`` and ``skimage`` stand-ins backed by tests/features79_ref.py's primitives (and
oracle.uwie_oracle's LAB / HSV / gray / Canny) and the real SciPy, so the fixture pins the reference's own glue: the
order of the 79 values, its slices, its float32 NumPy arithmetic, SciPy's NaN rule for skew / kurtosis and the dropped
DCT block of an odd-size frame (the stand-in dct raises there, as cv2.dct does).  The primitives themselves are held by
known-answer tests.  Only arrays travel: frame_<tag> (uint8) and row_<tag> (float64, 79 or 74 values).

Run:  python tests/gen_golden_features79.py
"""
from __future__ import annotations

import contextlib
import io
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", "oracle"))
sys.path.insert(0, HERE)
import features79_ref as R  # noqa: E402
import gen_golden as gg  # noqa: E402
from oracle import uwie_oracle as orc  # noqa: E402

OUT = os.path.join(HERE, "golden", "features79.npz")


def stand_ins():
    cv2 = types.ModuleType("cv2")
    cv2.COLOR_RGB2LAB, cv2.COLOR_RGB2HSV, cv2.COLOR_RGB2GRAY = "lab", "hsv", "gray"
    cv2.CV_32F, cv2.CV_64F = 5, 6
    cv2.cvtColor = lambda img, code: {"lab": orc.cv_rgb2lab_u8, "hsv": orc.cv_rgb2hsv_u8, "gray": orc.cv_rgb2gray_u8}[code](img)

    def resize(img, dsize):
        assert tuple(dsize) == (128, 128) and img.dtype == np.uint8
        return R.resize128(img)

    def dct(a):
        assert a.dtype == np.float32
        return R.dct2(a)

    def sobel(src, ddepth, dx, dy, ksize=3):
        assert ddepth == cv2.CV_32F and ksize == 3 and src.dtype == np.float32
        return R.sobel_f32(src, dx, dy)

    def laplacian(src, ddepth, ksize=1):
        assert ddepth == cv2.CV_64F and ksize == 3 and src.dtype == np.uint8
        return R.laplacian3(src)

    def canny(img, lo, hi):
        assert img.dtype == np.uint8
        return R.canny(img, lo, hi)

    cv2.resize, cv2.dct, cv2.Sobel, cv2.Laplacian, cv2.Canny = resize, dct, sobel, laplacian, canny

    sk = types.ModuleType("skimage")
    sk.__path__ = []
    feat = types.ModuleType("skimage.feature")

    def lbp(image, P, Rr, method="default"):
        assert (P, Rr, method) == (8, 1, "uniform")
        return R.local_binary_pattern_uniform(image)

    feat.local_binary_pattern, feat.graycomatrix, feat.graycoprops = lbp, R.graycomatrix, R.graycoprops
    meas = types.ModuleType("skimage.measure")
    meas.shannon_entropy = R.shannon_entropy
    mods = {"cv2": cv2, "skimage": sk, "skimage.feature": feat, "skimage.measure": meas,
            "skimage.color": types.ModuleType("skimage.color"), "skimage.filters": types.ModuleType("skimage.filters")}
    for name, m in mods.items():
        if "." in name:
            setattr(sk, name.split(".")[1], m)
    return mods


def import_feature_extraction():
    sys.dont_write_bytecode = True
    for name, m in stand_ins().items():
        sys.modules[name] = m
    sys.path.insert(0, gg.REF)
    import feature_extraction as fe  # noqa: E402
    sys.path.remove(gg.REF)
    return fe.FeatureExtractor


def frames():
    """tag -> uint8 frame: the cases the issue names (odd size, gray, constant, the 2x resize), each <= 96x128 but 256x256."""
    return {
        "underwater_96x128": R.frame("underwater", 96, 128, 1),
        "noise_64x80": R.frame("noise", 64, 80, 2),
        "hazy_90x120": R.frame("hazy", 90, 120, 3),
        "odd_37x53": R.frame("underwater", 37, 53, 4),
        "gray_48x64": R.frame("gray", 48, 64, 5),
        "const_32x48": R.frame("const", 32, 48, 6),
        "area2x_256x256": R.frame("underwater", 256, 256, 7),
        "row_1x96": R.frame("noise", 1, 96, 8),
    }


def main():
    FE = import_feature_extraction()
    out = {}
    for tag, u8 in frames().items():
        img = u8.astype(np.float32) / 255.0
        assert np.array_equal((img * 255).astype(np.uint8), u8)
        with contextlib.redirect_stdout(io.StringIO()) as log:
            row = np.asarray(FE.extract_all_features(img), dtype=np.float64)
        want = R.feature_count(*u8.shape[:2])
        assert row.shape == (want,), (tag, row.shape, log.getvalue())
        ref = R.features79(img)
        nan = np.isnan(row)
        assert np.array_equal(nan, np.isnan(ref)), tag
        assert np.allclose(row[~nan], ref[~nan], rtol=1e-6, atol=1e-9), (tag, np.abs(row - ref).max())
        out["frame_" + tag], out["row_" + tag] = u8, row
        print(f"{tag:18s} {row.size} values, {int(nan.sum())} NaN {log.getvalue().strip()[:60]}")
    np.savez_compressed(OUT, **out)
    print("wrote", OUT)


if __name__ == "__main__":
    main()
