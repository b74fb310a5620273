"""Float64 reference of quality_assessment.QualityAssessment (quality_assessment.py:15-286) for the device's scores.

``oracle.uwie_oracle.quality_assessment`` restates the reference file as it runs: float32 images, NumPy's float32 pairwise
sums.  This module evaluates the same eight definitions from the oracle's INTEGER planes (``cv_rgb2gray_u8``,
``cv_rgb2hsv_u8``, ``cv_rgb2lab_u8``, ``cv_canny_u8``, the reflect-101 Laplacian) with every mean, variance and histogram
statistic in float64, which is what ``csrc/k_quality.hip`` says it computes.  It does not import the package under test.

How a byte enters a float statistic (the same rule as the kernel's, stated once):
  * contrast, saturation, the three naturalness thresholds: byte ``k`` stands for the float32 value ``k / 255`` that NumPy
    holds for it, lifted to float64 exactly.
  * sharpness: the Laplacian of the integer gray plane, divided by 255 in float64 (the reference file's float64 Laplacian
    of the float32 plane differs from it by the float32 rounding of ``k / 255``: part of the distances in DISTANCE below).
  * brightness: the integer L plane.
  * colourfulness, ``img`` not given (the frame IS ``u8 / 255``): ``rg = (r - g) / 255`` and ``yb = (r + g - 2 b) / 510`` from
    the integers.  ``img`` given (float32 image, e.g. a strategy's output before quantisation): ``rg`` and ``yb`` in float64
    from the float32 values.  This is the one score that depends on float32 inputs; see ``bound``.

DISTANCE: max |quality_ref - oracle.quality_assessment| per score, measured on the CPU over the frames of
tests/test_gpu_quality.py up to 1080 x 1920 (``PYTHONPATH=. python tests/quality_ref.py`` prints the table).  It says how far the
reference file's own float32 arithmetic is from exact; nothing here comes from the device.
"""
import numpy as np

from oracle import uwie_oracle as orc

KEYS = orc.QUALITY_KEYS
DEFAULT_WEIGHTS = orc.QUALITY_WEIGHTS

# measured on the CPU (see the module docstring): max |quality_ref - oracle| on the 0..100 scale
DISTANCE = {
    "u8": {"contrast": 1.2e-5, "sharpness": 5.6e-6, "entropy": 0.0, "saturation": 1.5e-5, "brightness": 4.2e-5, "edge_density": 0.0,
           "colorfulness": 1.6e-5, "naturalness": 0.0, "total": 4.7e-6},
    "f32": {"contrast": 6e-6, "sharpness": 4.6e-7, "entropy": 0.0, "saturation": 3.7e-5, "brightness": 1.6e-5, "edge_density": 0.0,
            "colorfulness": 3.5e-6, "naturalness": 0.0, "total": 5.7e-6},
}
EXACT = 1e-9  # scores that are a function of integer sums and histograms only


def bound(key, kind="u8"):
    """The device's bound against this reference: 1e-9 for what is a function of integer sums and histograms; for
    colourfulness from a float32 image, twice the measured float64-vs-float32-oracle distance, at most 2e-3."""
    if key == "colorfulness" and kind == "f32":
        return min(2.0 * DISTANCE["f32"]["colorfulness"], 2e-3)
    return EXACT


def total_bound(weights=None, kind="u8"):
    w = DEFAULT_WEIGHTS if weights is None else weights
    return sum(abs(float(w.get(k, 0))) * bound(k, kind) for k in KEYS)


def laplacian_i64(gray_u8):
    """cv2.Laplacian, ksize 1, BORDER_REFLECT_101, of the integer plane (an axis of length 1 reflects onto itself)."""
    g = np.pad(gray_u8.astype(np.int64), 1, mode="reflect")
    return g[:-2, 1:-1] + g[2:, 1:-1] + g[1:-1, :-2] + g[1:-1, 2:] - 4 * g[1:-1, 1:-1]


def scores(u8, img=None, weights=None, gray_shift=orc.GRAY_SHIFT_DEFAULT, edge_count=None):
    """[9] float64: the eight scores in KEYS order and the weighted total.  ``u8``: the quantised frame; ``img``: the float32
    image it was quantised from (colourfulness reads it), or None when the frame is ``u8 / 255``.  ``edge_count``: the
    number of Canny edge pixels when the caller has it already (the oracle's Canny is slow on very large frames)."""
    u8 = np.ascontiguousarray(u8, dtype=np.uint8)
    n = float(u8.shape[0] * u8.shape[1])
    gray_u8 = orc.cv_rgb2gray_u8(u8, gray_shift)
    f32 = (np.arange(256, dtype=np.float32) / np.float32(255.0))  # the float32 value NumPy holds for a byte
    lift = f32.astype(np.float64)
    hg = np.bincount(gray_u8.ravel(), minlength=256).astype(np.float64)
    hs = np.bincount(orc.cv_rgb2hsv_u8(u8)[:, :, 1].ravel(), minlength=256).astype(np.float64)
    hl = np.bincount(orc.cv_rgb2lab_u8(u8)[:, :, 0].ravel(), minlength=256).astype(np.float64)
    sc = np.empty(9, np.float64)
    mg = np.sum(hg * lift) / n
    sc[0] = np.clip(np.sqrt(np.sum(hg * (lift - mg) ** 2) / n) / 0.5 * 100, 0, 100)
    sc[1] = np.clip(np.var(laplacian_i64(gray_u8).astype(np.float64)) / (255.0 * 255.0) / 0.5 * 100, 0, 100)
    pk = hg[hg > 0] / n
    sc[2] = np.clip((-np.sum(pk * np.log(pk)) / np.log(2.0) - 4) / 4 * 100, 0, 100)
    sc[3] = np.clip(np.sum(hs * lift) / n * 100, 0, 100)
    sc[4] = 100 - np.clip(abs(np.sum(hl * np.arange(256.0)) / n - 128) / 128 * 100, 0, 100)
    if edge_count is None:
        edge_count = int(np.count_nonzero(orc.cv_canny_u8(gray_u8, 50, 150)))
    sc[5] = np.clip(edge_count / n / 0.2 * 100, 0, 100)
    if img is None:
        c = u8.astype(np.int64)
        rg = (c[:, :, 0] - c[:, :, 1]) / 255.0
        yb = (c[:, :, 0] + c[:, :, 1] - 2 * c[:, :, 2]) / 510.0
    else:
        x = np.asarray(img, dtype=np.float32).astype(np.float64)
        rg, yb = x[:, :, 0] - x[:, :, 1], 0.5 * (x[:, :, 0] + x[:, :, 1]) - x[:, :, 2]
    sc[6] = np.clip((np.sqrt(np.var(rg) + np.var(yb)) + 0.3 * np.sqrt(np.mean(rg) ** 2 + np.mean(yb) ** 2)) / 0.5 * 100, 0, 100)
    unnatural = np.sum(hs[f32 > np.float32(0.9)]) / n + np.sum(hg[f32 < np.float32(0.1)]) / n + np.sum(hg[f32 > np.float32(0.9)]) / n
    sc[7] = 100 - np.clip(unnatural * 200, 0, 100)
    w = DEFAULT_WEIGHTS if weights is None else weights
    total = 0.0
    for i, k in enumerate(KEYS):
        total += sc[i] * float(w.get(k, 0))
    sc[8] = total
    return sc


def oracle_scores(u8, img=None, weights=None, gray_shift=orc.GRAY_SHIFT_DEFAULT):
    """The same [9] row from oracle.quality_assessment (float32 NumPy)."""
    x = orc.normalise_u8(np.asarray(u8)) if img is None else np.asarray(img, dtype=np.float32)
    total, sc = orc.quality_assessment(x, weights=weights, gray_shift=gray_shift)
    return np.array([float(sc[k]) for k in KEYS] + [float(total)], np.float64)


def _measure():
    """Print DISTANCE: max |scores - oracle_scores| per score over the frames of tests/test_gpu_quality.py up to 1080p."""
    import os
    import sys
    import time

    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import test_gpu_quality as t

    u8_frames = list(t.batch_1080p()) + list(t.content_edges().values()) + list(t.select_frames())
    for B in (1, 3, 17):
        u8_frames += list(t.mixed_batch(B, 72, 101, seed=100 + B))
    for shape in t.EDGE_SHAPES:
        rng = np.random.default_rng(shape[0] * 1000 + shape[1])
        u8_frames += [rng.integers(0, 256, shape + (3,), dtype=np.uint8), t.mixed_frame(rng, "smooth", *shape), t.binary_noise(rng, *shape)]
    d_u8 = np.zeros(9)
    for f in u8_frames:
        d_u8 = np.maximum(d_u8, np.abs(scores(f) - oracle_scores(f)))
    print("u8 ", {k: float(f"{v:.2g}") for k, v in zip(KEYS + ("total",), d_u8)})
    rng = np.random.default_rng(31)
    d_f = np.zeros(9)
    for H, W in ((96, 130), (480, 640), (1080, 1920)):
        for img in (rng.random((H, W, 3)), rng.random((H, W, 3)) * 0.3,
                    t.underwater(rng, H, W) / 255.0 * 0.999 + rng.random((H, W, 3)) * 1e-3):
            img = img.astype(np.float32)
            d_f = np.maximum(d_f, np.abs(scores((img * 255).astype(np.uint8), img=img) - oracle_scores(None, img=img)))
    print("f32", {k: float(f"{v:.2g}") for k, v in zip(KEYS + ("total",), d_f)})
    for name, f in (("1080p", t.binary_noise(np.random.default_rng(1), 1080, 1920)), ("4K", t.binary_noise(np.random.default_rng(1), 2160, 3840))):
        g = orc.cv_rgb2gray_u8(f)
        t0 = time.perf_counter()
        orc.cv_canny_u8(g, 50, 150)
        print(f"oracle Canny {name}: {time.perf_counter() - t0:.1f} s")


if __name__ == "__main__":
    _measure()
