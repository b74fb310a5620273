"""quality_assessment.QualityAssessment on the device (csrc/k_quality.hip: uw.quality_scores, uw.QualityAssessment, uw.select_best)
at scale, at the edges and bit for bit.  The winner of select_best is the strategy classifier's training label
(main.py:118-146), so a wrong score shows nowhere else.

References and bounds (none of them comes from the device's output):
  * ``oracle.quality_assessment`` (float32 NumPy, the restatement of the reference file): ``edge_density`` and ``naturalness``
    to 1e-9, and the value class (NaN or number) of every score on degenerate input.
  * ``tests/quality_ref.py``: the same eight definitions in float64 from the oracle's integer planes.  Every score of a u8
    frame is a function of integer sums and histograms and is held to 1e-9 absolute on the 0..100 scale; the total to
    sum(|w|) * 1e-9.  Colourfulness of a FLOAT image (comprehensive_assessment, select_best) reads float32 values: its bound
    is twice the measured distance between quality_ref and the float32 oracle, ``quality_ref.bound('colorfulness', 'f32')``.
  * max |quality_ref - oracle| per score, measured on the CPU over the frames of this file up to 1080 x 1920 (how far the
    reference file's float32 arithmetic is from exact; ``python tests/quality_ref.py``): see quality_ref.DISTANCE.

    u8 frames:    contrast 1.2e-5, sharpness 5.6e-6, entropy 0, saturation 1.5e-5, brightness 4.2e-5, edge_density 0,
                  colorfulness 1.6e-5, naturalness 0, total (default weights) 4.7e-6
    float images: colorfulness 3.5e-6 (bound 7e-6), contrast 6e-6, sharpness 4.6e-7, saturation 3.7e-5, brightness 1.6e-5

CPU cost of the references, measured: the oracle's Canny (C) takes 0.1 s on a 1080 x 1920 frame of binary noise and 0.2 s at
2160 x 3840, so every frame of this file, the 4K ones included, is compared with the oracle's own Canny; the whole float64
reference of a 4K frame takes about a second.  The 1080p batch's edge counts are computed once per module.
"""
import warnings

import numpy as np
import pytest

import quality_ref as qr

pytestmark = pytest.mark.gpu

KEYS = qr.KEYS
ALL_DIFFERENT = {"contrast": 0.31, "sharpness": 0.07, "entropy": 0.13, "saturation": 0.11, "brightness": 0.05,
                 "edge_density": 0.17, "colorfulness": 0.09, "naturalness": 0.03}


@pytest.fixture(scope="module")
def uw():
    import underwater_image_enhancement_amd as uw

    return uw


@pytest.fixture(scope="module")
def dev(uw):
    return uw.get_device(0)


@pytest.fixture(scope="module")
def orc():
    from oracle import uwie_oracle

    return uwie_oracle


# ------------------------------------------------------------------ frames
def underwater(rng, H, W, gains=(0.45, 0.85, 0.80), noise=0.02):
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    ph = rng.random(3) * 6.283
    field = 0.55 + 0.25 * (np.sin(xx / (W / 9.0) + ph[0]) * np.cos(yy / (H / 7.0) + ph[1])
                           + 0.5 * np.sin((xx + 2 * yy) / (W / 5.0) + ph[2])) / 1.5
    f = field[:, :, None] * np.array(gains, np.float32)[None, None, :] + rng.normal(0, noise, (H, W, 3)).astype(np.float32)
    return np.clip(np.floor(255 * f), 0, 255).astype(np.uint8)


def binary_noise(rng, H, W):
    """0 / 255 per channel: the largest Laplacian and colourfulness sums a frame of this size can have."""
    return (rng.integers(0, 2, (H, W, 3), dtype=np.uint8) * 255).astype(np.uint8)


def checkerboard(H, W, period):
    yy, xx = np.mgrid[0:H, 0:W]
    return np.repeat((((yy // period + xx // period) & 1) * 255).astype(np.uint8)[:, :, None], 3, axis=2)


def mixed_frame(rng, kind, H, W):
    if kind == "noise":
        return rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    if kind == "smooth":
        return underwater(rng, H, W)
    if kind == "blue":
        return underwater(rng, H, W, (0.45, 0.75, 0.90))
    if kind == "dark":
        return rng.integers(0, 40, (H, W, 3), dtype=np.uint8)
    if kind == "bright":
        return rng.integers(215, 256, (H, W, 3), dtype=np.uint8)
    if kind == "binary":
        return binary_noise(rng, H, W)
    assert kind == "flat"
    return np.full((H, W, 3), 128, np.uint8)


MIXED_KINDS = ("noise", "smooth", "dark", "bright", "binary", "blue")


def mixed_batch(B, H, W, seed):
    """B frames of mixed content; from three frames on, the middle one is flat."""
    rng = np.random.default_rng(seed)
    frames = [mixed_frame(rng, MIXED_KINDS[b % len(MIXED_KINDS)], H, W) for b in range(B)]
    if B >= 3:
        frames[B // 2] = mixed_frame(rng, "flat", H, W)
    return np.stack(frames)


def content_edges(H=64, W=96):
    """name -> u8 frame: constants, the largest Laplacian sums, saturated channels, V = 0 with S undefined."""
    out = {"all_0": np.zeros((H, W, 3), np.uint8), "all_255": np.full((H, W, 3), 255, np.uint8),
           "checker_1": checkerboard(H, W, 1), "checker_2": checkerboard(H, W, 2)}
    for c, name in enumerate(("red", "green", "blue")):
        f = np.zeros((H, W, 3), np.uint8)
        f[:, :, c] = 255
        out["pure_" + name] = f
    half = np.zeros((H, W, 3), np.uint8)  # left: V = 0 (S undefined, sdiv_table[0]); right: S = 255 at every V
    half[:, W // 2:, 0] = np.arange(H, dtype=np.uint8)[:, None] * 3 + 1
    out["v0_and_s255"] = half
    return out


EDGE_SHAPES = ((1, 1), (1, 40), (40, 1), (2, 3), (3, 2), (5, 7), (17, 255), (16, 257), (64, 1023))


def large_frames():
    """name -> u8 frame at 1080p (the 4K ones are made in their test)."""
    rng = np.random.default_rng(1080)
    return {"binary_1080p": binary_noise(rng, 1080, 1920), "smooth_1080p": underwater(rng, 1080, 1920)}


def batch_1080p():
    """Eight 1080 x 1920 frames of mixed content, the two of large_frames() among them."""
    big = large_frames()
    rng = np.random.default_rng(8)
    rest = [mixed_frame(rng, k, 1080, 1920) for k in ("noise", "dark", "flat", "bright", "blue", "smooth")]
    return np.stack([big["binary_1080p"], rest[0], rest[1], big["smooth_1080p"], rest[2], rest[3], rest[4], rest[5]])


def select_frames():
    """Four 480 x 640 frames whose best two totals are far apart in the oracle (checked on the CPU, see the winner test)."""
    rng = np.random.default_rng(480)
    return np.stack([underwater(rng, 480, 640, (0.45, 0.85, 0.80)), underwater(rng, 480, 640, (0.45, 0.75, 0.90)),
                     rng.integers(0, 256, (480, 640, 3), dtype=np.uint8),
                     np.floor(255 * (rng.random((480, 640, 3)) * 0.7 + 0.15)).astype(np.uint8)])


# ------------------------------------------------------------------ comparison
def check_rows(got, frames, weights, what, orc_rows=None, edge_counts=None):
    """Every column of ``got`` [B, 9] against quality_ref on the u8 frames; edge_density and naturalness against the oracle
    too when its rows are given.  Prints each distance before it asserts."""
    got = np.asarray(got)
    assert got.shape == (len(frames), 9) and got.dtype == np.float64
    tb = qr.total_bound(weights)
    for b, u8 in enumerate(frames):
        want = qr.scores(u8, weights=weights, edge_count=None if edge_counts is None else edge_counts[b])
        d = np.abs(got[b] - want)
        print(f"{what}[{b}] |device - quality_ref| = " + " ".join(f"{k}={v:.3g}" for k, v in zip(KEYS + ("total",), d)))
        for i, k in enumerate(KEYS):
            assert d[i] <= qr.bound(k), (what, b, k, got[b, i], want[i])
        assert d[8] <= tb, (what, b, "total", got[b, 8], want[8])
        if orc_rows is not None:
            for i in (5, 7):
                assert abs(got[b, i] - orc_rows[b][i]) <= 1e-9, (what, b, KEYS[i], got[b, i], orc_rows[b][i])


def same_bits(a, b, what):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    if not np.array_equal(a.view(np.uint64), b.view(np.uint64)):
        bad = np.argwhere(a.view(np.uint64) != b.view(np.uint64))
        i = tuple(bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {a.size} values differ in their bits; first at {i}: {a[i]!r} vs {b[i]!r} "
                             f"(difference {a[i] - b[i]:.3g})")


@pytest.fixture(scope="module")
def big(orc):
    """The 1080p batch and the oracle's own Canny edge count of every frame, computed once."""
    frames = batch_1080p()
    edges = [int(np.count_nonzero(orc.cv_canny_u8(orc.cv_rgb2gray_u8(f), 50, 150))) for f in frames]
    return {"frames": frames, "edges": edges}


def select_sets(uw, dev):
    from underwater_image_enhancement_amd.api import _dict_params

    plist = [_dict_params(dev, k, v) for k, v in uw.CONFIG_STRATEGIES.items()]
    return plist, [uw.CONFIG_QUALITY_WEIGHTS.get(k, 0) for k in uw.QUALITY_KEYS]


# ------------------------------------------------------------------ 1. every score, u8 batch form
@pytest.mark.parametrize("B", [1, 3, 17])
def test_every_score_of_a_u8_batch(uw, B):
    """All nine columns of uw.quality_scores for batches of mixed content (one flat frame in the middle), with the default
    weights and with eight different weights; row b of the batch is the single-frame call bit for bit (an offset error of
    b * npx, b * 768, b * 4 or b * 2 in any score shows here, whatever its weight)."""
    assert len(set(ALL_DIFFERENT.values())) == 8
    frames = mixed_batch(B, 72, 101, seed=100 + B)
    orc_rows = [qr.oracle_scores(f) for f in frames]
    for weights in (None, ALL_DIFFERENT):
        got = uw.quality_scores(frames, weights=weights)
        check_rows(got, frames, weights, f"batch{B}", orc_rows)
        for b in range(B):
            same_bits(uw.quality_scores(frames[b], weights=weights), got[b], f"batch {B} row {b} against the single-frame call")


# ------------------------------------------------------------------ 2. edges
@pytest.mark.parametrize("shape", EDGE_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_tiny_and_ragged_shapes(uw, shape):
    """k_qa_lap's reflect-101 rules for H == 1 and W == 1, widths that are not multiples of 4 or 256.  The oracle on the CPU
    returns finite numbers for every one of these shapes, 1 x 1 included (no NaN, no warning: std and var of one value are 0,
    np.pad reflects an axis of length 1 onto itself, the entropy of one value is 0): the device must return those numbers."""
    rng = np.random.default_rng(shape[0] * 1000 + shape[1])
    frames = np.stack([rng.integers(0, 256, shape + (3,), dtype=np.uint8), mixed_frame(rng, "smooth", *shape),
                       binary_noise(rng, *shape)])
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # the oracle raises no warning on these shapes
        orc_rows = [qr.oracle_scores(f) for f in frames]
    assert np.isfinite(np.array(orc_rows)).all()
    got = uw.quality_scores(frames, weights=ALL_DIFFERENT)
    assert np.isfinite(got).all()
    check_rows(got, frames, ALL_DIFFERENT, f"{shape[0]}x{shape[1]}", orc_rows)


def test_content_edges(uw):
    """Constant frames at 0 and 255, 0 / 255 checkerboards of period 1 and 2 (|l| = 1020 at every pixel: the largest Laplacian
    sums), one saturated channel, and V = 0 next to S = 255 (RGB2HSV's sdiv_table at both ends)."""
    edges = content_edges()
    frames = np.stack(list(edges.values()))
    orc_rows = [qr.oracle_scores(f) for f in frames]
    got = uw.quality_scores(frames, weights=ALL_DIFFERENT)
    check_rows(got, frames, ALL_DIFFERENT, "content", orc_rows)
    names = list(edges)
    assert got[names.index("checker_1"), 1] == 100.0 and got[names.index("all_0"), 1] == 0.0  # sharpness really at both ends
    assert got[names.index("pure_red"), 3] == 100.0 and got[names.index("all_255"), 3] == 0.0  # saturation too


# ------------------------------------------------------------------ 3. size
def test_1080p_frames_and_batch(uw, big):
    """Two single 1080 x 1920 frames (binary noise, smooth underwater) and a batch of eight, edge_density against the oracle's
    own Canny."""
    frames, edges = big["frames"], big["edges"]
    for b in (0, 3):
        check_rows(uw.quality_scores(frames[b:b + 1]), frames[b:b + 1], None, f"1080p frame {b}", edge_counts=edges[b:b + 1])
    check_rows(uw.quality_scores(frames, weights=ALL_DIFFERENT), frames, ALL_DIFFERENT, "1080p batch", edge_counts=edges)


def test_4k_frames(uw):
    """2160 x 3840, binary noise (the largest sums) and smooth underwater, every score, the oracle's own Canny included."""
    rng = np.random.default_rng(2160)
    for name, u8 in (("binary_4k", binary_noise(rng, 2160, 3840)), ("smooth_4k", underwater(rng, 2160, 3840))):
        check_rows(uw.quality_scores(u8[None]), u8[None], None, name, [qr.oracle_scores(u8)])


# ------------------------------------------------------------------ 4. bits
def test_two_runs_and_two_batch_positions_give_the_same_bits(uw, dev, big):
    """Every score and total is the same float64 bits in two runs, and for the same frame at another position of another
    batch: for quality_scores on the 1080p batch (u8 frames, and with the float images given, which is the colourfulness
    path select_best takes), and for select_best on four 480 x 640 frames."""
    frames = big["frames"]
    first = uw.quality_scores(frames)
    same_bits(uw.quality_scores(frames), first, "quality_scores, second run")
    other = np.stack([frames[5], frames[3], frames[0]])
    same_bits(uw.quality_scores(other), first[[5, 3, 0]], "quality_scores, other batch")
    f32 = frames[:4].astype(np.float32) / np.float32(255.0)
    first_f = uw.quality_scores(frames[:4], frames_f32=f32)
    for run in range(3):
        same_bits(uw.quality_scores(frames[:4], frames_f32=f32), first_f, f"quality_scores with float images, run {run + 2}")
    same_bits(uw.quality_scores(frames[[3, 1]], frames_f32=f32[[3, 1]]), first_f[[3, 1]], "quality_scores with float images, other batch")

    sel = select_frames()
    plist, wts = select_sets(uw, dev)
    runs = [dev.select_best_u8(dev.tensor(sel), plist, wts, want_all=True) for _ in range(3)]
    for r in runs[1:]:
        same_bits(r[2].cpu().numpy(), runs[0][2].cpu().numpy(), "select_best scores, repeated run")
        assert np.array_equal(r[0].cpu().numpy(), runs[0][0].cpu().numpy()) and np.array_equal(r[3].cpu().numpy(), runs[0][3].cpu().numpy())
    extra = underwater(np.random.default_rng(5), 480, 640)
    other = np.stack([sel[2], extra, sel[0], sel[3], extra[::-1].copy(), sel[1]])
    got = dev.select_best_u8(dev.tensor(other), plist, wts, want_all=True)
    same_bits(got[2].cpu().numpy()[:, [2, 5, 0, 3]], runs[0][2].cpu().numpy(), "select_best scores, other batch")
    assert np.array_equal(got[0].cpu().numpy()[[2, 5, 0, 3]], runs[0][0].cpu().numpy())
    dev.check_status()


# ------------------------------------------------------------------ 5. the tie rule
def test_first_of_two_tied_strategies_wins(uw, dev):
    """strong_dehazing, medium_dehazing and light_enhancement are one function of (omega, guided_radius, L_low, L_high, gamma)
    (enhancement_strategies.py:350-474), so the same parameters under two keys are the same parameter set under two names.
    Their totals are bit-equal and, wherever a copy holds the maximum, the first one listed wins; in the other order the
    other name wins.  With naturalness as the only weight the copies hold the maximum on frames 0, 1 and 3 (float64 reference
    of the oracle's outputs on the CPU: 31.2, 30.8 and 15.5 against at most 21.1, 18.6 and 5.5 for the other sets), so the
    rule decides three of the four frames.  Then six sets through the C entry point with the copy also as the last one, under
    three weight vectors: the winner is np.argmax of the device's totals (the first maximum) and never a later copy."""
    from underwater_image_enhancement_amd.api import _dict_params

    same = {"omega": 0.5, "guided_radius": 15, "L_low": 10, "L_high": 95, "gamma": 1.2, "apply_gamma": True}
    frames = select_frames()

    def table(order):
        return {key: dict(uw.CONFIG_STRATEGIES[key], name=name) if name in ("C", "H") else dict(same, name=name) for key, name in order}

    copy_won = 0
    for order, first in (((("strong_dehazing", "A"), ("clahe_enhancement", "C"), ("medium_dehazing", "B"), ("histogram_equalization", "H"),
                           ("light_enhancement", "Z")), "A"),
                         ((("medium_dehazing", "B"), ("clahe_enhancement", "C"), ("light_enhancement", "Z"), ("histogram_equalization", "H"),
                           ("strong_dehazing", "A")), "B")):
        names, images, scores, every = uw.select_best(frames, strategies=table(order), weights={"naturalness": 1.0}, return_all=True)
        for b in range(len(frames)):
            same_bits([scores[b]["A"], scores[b]["A"]], [scores[b]["B"], scores[b]["Z"]], f"frame {b}: totals of the copies")
            assert np.array_equal(every["A"][b], every["B"][b]) and np.array_equal(every["A"][b], every["Z"][b])
            assert names[b] == max(scores[b], key=scores[b].get)  # dicts keep the order: the first maximum
            if scores[b]["A"] == max(scores[b].values()):
                copy_won += 1
                assert names[b] == first, (b, names[b], first, scores[b])
    assert copy_won >= 6, f"the tied copies hold the maximum on {copy_won} (frame, order) pairs, 6 expected: the rule was not exercised"
    p = _dict_params(dev, "strong_dehazing", same)
    others = [_dict_params(dev, k, uw.CONFIG_STRATEGIES[k]) for k in ("clahe_enhancement", "histogram_equalization", "light_enhancement")]
    for plist, copies in (([p, others[0], p, others[1], others[2], p], (0, 2, 5)), ([others[0], p, others[1], others[2], p, p], (1, 4, 5))):
        for wts in ([0.25, 0.20, 0.15, 0.15, 0.15, 0.10, 0, 0], [0, 0, 0, 0, 1.0, 0, 0, 0], [0, 0, 0, 0, 0, 0, 0, 1.0]):
            best, _, sc, _ = dev.select_best_u8(dev.tensor(frames), plist, wts)
            best, tot = best.cpu().numpy(), sc.cpu().numpy()[:, :, 8]
            for c in copies[1:]:
                same_bits(tot[c], tot[copies[0]], "six sets: totals of the copies")
            assert np.array_equal(best, np.argmax(tot, axis=0)), (best, tot)  # np.argmax: the first maximum
            assert all(k not in copies[1:] for k in best), (best, copies)
            if wts[7]:
                assert [int(best[b]) for b in (0, 1, 3)] == [copies[0]] * 3, (best, copies)
    dev.check_status()


# ------------------------------------------------------------------ 6. the winner, unconditionally
def test_winner_is_the_first_maximum_and_the_references(uw, orc):
    """select_best on the four 480 x 640 frames: the winner is the first maximum of the device's own totals, every set's total
    is within its bound of the float64 reference, and the winner is the reference's whenever the reference's two best totals
    differ by more than the two bounds together.  Where gamma's pow moves a byte by 1 LSB the DEVICE's bytes are scored with
    the reference (the bytes themselves are held to the oracle's: identical, or <= 1 LSB with gamma), so no slack is added.
    Checked with the oracle on the CPU: in all 4 of the 4 frames the two best totals are further apart than the bounds
    (the smallest gap is 2.63 on the 0..100 scale; the bounds together are 2e-9)."""
    frames = select_frames()
    keys = list(uw.CONFIG_STRATEGIES)
    weights = uw.CONFIG_QUALITY_WEIGHTS
    names, images, scores, every = uw.select_best(frames, return_all=True)
    tb = qr.total_bound(weights, "f32")  # colourfulness (the float image) has weight 0 in Config.QUALITY_WEIGHTS
    decided = 0
    for b, u8 in enumerate(frames):
        x = orc.normalise_u8(u8)  # main.py:108
        want = {}
        for k in keys:
            name = uw.CONFIG_STRATEGIES[k]["name"]
            params = {kk: v for kk, v in uw.CONFIG_STRATEGIES[k].items() if kk != "name"}
            enhanced = orc.DictStrategyOracle.run(x, k, params)
            d = np.abs(every[name][b].astype(int) - (enhanced * 255).astype(np.uint8).astype(int))
            assert d.max() <= (1 if params.get("apply_gamma") else 0), (b, name, int(d.max()))
            want[name] = float(qr.scores(every[name][b], img=enhanced.astype(np.float32), weights=weights)[8])
            print(f"frame {b} {name}: device {scores[b][name]!r} reference {want[name]!r} bytes differing {np.count_nonzero(d)}")
            assert abs(scores[b][name] - want[name]) <= tb, (b, name, scores[b][name], want[name])
        assert names[b] == max(scores[b], key=scores[b].get)  # first maximum of the device's own totals (dicts keep order)
        assert np.array_equal(images[b], every[names[b]][b])
        ranked = sorted(want.values(), reverse=True)
        if ranked[0] - ranked[1] > 2 * tb:
            decided += 1
            assert names[b] == max(want, key=want.get), (b, names[b], want)
    assert decided == 4, decided


# ------------------------------------------------------------------ 7. NaN and the status word
def test_nan_pixel_and_status(uw, dev, orc):
    """A float frame with one NaN pixel through comprehensive_assessment.  The oracle on the CPU: (x * 255).astype(uint8) turns
    the NaN into a byte (a RuntimeWarning, 'invalid value encountered in cast'), so the seven scores of the quantised frame
    are numbers; colourfulness reads the float image and is NaN (np.clip keeps a NaN), and the weighted total is NaN even
    where colourfulness has weight 0 (NaN * 0).  The device returns the same class per score, the numbers within their
    bounds, leaves the status word clean, and the next call is unaffected."""
    rng = np.random.default_rng(7)
    img = (underwater(rng, 60, 84).astype(np.float32) / np.float32(255.0))
    clean = uw.QualityAssessment.comprehensive_assessment(img)
    bad = img.copy()
    bad[31, 40, 1] = np.nan
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        wtotal, want = orc.quality_assessment(bad)
        u8 = (bad * 255).astype(np.uint8)
        for weights in (None, uw.CONFIG_QUALITY_WEIGHTS):
            total, got = uw.QualityAssessment.comprehensive_assessment(bad, weights=weights)
            assert dev.check_status() == 0
            assert np.isnan(orc.quality_assessment(bad, weights=weights)[0]) and np.isnan(total)
            ref = qr.scores(u8, img=bad, weights=weights)
            for i, k in enumerate(KEYS):
                assert np.isnan(got[k]) == bool(np.isnan(want[k])), (k, got[k], want[k])
                if not np.isnan(want[k]):
                    assert abs(got[k] - ref[i]) <= qr.bound(k), (k, got[k], ref[i])
    assert [k for k in KEYS if np.isnan(want[k])] == ["colorfulness"]
    again = uw.QualityAssessment.comprehensive_assessment(img)
    assert again == clean and np.isfinite(again[0]) and dev.check_status() == 0
    ref = qr.scores((img * 255).astype(np.uint8), img=img)
    for i, k in enumerate(KEYS):
        assert abs(again[1][k] - ref[i]) <= qr.bound(k, "f32"), (k, again[1][k], ref[i])
    assert abs(again[0] - ref[8]) <= qr.total_bound(None, "f32")


def test_float_images_through_comprehensive_assessment(uw):
    """The float-image path at its bound: colourfulness from float32 values that are not k / 255 (the other seven scores come
    from the quantised frame and stay at 1e-9), on frames up to 1080p."""
    rng = np.random.default_rng(31)
    for H, W in ((96, 130), (480, 640), (1080, 1920)):
        for name, img in (("random", rng.random((H, W, 3))), ("dark", rng.random((H, W, 3)) * 0.3),
                          ("smooth", underwater(rng, H, W) / 255.0 * 0.999 + rng.random((H, W, 3)) * 1e-3)):
            img = img.astype(np.float32)
            total, got = uw.QualityAssessment.comprehensive_assessment(img, weights=ALL_DIFFERENT)
            ref = qr.scores((img * 255).astype(np.uint8), img=img, weights=ALL_DIFFERENT)
            d = [abs(got[k] - ref[i]) for i, k in enumerate(KEYS)] + [abs(total - ref[8])]
            print(f"{name} {H}x{W} |device - quality_ref| = " + " ".join(f"{k}={v:.3g}" for k, v in zip(KEYS + ("total",), d)))
            for i, k in enumerate(KEYS):
                assert d[i] <= qr.bound(k, "f32"), (name, H, W, k, got[k], ref[i])
            assert d[8] <= qr.total_bound(ALL_DIFFERENT, "f32"), (name, H, W, total, ref[8])
