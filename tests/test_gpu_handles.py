"""What the learned stack's shared host code must not change, in a few seconds: a handle owner that is closed frees its
network and packs it again at the next use, to the same bits; and the two byte-domain modules (csrc/k_diff_u8.hip) at the
smallest frames that reach every path of their kernels, against the CPU restatements as tests/test_gpu_diffenh_u8.py and
tests/test_gpu_gated_u8.py compare them.
  2 x 5 x 7: n = 35 = two whole 16-pixel groups and a 3-pixel tail; the second frame starts at byte 105 (unaligned)
  1 x 17 x 241: n = 16 * 256 + 1 = 256 groups, one for every thread of the one block, whose grid-stride loop takes it and ends,
                and a one-pixel tail"""
import os

import numpy as np
import pytest

import diffenh_u8_ref as RE
import gated_predictor_ref as GP
import gated_u8_ref as RG
import gen_golden_classifier as gen

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "classifier.npz")
SHAPES = [(2, 5, 7), (1, 17, 241)]


@pytest.fixture(scope="module")
def dev():
    import underwater_image_enhancement_amd as uw

    return uw.get_device(0)


def test_parameter_predictor_survives_close(dev):
    import underwater_image_enhancement_amd as uw

    net = uw.ParameterPredictor(GP.seeded_state(11, 79, 8, 1))
    rows = np.random.default_rng(3).standard_normal((2, 79))
    first = net.columns(rows, dev).cpu().numpy()
    assert first.shape == (2, 4) and np.isfinite(first).all() and len(net._handles) == 1
    net.close()
    assert len(net._handles) == 0
    net.close()
    again = net.columns(rows, dev).cpu().numpy()  # packed again
    assert np.array_equal(first.view(np.int32), again.view(np.int32)) and len(net._handles) == 1
    net.close()
    net.close()


def test_strategy_classifier_survives_close(dev):
    import underwater_image_enhancement_amd as uw

    with np.load(GOLDEN, allow_pickle=False) as z:
        golden = {k: z[k] for k in z.files}
    clf = uw.StrategyClassifier(gen.arrays_of(golden, "c5_rf"))
    X = golden["c5_X"]
    X = X[~np.isnan(X).any(axis=1)][:2]
    l0, p0 = clf.predict_rows(X)
    np.testing.assert_array_equal(l0, golden["c5_rf_sk_label"][~np.isnan(golden["c5_X"]).any(axis=1)][:2])
    clf.close()
    clf.close()
    l1, p1 = clf.predict_rows(X)
    assert np.array_equal(l0, l1) and np.array_equal(p0.view(np.int64), p1.view(np.int64))
    clf.close()
    clf.close()


def frames(shape):
    B, H, W = shape
    rng = np.random.default_rng(B * 1000003 + H * 1009 + W)
    u8 = np.empty((B, H, W, 3), np.uint8)
    for b in range(B):
        for c in range(3):  # each channel in its own sub-range of the bytes, so that the stretch has something to do
            lo = int(rng.integers(0, 100))
            u8[b, :, :, c] = rng.integers(lo, lo + int(rng.integers(40, 156)), (H, W))
    return u8


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_diff_enhance_u8_against_the_cpu_restatement(dev, shape):
    u8, B = frames(shape), shape[0]
    rng = np.random.default_rng(7)
    cols = np.stack([rng.uniform(2, 15, B), rng.uniform(60, 95, B), rng.uniform(0.3, 0.9, B), rng.uniform(1.0, 1.5, B)], 1).astype(np.float32)
    for flags in (0, 1, 2, 3):
        want = RE.float_image(u8, cols, flags)
        got_q, got_f = dev.diff_enhance_u8(dev.tensor(u8), dev.tensor(cols), flags, want_u8=True, want_f32=True)
        got = got_f.cpu().numpy()
        if not flags & 2:
            assert RE.same_bits(got, want), flags
            assert np.array_equal(got_q.cpu().numpy(), RE.quantise(want)), flags
        else:  # pow: <= 1 float32 ulp (values in [0, 1]: the int32 words are ordered as the values)
            assert np.all(got >= 0.0) and np.all(got <= 1.0)
            ulp = np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64)).max()
            print(f"{shape} flags {flags}: {ulp} ulp")
            assert ulp <= 1, flags
            assert np.array_equal(got_q.cpu().numpy(), RE.quantise(got)), flags  # the bytes are those of the floats beside them
    assert dev.check_status() == 0


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_diff_gated_u8_against_the_cpu_restatement(dev, shape):
    u8, B = frames(shape), shape[0]
    rng = np.random.default_rng(9)
    cols = np.stack([rng.uniform(1, 30, B), rng.uniform(65, 99, B), rng.uniform(0, 1, B), rng.uniform(0.5, 3, B)], 1).astype(np.float32)
    cols[0, 2] = 0.0  # use_gamma = 0: no pow, so this image is compared bit for bit
    want = RG.float_image(u8, cols)
    got_q, got_f = dev.diff_gated_u8(dev.tensor(u8), dev.tensor(cols), want_u8=True, want_f32=True)
    got, q = got_f.cpu().numpy(), got_q.cpu().numpy()
    assert np.all(got >= 0.0) and np.all(got <= 1.0)
    for b in range(B):
        if cols[b, 2] == 0:
            assert RG.same_bits(got[b], want[b]) and np.array_equal(q[b], RG.quantise(want[b])), b
        else:
            d = np.abs(got[b].astype(np.float64) - want[b].astype(np.float64)).max()
            print(f"{shape} image {b}: {d:.3g} from torch's CPU operations")
            assert d <= 2.0 ** -23, (b, d)
            assert np.array_equal(q[b], RG.quantise(got[b])), b  # the bytes are those of the floats beside them
    assert dev.check_status() == 0
