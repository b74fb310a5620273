"""StrategyClassifier on the MI355X (csrc/k_classify.hip) against tests/golden/classifier.npz and tests/classifier_ref.py:
scikit-learn's answers without scikit-learn, main.py's predict for frame batches, and each frame through its strategy."""
import os
import time

import numpy as np
import pytest
import torch

import classifier_ref as ref
import gen_golden_classifier as gen
import underwater_image_enhancement_amd as uw

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "classifier.npz")
MODELS = [(tag, kind) for tag in gen.SETS for kind in ("rf", "gb", "svc")]
GRAY_MEAN = uw.FEATURE_EXTRACTOR_KEYS.index("gray_mean")


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def _clf(golden, prefix):
    return uw.StrategyClassifier(gen.arrays_of(golden, prefix))


def _frames(levels, H=48, W=64, seed=0):
    """Textured frames whose gray mean sits near each level (the stump forest's feature)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    out = []
    for i, lv in enumerate(levels):
        field = 25 * np.sin(xx / (5.0 + i)) * np.cos(yy / 7.0)
        tint = np.array([0.9, 1.05, 1.05])
        img = (lv + field)[:, :, None] * tint + rng.normal(0, 6, (H, W, 3))
        out.append(np.clip(img, 0, 255).astype(np.uint8))
    return np.stack(out)


@pytest.mark.parametrize("tag,kind", MODELS)
def test_predict_rows_matches_sklearn(golden, tag, kind):
    clf = _clf(golden, f"{tag}_{kind}")
    X = golden[f"{tag}_X"]
    want_l, want_p = golden[f"{tag}_{kind}_sk_label"], golden[f"{tag}_{kind}_sk_proba"]
    ok = want_l >= 0
    labels, proba = clf.predict_rows(X[ok])
    np.testing.assert_array_equal(labels, want_l[ok])
    if kind == "rf":
        assert ok.all()
        assert np.array_equal(proba, want_p)  # bit for bit, NaN rows routed like the forest
    elif kind == "gb":
        np.testing.assert_allclose(proba, want_p[ok], rtol=0, atol=1e-15)
    else:
        np.testing.assert_allclose(proba, want_p[ok], rtol=0, atol=1e-9)
    # and the restatement the frame tests use agrees with the device on every row
    rl, rp = ref.predict(gen.arrays_of(golden, f"{tag}_{kind}"), X[ok])
    np.testing.assert_array_equal(labels, rl)
    if kind == "rf":
        assert np.array_equal(proba, rp)


@pytest.mark.parametrize("kind", ["rf", "gb", "svc"])
def test_same_bits_at_every_batch_size_and_run(golden, kind):
    clf = _clf(golden, f"c5_{kind}")
    X = golden["c5_X"]
    X = X[~np.isnan(X).any(axis=1)]
    big = np.resize(X, (4096, X.shape[1]))
    l_big, p_big = clf.predict_rows(big)
    l_again, p_again = clf.predict_rows(torch.from_numpy(big).cuda())  # a device tensor, a second run
    assert np.array_equal(l_big, l_again) and np.array_equal(p_big, p_again)
    l37, p37 = clf.predict_rows(big[100:137])
    assert np.array_equal(l37, l_big[100:137]) and np.array_equal(p37, p_big[100:137])
    for i in (0, 5, 4095):
        l1, p1 = clf.predict_rows(big[i])
        assert l1 == l_big[i] and np.array_equal(p1, p_big[i])


@pytest.mark.parametrize("kind", ["rf", "gb", "svc"])
def test_nan_rows(golden, kind):
    clf = _clf(golden, f"c5_{kind}")
    X = golden["c5_X"]
    nan = np.isnan(X).any(axis=1)
    if kind == "rf":
        labels, proba = clf.predict_rows(X[nan])
        np.testing.assert_array_equal(labels, golden["c5_rf_sk_label"][nan])
        assert np.array_equal(proba, golden["c5_rf_sk_proba"][nan])
        return
    with pytest.raises(ValueError, match="NaN"):
        clf.predict_rows(X)
    dev = uw.get_device()
    assert dev.check_status() == 0  # the bit was consumed by the call that raised
    # the device's own answer for the batch: -1 and NaN on exactly the NaN rows, the others untouched
    t = torch.from_numpy(np.ascontiguousarray(X)).cuda()
    label = torch.empty(len(X), dtype=torch.int32, device="cuda")
    proba = torch.empty((len(X), 5), dtype=torch.float64, device="cuda")
    import ctypes

    uw._lib.check(dev.lib.uwie_classify_f64(dev._ctx, clf._model(dev), ctypes.c_void_p(t.data_ptr()), len(X), 79,
                                            ctypes.c_void_p(label.data_ptr()), ctypes.c_void_p(proba.data_ptr()), dev.stream()))
    lh, ph = label.cpu().numpy(), proba.cpu().numpy()
    assert dev.check_status(allow=uw._lib.STATUS_CLASSIFY_NAN) == uw._lib.STATUS_CLASSIFY_NAN
    np.testing.assert_array_equal(lh == -1, nan)
    assert np.isnan(ph[nan]).all() and not np.isnan(ph[~nan]).any()
    np.testing.assert_array_equal(lh[~nan], golden[f"c5_{kind}_sk_label"][~nan])


@pytest.mark.parametrize("kind", ["rf", "gb", "svc"])
def test_predict_frames_is_main_py_predict(golden, kind):
    frames = _frames([30, 90, 140, 200, 240, 60], seed=3)
    clf = _clf(golden, f"c5_{kind}")
    rows = uw.feature_extractor_rows(frames)
    want_l, want_p = ref.predict(clf.arrays, rows)
    names, probs = clf.predict(frames)
    assert names == [clf.classes[i] for i in want_l]
    got_p = np.array([[p[c] for c in clf.classes] for p in probs])
    if kind == "rf":
        assert np.array_equal(got_p, want_p)
    else:
        np.testing.assert_allclose(got_p, want_p, rtol=0, atol=1e-9)
    name, prob = clf.predict(frames[2])  # one frame: single values, as main.py returns
    assert name == names[2] and list(prob) == clf.classes
    # a float RGB image in [0, 1] that is u8-derived takes the same path (main.py:415)
    name_f, _ = clf.predict(frames[2].astype(np.float32) / np.float32(255))
    assert name_f == names[2]


def test_odd_frame_size_against_a_79_feature_model(golden):
    clf = _clf(golden, "c5_rf")
    with pytest.raises(ValueError, match="74.*79"):
        clf.predict(_frames([100], H=47, W=64))
    with pytest.raises(ValueError, match="74.*79"):
        clf.predict_rows(np.zeros((2, 74)))


def test_enhance_runs_each_frame_through_its_strategy(golden):
    clf = _clf(golden, "stump")
    frames = _frames([40, 100, 160, 220, 35, 170], seed=5)
    rows = uw.feature_extractor_rows(frames)
    want_l, _ = ref.predict(clf.arrays, rows)
    assert len(set(want_l.tolist())) >= 3, rows[:, GRAY_MEAN]
    out, names = clf.enhance(frames)
    assert names == [clf.classes[i] for i in want_l]
    assert out.shape == frames.shape and out.dtype == np.uint8
    for i, frame in enumerate(frames):
        key = clf.strategy_keys[want_l[i]]
        y = uw.EnhancementStrategies.apply_strategy(frame.astype(np.float32) / np.float32(255), key, uw.CONFIG_STRATEGIES[key])
        assert np.array_equal(out[i], (y * 255).astype(np.uint8)), (i, key)
    one, name = clf.enhance(frames[1])
    assert name == names[1] and np.array_equal(one, out[1])


def test_predict_4k_batch_completes_in_time(golden):
    clf = _clf(golden, "c5_rf")
    g = torch.Generator(device="cuda").manual_seed(0)
    frames = torch.randint(0, 256, (16, 2160, 3840, 3), dtype=torch.uint8, device="cuda", generator=g)
    clf.predict(frames[:1])  # model upload, first launches
    t0 = time.perf_counter()
    names, probs = clf.predict(frames)
    elapsed = time.perf_counter() - t0
    assert len(names) == 16 and all(abs(sum(p.values()) - 1) < 1e-12 for p in probs)
    assert elapsed < 5.0, f"4K x 16 predict took {elapsed:.2f} s"
