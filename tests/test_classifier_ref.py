"""CPU checks of the strategy classifier's export and its NumPy restatement (tests/classifier_ref.py), against live
scikit-learn where it is installed, and of uwie_model_check, which needs no GPU."""
import os

import numpy as np
import pytest

import classifier_ref as ref
import gen_golden_classifier as gen
import underwater_image_enhancement_amd as uw
from underwater_image_enhancement_amd import _lib
from underwater_image_enhancement_amd.classifier import model_check

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "classifier.npz")
MODELS = [(tag, kind) for tag in gen.SETS for kind in ("rf", "gb", "svc")]


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def fresh():
    pytest.importorskip("sklearn")
    return gen.build()


@pytest.fixture(scope="module")
def fitted():
    pytest.importorskip("sklearn")
    return {tag: gen.fit_set(tag) for tag in gen.SETS}


@pytest.mark.parametrize("tag,kind", MODELS)
def test_restatement_matches_live_sklearn(fitted, tag, kind):
    from underwater_image_enhancement_amd.classifier import export_sklearn

    scaler, models, Q, _ = fitted[tag]
    model = models[kind]
    a = export_sklearn(model, scaler)
    want = gen.answers(scaler, model, Q, kind)
    labels, proba = ref.predict(a, Q)
    np.testing.assert_array_equal(labels, want["label"])
    ok = want["label"] >= 0
    if kind == "rf":
        assert ok.all()
        assert np.array_equal(proba, want["proba"])  # bit for bit
    elif kind == "gb":
        np.testing.assert_allclose(proba[ok], want["proba"][ok], rtol=0, atol=1e-15)
        Qs = scaler.transform(Q[ok])
        assert np.array_equal(ref.gb_raw(a, Qs).reshape(ok.sum(), -1), model.decision_function(Qs).reshape(ok.sum(), -1))
    else:
        np.testing.assert_allclose(proba[ok], want["proba"][ok], rtol=0, atol=1e-9)
        np.testing.assert_allclose(ref.svc_decision(a, ref.scale(a, Q[ok])), want["dec"][ok], rtol=0, atol=1e-12)
    assert np.isnan(proba[~ok]).all()


@pytest.mark.parametrize("kind", ["rf", "gb", "svc"])
def test_nan_rows_per_model_kind(fitted, kind):
    from underwater_image_enhancement_amd.classifier import export_sklearn

    scaler, models, Q, _ = fitted["c5"]
    nan_rows = Q[np.isnan(Q).any(axis=1)]
    assert len(nan_rows) == 6
    Qs = scaler.transform(nan_rows)
    labels, proba = ref.predict(export_sklearn(models[kind], scaler), nan_rows)
    if kind == "rf":  # the forest routes NaN through missing_go_to_left
        assert np.array_equal(proba, models[kind].predict_proba(Qs))
        np.testing.assert_array_equal(np.asarray(models[kind].classes_)[labels], models[kind].predict(Qs))
    else:
        with pytest.raises(ValueError, match="NaN"):
            models[kind].predict(Qs)
        assert (labels == -1).all() and np.isnan(proba).all()


def test_unsupported_estimators_raise_type_error(fitted):
    from sklearn.ensemble import GradientBoostingClassifier, HistGradientBoostingClassifier, RandomForestClassifier
    from sklearn.linear_model import LogisticRegression
    from sklearn.svm import SVC

    rng = np.random.default_rng(0)
    X, y = rng.normal(size=(40, 5)), np.array(["StrongDehazing", "CLAHEEnhancement"] * 20)
    bad = [LogisticRegression().fit(X, y), HistGradientBoostingClassifier(max_iter=3).fit(X, y),
           SVC(kernel="linear", probability=True).fit(X, y), SVC().fit(X, y),
           GradientBoostingClassifier(loss="exponential", n_estimators=3).fit(X, y),
           RandomForestClassifier(n_estimators=3).fit(X, np.stack([y, y[::-1]], axis=1))]
    for est in bad:
        with pytest.raises(TypeError):
            uw.StrategyClassifier.from_sklearn(est)
    with pytest.raises(TypeError, match="LogisticRegression"):
        uw.StrategyClassifier.from_sklearn(bad[0])
    ok = GradientBoostingClassifier(n_estimators=3, init="zero").fit(X, y)
    clf = uw.StrategyClassifier.from_sklearn(ok)
    assert clf.classes == ["CLAHEEnhancement", "StrongDehazing"]
    assert np.array_equal(clf.arrays["init"], [0.0])


def test_save_load_round_trip_and_model_data(fitted, tmp_path):
    scaler, models, Q, names = fitted["c3"]
    for kind, model in models.items():
        clf = uw.StrategyClassifier.from_model_data({"classifier": model, "scaler": scaler, "classes": sorted(names)})
        assert clf.strategy_keys == ["clahe_enhancement", "histogram_equalization", "medium_dehazing"]
        path = tmp_path / f"{kind}.npz"
        clf.save(path)
        back = uw.StrategyClassifier.load(path)
        assert back.kind == clf.kind and back.classes == clf.classes and back.strategies == clf.strategies
        assert sorted(back.arrays) == sorted(clf.arrays)
        for k, v in clf.arrays.items():
            assert np.array_equal(np.asarray(back.arrays[k]), np.asarray(v)), k
        with np.load(path, allow_pickle=False) as z:
            assert int(z["format_version"]) == 1
    custom = {"light_enhancement": {"name": "MediumDehazing", "omega": 0.3},
              "clahe_enhancement": {"name": "CLAHEEnhancement", "clip_limit": 3.0, "tile_grid_size": (4, 4)},
              "histogram_equalization": {"name": "HistogramEqualization"}}
    clf = uw.StrategyClassifier.from_sklearn(models["rf"], scaler, strategies=custom)
    assert clf.strategy_keys == ["clahe_enhancement", "histogram_equalization", "light_enhancement"]
    clf.save(tmp_path / "custom.npz")
    assert uw.StrategyClassifier.load(tmp_path / "custom.npz").strategies["light_enhancement"]["omega"] == 0.3
    with pytest.raises(ValueError, match="names no strategy"):
        uw.StrategyClassifier.from_sklearn(models["rf"], scaler, strategies={"clahe_enhancement": {"name": "CLAHEEnhancement"}})


def test_fixture_regenerates_to_the_same_arrays(golden, fresh):
    assert sorted(golden) == sorted(fresh)
    for k in golden:
        assert golden[k].dtype == np.asarray(fresh[k]).dtype, k
        assert np.array_equal(golden[k], fresh[k], equal_nan=golden[k].dtype.kind == "f"), k


def test_stump_labels_are_the_thresholds():
    rows = np.zeros((5, 79))
    f = uw.FEATURE_EXTRACTOR_KEYS.index("gray_mean")
    rows[:, f] = [0.1, 0.27, 0.4, 0.75, 0.9]
    labels, proba = ref.predict(gen.stump_arrays(), rows)
    # the rows are compared as float32: float32(0.27) > 0.27 goes right, float32(0.75) == 0.75 goes left
    assert labels.tolist() == [0, 1, 1, 2, 3]
    assert (proba.max(axis=1) == 1.0).all()


# ------------------------------------------------------------------ uwie_model_check: host only, no context, no GPU
def _corrupt(golden, prefix, change=None):
    a = {k: np.array(v, copy=True) for k, v in gen.arrays_of(golden, prefix).items()}
    if change is not None:
        change(a)
    return a


def test_model_check_accepts_every_fixture_model(golden):
    uw.load()
    for tag, kind in MODELS:
        assert model_check(gen.arrays_of(golden, f"{tag}_{kind}")) == 0, (tag, kind, _lib.load().uwie_last_error())
    assert model_check(gen.stump_arrays()) == 0


def test_model_check_rejects_corrupt_descriptors(golden):
    lib = uw.load()

    def child_not_after_parent(a):
        i = int(np.flatnonzero(a["left"][: a["tree_offset"][1]] >= 0)[-1])  # last internal node of tree 0
        a["left"][i] = i

    def child_out_of_tree(a):
        a["right"][0] = int(a["tree_offset"][1])  # one past tree 0's last node

    def feature_out_of_range(a):
        a["feature"][0] = 79

    def sv_count(a):
        a["n_support"][0] += 1

    def bad_threshold(a):
        a["threshold"][0] = np.inf

    def bad_coef(a):
        a["dual_coef"][0, 0] = np.nan

    cases = [("c5_rf", child_not_after_parent, "children"), ("c5_gb", child_out_of_tree, "children"),
             ("c3_rf", feature_out_of_range, "feature"), ("c5_svc", sv_count, "n_support"),
             ("c2_gb", bad_threshold, "threshold"), ("c3_svc", bad_coef, "coefficient")]
    for prefix, fn, word in cases:
        assert model_check(_corrupt(golden, prefix, fn)) == -1, (prefix, word)
        assert word in lib.uwie_last_error().decode(), (prefix, lib.uwie_last_error())
    a = _corrupt(golden, "c2_rf")
    a["kind"] = np.int64(7)
    assert model_check(a) == -1
    assert lib.uwie_model_check(None) == -1
