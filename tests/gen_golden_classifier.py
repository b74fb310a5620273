"""Writes tests/golden/classifier.npz: strategy classifiers fitted by scikit-learn, exported, and scikit-learn's answers.

Run by hand where scikit-learn is installed (``python tests/gen_golden_classifier.py``); the GPU tests read only the file.

* Three label sets of seeded synthetic 79-value rows (``c5``: the five Config.STRATEGIES names, ``c3``, ``c2``), each fitted
  with config.py's CLASSIFIERS (RANDOM_SEED = 42) as main.py:262-275 does: StandardScaler, then RandomForestClassifier,
  GradientBoostingClassifier and SVC(probability=True).
* ``{set}_{rf,gb,svc}_{array}``: StrategyClassifier's exported arrays; ``{set}_X``: unscaled query rows (held-out rows,
  training rows -- each sits just below some split's threshold --, rows moved onto a root threshold, rows with NaN);
  ``{set}_{model}_sk_label`` / ``_sk_proba``: scikit-learn's predict (index into classes) and predict_proba, ``{set}_svc_sk_dec``
  the one-vs-one decision values in libsvm's sign; rows scikit-learn refuses (GB / SVC with NaN) hold -1 and NaN.
* ``stump_*``: a hand-built forest of one tree that splits on ``gray_mean`` at 0.27, 0.51 and 0.75 (identity scaler): frames
  of different brightness get known, mixed labels.
"""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NAMES5 = ["StrongDehazing", "MediumDehazing", "LightEnhancement", "CLAHEEnhancement", "HistogramEqualization"]
SETS = {"c5": (NAMES5, 120), "c3": (["MediumDehazing", "CLAHEEnhancement", "HistogramEqualization"], 90),
        "c2": (["LightEnhancement", "StrongDehazing"], 70)}
RANDOM_SEED = 42
CLASSIFIERS = {  # config.py:100-119
    "random_forest": {"n_estimators": 200, "max_depth": 20, "min_samples_split": 5, "random_state": RANDOM_SEED},
    "gradient_boosting": {"n_estimators": 100, "learning_rate": 0.1, "max_depth": 5, "random_state": RANDOM_SEED},
    "svm": {"kernel": "rbf", "C": 1.0, "gamma": "scale", "random_state": RANDOM_SEED},
}
N_HELD_OUT = 100
STUMP_FEATURE = "gray_mean"
STUMP_THRESHOLDS = (0.27, 0.51, 0.75)  # gray_mean is on the [0, 1] scale
STUMP_CLASSES = ["HistogramEqualization", "CLAHEEnhancement", "LightEnhancement", "MediumDehazing"]


def synthetic_rows(seed: int, n: int, n_classes: int):
    """Rows on feature-like scales (offsets and spreads from 1e-3 to 1e2) with labels from a noisy rule on a few features."""
    rng = np.random.default_rng(seed)
    spread = 10.0 ** rng.uniform(-3, 2, 79)
    offset = rng.normal(0, 1, 79) * spread * 3
    z = rng.normal(size=(n, 79))
    w = np.zeros((79, n_classes))
    informative = rng.choice(79, 8, replace=False)
    w[informative] = rng.normal(size=(8, n_classes)) * 2
    y = np.argmax(z @ w + rng.normal(0, 0.7, (n, n_classes)), axis=1)
    return z * spread + offset, y


def fit_set(tag: str):
    """(scaler, {rf, gb, svc}: fitted model, query rows, class names) of one label set."""
    from sklearn.ensemble import GradientBoostingClassifier, RandomForestClassifier
    from sklearn.preprocessing import StandardScaler
    from sklearn.svm import SVC

    names, n_train = SETS[tag]
    X, y = synthetic_rows({"c5": 5, "c3": 3, "c2": 2}[tag], n_train + N_HELD_OUT, len(names))
    labels = np.asarray(names)[y]
    Xtr, ytr, Xte = X[:n_train], labels[:n_train], X[n_train:]
    scaler = StandardScaler().fit(Xtr)
    Xs = scaler.transform(Xtr)
    models = {"rf": RandomForestClassifier(**CLASSIFIERS["random_forest"]).fit(Xs, ytr),
              "gb": GradientBoostingClassifier(**CLASSIFIERS["gradient_boosting"]).fit(Xs, ytr),
              "svc": SVC(**CLASSIFIERS["svm"], probability=True).fit(Xs, ytr)}
    # queries: held-out rows, training rows, rows moved onto the first trees' root thresholds, NaN rows
    rf = models["rf"]
    on_thr = []
    for t in range(8):
        tree = rf.estimators_[t].tree_
        f, thr = int(tree.feature[0]), float(tree.threshold[0])
        row = Xte[t].copy()
        row[f] = thr * scaler.scale_[f] + scaler.mean_[f]
        on_thr.append(row)
        row = Xte[t].copy()  # exactly a float32 just at or below the threshold, in scaled units
        row[f] = float(np.float32(thr)) * scaler.scale_[f] + scaler.mean_[f]
        on_thr.append(row)
    nan_rows = Xte[:6].copy()
    gb_root = models["gb"].estimators_[0, 0].tree_
    nan_rows[0, int(gb_root.feature[0])] = np.nan
    nan_rows[1, int(rf.estimators_[0].tree_.feature[0])] = np.nan
    nan_rows[2, :] = np.nan
    nan_rows[3, 10:40] = np.nan
    nan_rows[4, int(rf.estimators_[1].tree_.feature[0])] = np.nan
    nan_rows[5, 78] = np.nan
    Q = np.concatenate([Xte, Xtr[:40], np.asarray(on_thr), nan_rows])
    return scaler, models, Q, names


def answers(scaler, model, Q, kind: str):
    """scikit-learn's (label index, proba[, ovo decision in libsvm's sign]) per row; -1 / NaN where it raises."""
    C = len(model.classes_)
    Qs = scaler.transform(Q)
    ok = np.ones(len(Q), bool) if kind == "rf" else ~np.isnan(Qs).any(axis=1)
    label = np.full(len(Q), -1, np.int32)
    proba = np.full((len(Q), C), np.nan)
    label[ok] = np.searchsorted(model.classes_, model.predict(Qs[ok]))
    proba[ok] = model.predict_proba(Qs[ok])
    out = {"label": label, "proba": proba}
    if kind == "svc":
        dec = np.full((len(Q), C * (C - 1) // 2), np.nan)
        d = model._decision_function(Qs[ok])  # one-vs-one; scikit-learn flips the sign for two classes
        dec[ok] = -d.reshape(-1, 1) if C == 2 else d
        out["dec"] = dec
    return out


def stump_arrays():
    """The hand-built forest: one tree splitting on gray_mean at STUMP_THRESHOLDS, identity scaler."""
    from underwater_image_enhancement_amd.api import FEATURE_EXTRACTOR_KEYS

    f = FEATURE_EXTRACTOR_KEYS.index(STUMP_FEATURE)
    C = len(STUMP_CLASSES)
    # node 0: <= t0 -> leaf 1 (class 0), else node 2: <= t1 -> leaf 3 (class 1), else node 4: <= t2 -> leaf 5 / leaf 6
    left = np.array([1, -1, 3, -1, 5, -1, -1], np.int32)
    right = np.array([2, -1, 4, -1, 6, -1, -1], np.int32)
    feature = np.array([f, -2, f, -2, f, -2, -2], np.int32)
    t0, t1, t2 = STUMP_THRESHOLDS
    threshold = np.array([t0, -2, t1, -2, t2, -2, -2], np.float64)
    value = np.zeros((7, C))
    value[1, 0] = value[3, 1] = value[5, 2] = value[6, 3] = 1.0
    value[[0, 2, 4]] = 1.0 / C
    return {"kind": np.int64(0), "classes": np.asarray(STUMP_CLASSES), "mean": np.zeros(79), "scale": np.ones(79),
            "tree_offset": np.array([0, 7], np.int32), "left": left, "right": right, "feature": feature,
            "threshold": threshold, "missing_left": np.array([1, 0, 1, 0, 1, 0, 0], np.uint8), "value": value}


def build() -> dict:
    from underwater_image_enhancement_amd.classifier import export_sklearn

    out = {}
    for tag in SETS:
        scaler, models, Q, names = fit_set(tag)
        out[f"{tag}_X"] = Q
        for kind, model in models.items():
            for k, v in export_sklearn(model, scaler).items():
                out[f"{tag}_{kind}_{k}"] = np.asarray(v)
            for k, v in answers(scaler, model, Q, kind).items():
                out[f"{tag}_{kind}_sk_{k}"] = v
    for k, v in stump_arrays().items():
        out[f"stump_{k}"] = np.asarray(v)
    return out


def arrays_of(golden: dict, prefix: str) -> dict:
    """The export dict stored under ``prefix`` (e.g. ``c5_rf``), as StrategyClassifier takes it."""
    n = len(prefix) + 1
    return {k[n:]: v for k, v in golden.items() if k.startswith(prefix + "_") and not k[n:].startswith("sk_")}


if __name__ == "__main__":
    path = os.path.join(ROOT, "tests", "golden", "classifier.npz")
    data = build()
    np.savez_compressed(path, **data)
    print(f"wrote {path}: {len(data)} arrays, {os.path.getsize(path)} bytes")
