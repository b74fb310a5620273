"""The predict phase of ``SelfSupervisedSystem`` (main.py:398-433) on the device: a fitted scikit-learn model, exported to
flat arrays, classifies ``FeatureExtractor`` rows and picks each frame's enhancement strategy.

* ``StrategyClassifier.from_sklearn`` / ``from_model_data`` read the three estimators ``train_classifier`` fits
  (main.py:271-275) and the ``StandardScaler`` in front of them; they are the only places that import scikit-learn.
* ``save`` / ``load`` keep the arrays in an ``.npz`` (no pickle), so a deployed box needs no scikit-learn.
* ``predict_rows`` / ``predict`` / ``enhance`` run ``uwie_classify_f64`` / ``uwie_predict_strategy_u8`` (csrc/k_classify.hip)
  and, for ``enhance``, the dict-surface strategy of each frame's label (``EnhancementStrategies.apply_strategy``).

The arithmetic each model follows is stated in include/uwie.h and DESIGN.md section 12.
"""
from __future__ import annotations

import ctypes
import json

import numpy as np
import torch

from . import _lib
from ._lib import check
from .runtime import HandleOwner

KIND_RF, KIND_GB, KIND_SVC = 0, 1, 2  # include/uwie.h UWIE_MODEL_*
KIND_NAMES = {KIND_RF: "RandomForestClassifier", KIND_GB: "GradientBoostingClassifier", KIND_SVC: "SVC"}
FORMAT_VERSION = 1
STATUS_CLASSIFY_NAN = _lib.STATUS_CLASSIFY_NAN

# arrays of each kind, in the .npz and in the export dict (besides kind / classes / mean / scale)
_TREE_KEYS = ("tree_offset", "left", "right", "feature", "threshold", "missing_left", "value")
_KIND_KEYS = {KIND_RF: _TREE_KEYS, KIND_GB: _TREE_KEYS + ("learning_rate", "init"),
              KIND_SVC: ("sv", "dual_coef", "intercept", "n_support", "prob_a", "prob_b", "gamma")}


def _export_trees(trees, value_of):
    """Concatenate sklearn ``Tree`` objects: tree-local child indices, a root offset per tree (plus the total at the end)."""
    offs, parts = [0], {k: [] for k in ("left", "right", "feature", "threshold", "missing_left", "value")}
    for t in trees:
        parts["left"].append(np.asarray(t.children_left, np.int32))
        parts["right"].append(np.asarray(t.children_right, np.int32))
        parts["feature"].append(np.asarray(t.feature, np.int32))
        parts["threshold"].append(np.asarray(t.threshold, np.float64))
        parts["missing_left"].append(np.asarray(t.missing_go_to_left, np.uint8))
        parts["value"].append(value_of(t))
        offs.append(offs[-1] + int(t.node_count))
    out = {k: np.ascontiguousarray(np.concatenate(v)) for k, v in parts.items()}
    out["tree_offset"] = np.asarray(offs, np.int32)
    return out


def export_sklearn(classifier, scaler=None) -> dict:
    """Flat arrays of a fitted RandomForestClassifier / GradientBoostingClassifier (log_loss) / SVC(kernel='rbf',
    probability=True) and its StandardScaler.  Raises ``TypeError`` for anything else."""
    from sklearn.ensemble import GradientBoostingClassifier, RandomForestClassifier
    from sklearn.preprocessing import StandardScaler
    from sklearn.svm import SVC

    name = type(classifier).__name__
    if type(classifier) not in (RandomForestClassifier, GradientBoostingClassifier, SVC):
        raise TypeError(f"StrategyClassifier takes RandomForestClassifier, GradientBoostingClassifier or SVC, not {name}")
    if not hasattr(classifier, "classes_"):
        raise TypeError(f"{name} is not fitted")
    if getattr(classifier, "n_outputs_", 1) != 1 or np.ndim(classifier.classes_) != 1:
        raise TypeError(f"multi-output {name} is not supported")
    classes = np.asarray(classifier.classes_)
    C = len(classes)
    F = int(classifier.n_features_in_)
    d = {"classes": classes.astype(str)}
    if isinstance(classifier, RandomForestClassifier):
        d["kind"] = KIND_RF
        d.update(_export_trees([e.tree_ for e in classifier.estimators_],
                               lambda t: np.asarray(t.value, np.float64).reshape(t.node_count, C)))
    elif isinstance(classifier, GradientBoostingClassifier):
        if classifier.loss != "log_loss":
            raise TypeError(f"GradientBoostingClassifier(loss={classifier.loss!r}) is not supported (log_loss only)")
        if classifier.init not in (None, "zero"):
            raise TypeError("GradientBoostingClassifier with a custom init estimator is not supported (default or 'zero')")
        est = classifier.estimators_  # [n_stages, K] of DecisionTreeRegressor, stage-major
        d["kind"] = KIND_GB
        d.update(_export_trees([e.tree_ for e in est.ravel()],
                               lambda t: np.asarray(t.value, np.float64).reshape(t.node_count)))
        d["learning_rate"] = np.float64(classifier.learning_rate)
        d["init"] = np.asarray(classifier._raw_predict_init(np.zeros((1, F), np.float32)), np.float64).reshape(-1)
        if d["init"].size != est.shape[1]:
            raise TypeError("GradientBoostingClassifier: unexpected init shape")
    else:
        if classifier.kernel != "rbf":
            raise TypeError(f"SVC(kernel={classifier.kernel!r}) is not supported (rbf only)")
        if not classifier.probability or classifier._probA.size == 0:
            raise TypeError("SVC without probability=True has no predict_proba (main.py fits probability=True)")
        d["kind"] = KIND_SVC
        d["sv"] = np.ascontiguousarray(classifier.support_vectors_, np.float64)
        d["dual_coef"] = np.ascontiguousarray(classifier._dual_coef_, np.float64)
        d["intercept"] = np.ascontiguousarray(classifier._intercept_, np.float64)
        d["n_support"] = np.asarray(classifier._n_support, np.int32)
        d["prob_a"] = np.ascontiguousarray(classifier._probA, np.float64)
        d["prob_b"] = np.ascontiguousarray(classifier._probB, np.float64)
        d["gamma"] = np.float64(classifier._gamma)
    if scaler is None:
        d["mean"], d["scale"] = np.zeros(F), np.ones(F)
    else:
        if type(scaler) is not StandardScaler:
            raise TypeError(f"the scaler must be a StandardScaler, not {type(scaler).__name__}")
        d["mean"] = np.asarray(scaler.mean_, np.float64) if scaler.with_mean else np.zeros(F)
        d["scale"] = np.asarray(scaler.scale_, np.float64) if scaler.with_std else np.ones(F)
    if d["mean"].shape != (F,) or d["scale"].shape != (F,):
        raise TypeError(f"scaler has {d['mean'].size} features, the classifier {F}")
    return d


def model_desc(d: dict):
    """(UwieModelDesc, the arrays it points into) of an export dict: keep the second value alive while the first is used."""
    kind = int(d["kind"])
    keep = {}

    def ptr(key, dtype):
        a = np.ascontiguousarray(d[key], dtype)
        keep[key] = a
        return a.ctypes.data_as(ctypes.c_void_p)

    F, C = int(np.size(d["mean"])), int(np.size(d["classes"]))
    P = C * (C - 1) // 2
    # the C side reads every array at the sizes the counts give: hold the shapes to them here
    if kind in (KIND_RF, KIND_GB):
        T, N = int(np.size(d["tree_offset"])) - 1, int(np.size(d["left"]))
        K = 1 if C == 2 else C
        want = {"tree_offset": (T + 1,), "right": (N,), "feature": (N,), "threshold": (N,), "missing_left": (N,),
                "value": (N, C) if kind == KIND_RF else (N,)}
        if kind == KIND_GB:
            want["init"] = (K,)
    elif kind == KIND_SVC:
        S = int(np.shape(d["sv"])[0]) if np.ndim(d["sv"]) == 2 else -1
        want = {"sv": (S, F), "dual_coef": (C - 1, S), "intercept": (P,), "n_support": (C,), "prob_a": (P,), "prob_b": (P,)}
    else:
        want = {}
    want["scale"] = (F,)
    for key, shape in want.items():
        if np.shape(d[key]) != shape:
            raise ValueError(f"model array {key!r} has shape {np.shape(d[key])}, expected {shape}")
    m = _lib.UwieModelDesc()
    m.kind = kind
    m.n_features = F
    m.n_classes = C
    m.mean, m.scale = ptr("mean", np.float64), ptr("scale", np.float64)
    if kind in (KIND_RF, KIND_GB):
        m.n_trees = int(np.size(d["tree_offset"])) - 1
        m.n_nodes = int(np.size(d["left"]))
        m.tree_offset = ptr("tree_offset", np.int32)
        m.left, m.right, m.feature = ptr("left", np.int32), ptr("right", np.int32), ptr("feature", np.int32)
        m.threshold, m.missing_left = ptr("threshold", np.float64), ptr("missing_left", np.uint8)
        m.value = ptr("value", np.float64)
        if kind == KIND_GB:
            m.learning_rate = float(d["learning_rate"])
            m.init = ptr("init", np.float64)
    elif kind == KIND_SVC:
        m.n_sv = int(np.shape(d["sv"])[0])
        m.sv, m.dual_coef, m.intercept = ptr("sv", np.float64), ptr("dual_coef", np.float64), ptr("intercept", np.float64)
        m.n_support = ptr("n_support", np.int32)
        m.prob_a, m.prob_b = ptr("prob_a", np.float64), ptr("prob_b", np.float64)
        m.gamma = float(d["gamma"])
    return m, keep


def model_check(d: dict) -> int:
    """``uwie_model_check`` of an export dict (host only: no context, no GPU): 0 or ``UWIE_E_INVALID``."""
    m, _keep = model_desc(d)
    return _lib.load().uwie_model_check(ctypes.byref(m))


def _strategy_table(classes, strategies):
    """class name -> strategy key, through each strategy's ``'name'`` (main.py:135 labels with it) or the key itself."""
    from .api import CONFIG_STRATEGIES

    strategies = CONFIG_STRATEGIES if strategies is None else strategies
    by_name = {}
    for key, params in strategies.items():
        if key not in _lib.DICT_STRATEGIES:
            raise ValueError(f"未知策略: {key}")
        by_name.setdefault(str(params.get("name", key)), key)
    keys = []
    for c in classes:
        c = str(c)
        key = by_name.get(c, c if c in strategies else None)
        if key is None:
            raise ValueError(f"class {c!r} names no strategy (known names: {sorted(by_name)})")
        keys.append(key)
    # the parameters as the saved file holds them (JSON: tuples become lists, NumPy scalars Python numbers)
    return keys, json.loads(json.dumps({k: dict(strategies[k]) for k in keys}, default=_json_value))


def _json_value(v):
    return v.tolist() if hasattr(v, "tolist") else list(v)


class StrategyClassifier(HandleOwner):
    """A fitted strategy classifier (main.py:225-335 trains it, :398-433 predicts with it) run on the device.

    ``clf.predict(frames)`` is main.py's ``predict`` for one frame or a batch; ``predict_rows`` classifies given feature
    rows; ``enhance`` runs each frame through its predicted strategy.  Construct with ``from_sklearn``,
    ``from_model_data`` (the dict main.py pickles) or ``load``."""

    def __init__(self, arrays: dict, strategies=None):
        kind = int(arrays["kind"])
        if kind not in _KIND_KEYS:
            raise ValueError(f"unknown model kind {kind}")
        self.arrays = {"kind": kind, "classes": np.asarray(arrays["classes"]).astype(str),
                       "mean": np.asarray(arrays["mean"], np.float64), "scale": np.asarray(arrays["scale"], np.float64)}
        for k in _KIND_KEYS[kind]:
            self.arrays[k] = np.asarray(arrays[k])
        self.kind = kind
        self.classes = [str(c) for c in self.arrays["classes"]]
        self.n_features = int(self.arrays["mean"].size)
        self.strategy_keys, self.strategies = _strategy_table(self.classes, strategies)
        rc = model_check(self.arrays)
        if rc != 0:
            raise ValueError(f"invalid model: {_lib.load().uwie_last_error().decode()}")

    # ------------------------------------------------------------------ construction
    @classmethod
    def from_sklearn(cls, classifier, scaler=None, strategies=None):
        return cls(export_sklearn(classifier, scaler), strategies)

    @classmethod
    def from_model_data(cls, d: dict, strategies=None):
        """The dict ``train_classifier`` pickles (main.py:318-329): ``classifier``, ``scaler`` and ``classes``."""
        clf = cls.from_sklearn(d["classifier"], d.get("scaler"), strategies)
        if "classes" in d and [str(c) for c in d["classes"]] != clf.classes:
            raise ValueError("model_data['classes'] differs from the classifier's classes_")
        return clf

    def save(self, path):
        """Write the model to an ``.npz`` (no pickle); ``load`` reads it without scikit-learn."""
        extra = {"format_version": np.int64(FORMAT_VERSION),
                 "strategies_json": np.asarray(json.dumps(self.strategies, sort_keys=True))}
        np.savez_compressed(path, **self.arrays, **extra)

    @classmethod
    def load(cls, path, strategies=None):
        with np.load(path, allow_pickle=False) as z:
            if "format_version" not in z.files or int(z["format_version"]) != FORMAT_VERSION:
                raise ValueError(f"{path}: not a StrategyClassifier file of format version {FORMAT_VERSION}")
            arrays = {k: z[k] for k in z.files if k not in ("format_version", "strategies_json")}
            if strategies is None and "strategies_json" in z.files:
                strategies = json.loads(str(z["strategies_json"]))
        return cls(arrays, strategies)

    # ------------------------------------------------------------------ device
    def _create_handle(self, dev):
        m, _keep = model_desc(self.arrays)
        h = ctypes.c_void_p()
        check(dev.lib.uwie_model_create(dev._ctx, ctypes.byref(m), ctypes.byref(h)))
        return h

    @staticmethod
    def _destroy_handle(dev, handle):
        dev._net_destroy(dev.lib.uwie_model_destroy, handle)

    _model = HandleOwner._handle  # the uwie_model of this classifier on ``dev``

    def _raise_nan(self, labels_h):
        bad = np.flatnonzero(labels_h < 0)
        raise ValueError(f"Input X contains NaN ({KIND_NAMES[self.kind]} does not accept missing values natively; "
                         f"rows {bad[:8].tolist()}{' ...' if bad.size > 8 else ''})")

    def _finish(self, dev, label, proba):
        """Read labels and proba back once, poll the device status word, raise on GB / SVC NaN rows."""
        label_h, proba_h = label.cpu().numpy(), proba.cpu().numpy()
        bits = dev.check_status(allow=STATUS_CLASSIFY_NAN)
        if bits & STATUS_CLASSIFY_NAN:
            self._raise_nan(label_h)
        return label_h, proba_h

    def predict_rows(self, rows, device: int | None = None):
        """Scaler + classifier on ``[B, F]`` (or ``[F]``) float64 rows, host NumPy or a device tensor.  Returns
        ``(labels, proba)``: int indices into ``classes`` ``[B]`` and ``predict_proba`` ``[B, n_classes]`` (NumPy)."""
        from .runtime import get_device

        dev = get_device(device)
        t = rows if isinstance(rows, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(rows, np.float64))
        single = t.dim() == 1
        t = t.reshape(1, -1) if single else t
        if t.dim() != 2 or t.shape[0] == 0:
            raise ValueError(f"expected [B, {self.n_features}] rows, got {tuple(rows.shape)}")
        if t.shape[1] != self.n_features:
            raise ValueError(f"X has {t.shape[1]} features, but the model expects {self.n_features} features as input")
        t = t.to(device=dev.torch_device, dtype=torch.float64).contiguous()
        B = int(t.shape[0])
        label = dev.empty((B,), torch.int32)
        proba = dev.empty((B, len(self.classes)), torch.float64)
        check(dev.lib.uwie_classify_f64(dev._ctx, self._model(dev), ctypes.c_void_p(t.data_ptr()), B, self.n_features,
                                        ctypes.c_void_p(label.data_ptr()), ctypes.c_void_p(proba.data_ptr()), dev.stream()))
        label_h, proba_h = self._finish(dev, label, proba)
        return (label_h[0], proba_h[0]) if single else (label_h, proba_h)

    def _frames(self, frames, dev):
        """u8 [H,W,3] / [B,H,W,3] frames, or float RGB in [0, 1] (``(x * 255).astype(uint8)`` plus the float image for the
        RGB block when it is not u8-derived, as FeatureExtractor) -> (u8 batch, f32 batch or None, single)."""
        from .api import _F255, _as_batch_u8

        if isinstance(frames, torch.Tensor) or np.asarray(frames).dtype == np.uint8:
            u8, _, single = _as_batch_u8(frames, dev)
            return u8, None, single
        x = np.asarray(frames)
        if x.dtype.kind != "f":
            raise TypeError(f"expected uint8 frames or float RGB in [0, 1], got {x.dtype}")
        if not (np.all(x >= 0) and np.all(x <= 1)):
            raise ValueError("float image values must lie in [0, 1]")
        u8_h = (x * 255).astype(np.uint8)  # feature_extraction.py:30,89,134,176,215
        u8, _, single = _as_batch_u8(u8_h, dev)
        f32 = None
        if not (x.dtype == np.float32 and np.array_equal(u8_h.astype(np.float32) / _F255, x)):
            f32 = dev.tensor(np.ascontiguousarray(x, np.float32)).reshape(u8.shape)
        return u8, f32, single

    def _predict_device(self, dev, u8, f32, want_rows: bool = False):
        B, H, W = dev._bhw(u8)
        n = dev.lib.uwie_feature_extractor_count(H, W)
        if n != self.n_features:
            raise ValueError(f"a {H}x{W} frame gives {n} feature values, but the model expects {self.n_features}"
                             + (" (the DCT block is absent when H or W is odd)" if n == 74 else ""))
        nbytes = dev.lib.uwie_workspace_bytes_predict(B, H, W)
        if nbytes == 0:
            raise _lib.UwieError("predict: batch/H/W out of range")
        ws = dev.workspace(nbytes)
        label = dev.empty((B,), torch.int32)
        proba = dev.empty((B, len(self.classes)), torch.float64)
        rows = dev.empty((B, n), torch.float64) if want_rows else None

        def p(t):
            return ctypes.c_void_p(t.data_ptr()) if t is not None else None

        check(dev.lib.uwie_predict_strategy_u8(dev._ctx, self._model(dev), p(u8), p(f32), B, H, W, 15, p(label), p(proba),
                                               p(rows), p(ws), ws.numel(), dev.stream()))
        return label, proba, rows

    def predict(self, frames, device: int | None = None):
        """main.py:398-433 for one frame (``(name, {class: p})``) or a batch (two lists): FeatureExtractor row, scaler,
        classifier, all on the device."""
        from .runtime import get_device

        dev = get_device(device)
        u8, f32, single = self._frames(frames, dev)
        label, proba, _ = self._predict_device(dev, u8, f32)
        label_h, proba_h = self._finish(dev, label, proba)
        names = [self.classes[i] for i in label_h]
        probs = [dict(zip(self.classes, (float(v) for v in row))) for row in proba_h]
        return (names[0], probs[0]) if single else (names, probs)

    def enhance(self, frames, device: int | None = None):
        """Each frame through ITS predicted strategy: ``(apply_strategy(x, key, params) * 255).astype(uint8)``
        (main.py:155's quantisation).  Returns ``(images, names)``: uint8 like the input batch (NumPy in, NumPy out), and
        the predicted class per frame."""
        from .api import _dict_params
        from .runtime import get_device

        dev = get_device(device)
        was_numpy = not isinstance(frames, torch.Tensor)
        u8, f32, single = self._frames(frames, dev)
        if f32 is not None:
            from .api import UnsupportedInputError

            raise UnsupportedInputError("enhance takes uint8 frames or their u8 / 255 float32 images (main.py:108)")
        label, proba, _ = self._predict_device(dev, u8, f32)
        label_h, _ = self._finish(dev, label, proba)
        out = torch.empty_like(u8)
        for c in np.unique(label_h):
            key = self.strategy_keys[int(c)]
            idx = torch.from_numpy(np.flatnonzero(label_h == c)).to(dev.torch_device)
            group = u8.index_select(0, idx).contiguous()
            img, _f64 = dev.enhance_u8_f64(group, _dict_params(dev, key, self.strategies[key]))
            out.index_copy_(0, idx, img)
            del _f64
        dev.check_status()
        names = [self.classes[i] for i in label_h]
        if single:
            out, names = out[0], names[0]
        if was_numpy:
            out = out.cpu().numpy()
            dev.check_status()
        return out, names
