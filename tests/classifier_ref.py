"""NumPy restatement of the three strategy classifiers (csrc/k_classify.hip), run from StrategyClassifier's exported arrays.

* ``scale``: ``StandardScaler.transform``, ``(x - mean_) / scale_`` in float64.
* trees: the rows cast to float32 (scikit-learn's ``DTYPE``), ``x <= threshold`` per node, NaN goes left iff
  ``missing_go_to_left``.
* ``rf_proba``: ``RandomForestClassifier.predict_proba``: the leaves' class fractions summed in tree order from 0, then
  divided by the tree count; ``predict`` is the first maximum.
* ``gb_raw`` / ``gb_proba``: ``predict_stages``: ``raw = init``, then ``raw[k] += learning_rate * value[leaf]`` stage by
  stage; softmax (multinomial) or expit (binary, ``[1 - p, p]``).
* ``svc_decision`` / ``svc_predict`` / ``svc_proba``: libsvm's ``svm_predict_values`` (RBF kernel, one-vs-one decision
  values and votes) and ``svm_predict_probability`` (Platt sigmoid, ``multiclass_probability``).

``predict(arrays, X) -> (labels, proba)`` is what the device returns; GB / SVC rows holding NaN get label -1 and NaN.
"""
from __future__ import annotations

import numpy as np

KIND_RF, KIND_GB, KIND_SVC = 0, 1, 2


def scale(a, X):
    X = np.asarray(X, np.float64)
    return (X - a["mean"]) / a["scale"]


def leaves(a, X32, t):
    """Tree-local leaf index of every row of float32 ``X32`` in tree ``t``."""
    o0 = int(a["tree_offset"][t])
    left, right = a["left"][o0:], a["right"][o0:]
    feat, thr, miss = a["feature"][o0:], a["threshold"][o0:], a["missing_left"][o0:]
    node = np.zeros(len(X32), np.int64)
    live = left[node] >= 0
    while live.any():
        n = node[live]
        x = X32[np.flatnonzero(live), feat[n]].astype(np.float64)
        go_left = np.where(np.isnan(x), miss[n] != 0, x <= thr[n])
        node[live] = np.where(go_left, left[n], right[n])
        live = left[node] >= 0
    return node


def rf_proba(a, Xs):
    X32 = Xs.astype(np.float32)
    T = len(a["tree_offset"]) - 1
    C = a["value"].shape[1]
    acc = np.zeros((len(Xs), C))
    for t in range(T):
        acc += a["value"][int(a["tree_offset"][t]) + leaves(a, X32, t)]
    return acc / T


def gb_raw(a, Xs):
    X32 = Xs.astype(np.float32)
    K = len(a["init"])
    T = len(a["tree_offset"]) - 1
    raw = np.tile(a["init"], (len(Xs), 1))
    lr = float(a["learning_rate"])
    for t in range(T):
        raw[:, t % K] += lr * a["value"][int(a["tree_offset"][t]) + leaves(a, X32, t)]
    return raw


def gb_proba(raw):
    if raw.shape[1] == 1:
        p = 1.0 / (1.0 + np.exp(-raw[:, 0]))  # scipy.special.expit
        return np.stack([1 - p, p], axis=1)
    e = np.exp(raw - np.amax(raw, axis=1, keepdims=True))  # scipy.special.softmax
    return e / np.sum(e, axis=1, keepdims=True)


def gb_predict(raw):
    return (raw[:, 0] >= 0).astype(np.int64) if raw.shape[1] == 1 else np.argmax(raw, axis=1)


def svc_decision(a, Xs):
    """[B, n_pairs] libsvm decision values (pairs (i, j), i < j, in row-major order)."""
    sv, coef, ns = a["sv"], a["dual_coef"], a["n_support"]
    C = len(ns)
    d = Xs[:, None, :] - sv[None, :, :]
    k = np.exp(-float(a["gamma"]) * np.einsum("bsf,bsf->bs", d, d))
    start = np.concatenate([[0], np.cumsum(ns)])
    rho = -a["intercept"]
    out, p = [], 0
    for i in range(C):
        for j in range(i + 1, C):
            si, sj = slice(start[i], start[i + 1]), slice(start[j], start[j + 1])
            s = k[:, si] @ coef[j - 1, si] + k[:, sj] @ coef[i, sj]
            out.append(s - rho[p])
            p += 1
    return np.stack(out, axis=1)


def svc_predict(dec, C):
    votes = np.zeros((len(dec), C), np.int64)
    p = 0
    for i in range(C):
        for j in range(i + 1, C):
            win = dec[:, p] > 0
            votes[win, i] += 1
            votes[~win, j] += 1
            p += 1
    return np.argmax(votes, axis=1)  # first maximum: ties go to the lower class index


def _sigmoid(f, A, B):
    fApB = f * A + B
    if fApB >= 0:
        return np.exp(-fApB) / (1.0 + np.exp(-fApB))
    return 1.0 / (1 + np.exp(fApB))


def multiclass_probability(r):
    """Wu, Lin and Weng's method 2 as libsvm iterates it."""
    k = len(r)
    Q = np.zeros((k, k))
    p = np.full(k, 1.0 / k)
    for t in range(k):
        for j in range(t):
            Q[t, t] += r[j, t] * r[j, t]
            Q[t, j] = Q[j, t]
        for j in range(t + 1, k):
            Q[t, t] += r[j, t] * r[j, t]
            Q[t, j] = -r[j, t] * r[t, j]
    Qp = np.zeros(k)
    for _ in range(max(100, k)):
        pQp = 0.0
        for t in range(k):
            Qp[t] = 0.0
            for j in range(k):
                Qp[t] += Q[t, j] * p[j]
            pQp += p[t] * Qp[t]
        if max(abs(Qp[t] - pQp) for t in range(k)) < 0.005 / k:
            break
        for t in range(k):
            diff = (-Qp[t] + pQp) / Q[t, t]
            p[t] += diff
            pQp = (pQp + diff * (diff * Q[t, t] + 2 * Qp[t])) / (1 + diff) / (1 + diff)
            for j in range(k):
                Qp[j] = (Qp[j] + diff * Q[t, j]) / (1 + diff)
                p[j] /= 1 + diff
    return p


def svc_proba(a, dec):
    C = len(a["n_support"])
    out = np.empty((len(dec), C))
    for b in range(len(dec)):
        r = np.zeros((C, C))
        p = 0
        for i in range(C):
            for j in range(i + 1, C):
                v = _sigmoid(dec[b, p], a["prob_a"][p], a["prob_b"][p])
                r[i, j] = min(max(v, 1e-7), 1 - 1e-7)
                r[j, i] = 1 - r[i, j]
                p += 1
        out[b] = multiclass_probability(r)
    return out


def predict(a, X):
    """(labels int64 [B], proba float64 [B, C]) the device returns for unscaled rows ``X``."""
    kind = int(a["kind"])
    Xs = scale(a, X)
    C = len(a["classes"])
    if kind == KIND_RF:
        proba = rf_proba(a, Xs)
        return np.argmax(proba, axis=1), proba
    bad = np.isnan(Xs).any(axis=1)
    Xc = np.where(bad[:, None], 0.0, Xs)
    if kind == KIND_GB:
        raw = gb_raw(a, Xc)
        labels, proba = gb_predict(raw), gb_proba(raw)
    else:
        dec = svc_decision(a, Xc)
        labels, proba = svc_predict(dec, C), svc_proba(a, dec)
    labels = np.where(bad, -1, labels)
    proba[bad] = np.nan
    return labels, proba
