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

The functions above leave three summation orders to NumPy (``np.sum``, ``@``, ``einsum``).  include/uwie.h fixes them, and the
``*_seq`` functions at the end of the file state them: the softmax's sum class by class, the squared distance feature by
feature, the decision value over class i's vectors and then class j's, every step one rounded float64 operation.
``predict_seq`` is ``predict`` with them; ``multiclass_probability_rows`` is ``multiclass_probability`` for all rows at once
(the same operations in the same order per row), and also reports each row's iteration count and stopping errors.
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


# ------------------------------------------------------------------ the contract's own orders (include/uwie.h)
def _serial_sum(terms):
    """((0 + t_0) + t_1) + ... along the last axis: ``np.add.accumulate`` adds one element at a time."""
    if terms.shape[-1] == 0:
        return np.zeros(terms.shape[:-1])
    return np.add.accumulate(terms, axis=-1)[..., -1]


def leaf_table(a, Xs):
    """[T, B] global node index of every row's leaf in every tree (what the tree kernel keeps in LDS)."""
    X32 = Xs.astype(np.float32)
    T = len(a["tree_offset"]) - 1
    return np.stack([int(a["tree_offset"][t]) + leaves(a, X32, t) for t in range(T)])


def rf_proba_from_leaves(a, L):
    acc = np.zeros((L.shape[1], a["value"].shape[1]))
    for t in range(len(L)):
        acc += a["value"][L[t]]
    return acc / len(L)


def gb_raw_from_leaves(a, L):
    K = len(a["init"])
    raw = np.tile(a["init"], (L.shape[1], 1))
    lr = float(a["learning_rate"])
    for t in range(len(L)):
        raw[:, t % K] += lr * a["value"][L[t]]
    return raw


def gb_proba_seq(raw):
    """``exp(raw - max) / sequential sum`` (binary: ``gb_proba``'s expit, which has no sum)."""
    if raw.shape[1] == 1:
        return gb_proba(raw)
    e = np.exp(raw - np.amax(raw, axis=1, keepdims=True))
    return e / _serial_sum(e)[:, None]


def svc_sqdist_seq(a, Xs):
    """[B, S] squared distances, ``d = 0; d += (x[f] - sv[f]) ** 2`` for f = 0, 1, ..."""
    sv = a["sv"]
    d = np.zeros((len(Xs), len(sv)))
    for f in range(sv.shape[1]):
        diff = Xs[:, f, None] - sv[None, :, f]
        d += diff * diff
    return d


def svc_kernel_seq(a, Xs):
    return np.exp(-float(a["gamma"]) * svc_sqdist_seq(a, Xs))


def svc_decision_from_kernel(a, k):
    """libsvm's ``sum`` of svm_predict_values: from 0, class i's vectors (coefficient row j - 1) one by one, then class j's
    (row i), then ``- rho``."""
    coef, ns = a["dual_coef"], a["n_support"]
    C = len(ns)
    start = np.concatenate([[0], np.cumsum(ns)]).astype(np.int64)
    rho = -a["intercept"]
    out = np.empty((len(k), C * (C - 1) // 2))
    p = 0
    for i in range(C):
        si = slice(start[i], start[i + 1])
        for j in range(i + 1, C):
            sj = slice(start[j], start[j + 1])
            terms = np.concatenate([k[:, si] * coef[j - 1, si], k[:, sj] * coef[i, sj]], axis=1)
            out[:, p] = _serial_sum(terms) - rho[p]
            p += 1
    return out


def svc_decision_seq(a, Xs):
    return svc_decision_from_kernel(a, svc_kernel_seq(a, Xs))


def pairwise_r(a, dec):
    """[B, C, C] clamped Platt probabilities of svm_predict_probability."""
    C = len(a["n_support"])
    r = np.zeros((len(dec), C, C))
    p = 0
    for i in range(C):
        for j in range(i + 1, C):
            fApB = dec[:, p] * a["prob_a"][p] + a["prob_b"][p]
            with np.errstate(over="ignore"):
                v = np.where(fApB >= 0, np.exp(-fApB) / (1.0 + np.exp(-fApB)), 1.0 / (1 + np.exp(fApB)))
            r[:, i, j] = np.minimum(np.maximum(v, 1e-7), 1 - 1e-7)
            r[:, j, i] = 1 - r[:, i, j]
            p += 1
    return r


def multiclass_probability_rows(r):
    """``multiclass_probability`` for every row of ``r`` [B, k, k]: the same float64 operations in the same order per row
    (a row that has stopped is left alone).  Returns ``(p [B, k], iterations [B], errors)``; ``errors[n]`` is the
    ``max_error`` each row saw at its check number n (NaN once the row has stopped), ``iterations`` the number of updates a
    row made (``max_iter`` if it never passed the check)."""
    B, k = r.shape[0], r.shape[1]
    Q = np.zeros((B, k, k))
    for t in range(k):
        for j in range(t):
            Q[:, t, t] += r[:, j, t] * r[:, j, t]
            Q[:, t, j] = Q[:, j, t]
        for j in range(t + 1, k):
            Q[:, t, t] += r[:, j, t] * r[:, j, t]
            Q[:, t, j] = -r[:, j, t] * r[:, t, j]
    p = np.full((B, k), 1.0 / k)
    live = np.ones(B, bool)
    iters = np.zeros(B, np.int64)
    errors = []
    max_iter, eps = max(100, k), 0.005 / k
    for _ in range(max_iter):
        rows = np.flatnonzero(live)
        if rows.size == 0:
            break
        Ql, pl = Q[rows], p[rows]
        Qp = _serial_sum(Ql * pl[:, None, :])  # Qp[t] = ((0 + Q[t,0] p[0]) + Q[t,1] p[1]) + ...
        pQp = _serial_sum(pl * Qp)
        err = np.abs(Qp - pQp[:, None]).max(axis=1)
        e = np.full(B, np.nan)
        e[rows] = err
        errors.append(e)
        go = err >= eps
        live[rows[~go]] = False
        rows, Ql, pl, Qp, pQp = rows[go], Ql[go], pl[go], Qp[go], pQp[go]
        if rows.size == 0:
            break
        for t in range(k):
            qtt = Ql[:, t, t]
            diff = (-Qp[:, t] + pQp) / qtt
            pl[:, t] += diff
            pQp = (pQp + diff * (diff * qtt + 2 * Qp[:, t])) / (1 + diff) / (1 + diff)
            Qp = (Qp + diff[:, None] * Ql[:, t, :]) / (1 + diff)[:, None]
            pl /= (1 + diff)[:, None]
        p[rows] = pl
        iters[rows] += 1
    return p, iters, errors


def svc_proba_seq(a, dec):
    return multiclass_probability_rows(pairwise_r(a, dec))[0]


def predict_seq(a, X):
    """``predict`` in the header's summation orders."""
    kind = int(a["kind"])
    Xs = scale(a, X)
    C = len(a["classes"])
    if kind == KIND_RF:
        proba = rf_proba_from_leaves(a, leaf_table(a, Xs))
        return np.argmax(proba, axis=1), proba
    bad = np.isnan(Xs).any(axis=1)
    Xc = np.where(bad[:, None], 0.0, Xs)
    if kind == KIND_GB:
        raw = gb_raw_from_leaves(a, leaf_table(a, Xc))
        labels, proba = gb_predict(raw), gb_proba_seq(raw)
    else:
        dec = svc_decision_seq(a, Xc)
        labels, proba = svc_predict(dec, C), svc_proba_seq(a, dec)
    labels = np.where(bad, -1, labels)
    proba[bad] = np.nan
    return labels, proba
