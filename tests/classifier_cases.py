"""Seeded strategy-classifier models at the sizes uwie_model_check admits and csrc/k_classify.hip's loops are built around
(256 threads, 1024 kernel values per chunk, two pairs per lane), with their query rows.  No GPU, no scikit-learn, nothing
committed: every model is an export dict (what ``classifier.model_desc`` takes) built in code.

* trees are in pre-order (children strictly after their parent); thresholds are float32 values or midpoints of two adjacent
  float32 values, as scikit-learn's splitter produces; ``missing_left`` takes both values; features cover ``0 .. F-1`` and,
  for F > 256, two internal nodes in five are drawn from ``256 .. F-1``.  The leaves hold what the query rows that reach them
  say (class fractions for RF, a signed share for GB), so the forests answer their rows with a clear margin.
* the scaler is the identity on every third feature (the rows planted on a threshold need an exact scaled value there) and a
  seeded mean / scale elsewhere.
* every model has ROWS rows; SLICE is the 37-row slice the batch tests cut.  Row NAN_ROW holds one NaN in feature F - 1 (GB,
  SVC); RF rows NAN_ROW .. NAN_ROW + 5 hold NaN in features below and, where there are any, from 256 on.  Rows from EDGE_ROW
  on are planted on nodes one below a root: four with ``float32(v) == thr < v`` (float64 would go right, the cast goes left)
  and four with ``v == thr < float32(v)`` (the mirror: a midpoint that rounds to even upwards).

``case(name)`` builds and caches one case; ``reference(name)`` is its sequential-order restatement (computed once, shared by the
CPU and the GPU tests, never modified).  tests/test_classifier_cases.py proves what is claimed here.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np

import classifier_ref as ref

ROWS = 300
SLICE = slice(100, 137)
NAN_ROW = 110
EDGE_ROW = 120
THREADS, CHUNK = 256, 1024  # kClsThreads, kClsChunk
SUB = 2.0 ** -149  # the smallest float32 subnormal


@dataclass
class Case:
    name: str
    kind: str  # "rf" | "gb" | "svc"
    arrays: dict
    X: np.ndarray
    paths: tuple = ()  # which of "feat256", "tree256", "pair256", "sv1024" the model is there for
    exact: bool = False
    edge_rows: tuple = ()  # rows planted on a threshold
    note: dict = field(default_factory=dict)


# ------------------------------------------------------------------ trees
def tree_shape(n_internal, rng, shape="random"):
    """(left, right), tree-local, pre-order.  ``left_chain`` / ``right_chain``: every internal node's other child is a leaf."""
    left, right = [], []
    stack = [(n_internal, -1, 0)]
    while stack:
        n, parent, side = stack.pop()
        i = len(left)
        left.append(-1)
        right.append(-1)
        if parent >= 0:
            (right if side else left)[parent] = i
        if n > 0:
            k = n - 1 if shape == "left_chain" else 0 if shape == "right_chain" else int(rng.integers(0, n))
            stack.append((n - 1 - k, i, 1))
            stack.append((k, i, 0))  # popped first: the left subtree takes the next indices
    return np.array(left, np.int32), np.array(right, np.int32)


def sklearn_threshold(rng, value):
    """A float32 value near ``value``, or the midpoint of it and its upper float32 neighbour."""
    a = np.float32(value)
    if rng.random() < 0.5:
        return float(a)
    return (float(a) + float(np.nextafter(a, np.float32(np.inf)))) / 2


def draw_feature(rng, F):
    if F > THREADS and rng.random() < 0.4:
        return int(rng.integers(THREADS, F))
    return int(rng.integers(0, F))


def grow(rng, X32, F, shapes, leaf_value):
    """Concatenated trees over the float32 rows ``X32``.  ``shapes``: one (shape, n_internal) per tree; ``leaf_value(t, rows)``
    gives a leaf's value from the indices of the rows that reach it."""
    parts = {k: [] for k in ("left", "right", "feature", "threshold", "missing_left", "value")}
    offs = [0]
    for t, (shape, n_int) in enumerate(shapes):
        left, right = tree_shape(n_int, rng, shape)
        n = len(left)
        feat, thr, miss = np.zeros(n, np.int32), np.zeros(n), np.zeros(n, np.uint8)
        reach = {0: np.arange(len(X32))}
        value = [None] * n
        for i in range(n):
            rows = reach.pop(i)
            if left[i] < 0:
                feat[i], thr[i] = -2, -2.0  # scikit-learn's TREE_UNDEFINED
                value[i] = leaf_value(t, rows)
                continue
            f = draw_feature(rng, F)
            x = X32[rows, f]
            if shape == "left_chain":
                c = 2.5 + 0.05 * rng.random()  # two noise widths past the outermost centre: a row in 200 leaves the chain here
            elif shape == "right_chain":
                c = -2.5 - 0.05 * rng.random()
            elif len(rows) >= 2:
                c = np.quantile(x, rng.uniform(0.3, 0.7))
            else:
                c = rng.normal(0, 1)
            feat[i], thr[i], miss[i] = f, sklearn_threshold(rng, c), rng.integers(0, 2)
            go = x <= thr[i]
            reach[int(left[i])], reach[int(right[i])] = rows[go], rows[~go]
        blank = np.zeros_like(next(v for v in value if v is not None))  # an internal node's value is never read
        value = np.array([blank if v is None else v for v in value], np.float64)
        for k, v in (("left", left), ("right", right), ("feature", feat), ("threshold", thr), ("missing_left", miss),
                     ("value", value)):
            parts[k].append(v)
        offs.append(offs[-1] + n)
    out = {k: np.ascontiguousarray(np.concatenate(v)) for k, v in parts.items()}
    out["tree_offset"] = np.asarray(offs, np.int32)
    return out


def tree_shapes(rng, T, lo=4, hi=16):
    """A lone leaf, a stump, both chains of 300 internal nodes (as far as T allows), then random shapes."""
    fixed = [("random", 0), ("random", 1), ("left_chain", 300), ("right_chain", 300)]
    shapes = [("random", int(rng.integers(lo, hi + 1))) for _ in range(T)]
    if T == 1:
        return shapes
    for k, s in enumerate(fixed[:T - 1]):  # spread over the forest; the last tree (often index >= 256) takes one too
        shapes[(k * 97 + 1) % T if k < 3 else T - 1] = s
    return shapes


def scaler(rng, F):
    mean, scale = rng.normal(0, 2, F), rng.uniform(0.25, 4, F)
    mean[::3], scale[::3] = 0.0, 1.0
    return mean, scale


def cluster_rows(rng, F, C, mean, scale):
    """ROWS rows around one centre per class (label ``row % C``), unscaled, and their scaled float32 values."""
    y = np.arange(ROWS) % C
    centres = np.stack([rng.permutation(np.linspace(-2, 2, C)) for _ in range(F)], axis=1)
    Xs = centres[y] + rng.normal(0, 0.25 if F > 1 else 0.5 / C, (ROWS, F))
    X = Xs * scale + mean
    return X, y, ((X - mean) / scale).astype(np.float32)


def plant_edge_rows(rng, a, X, F, T):
    """Move EDGE_ROW .. EDGE_ROW + 7 onto thresholds of nodes one below a root (see the module docstring)."""
    if F < 4:
        return ()
    planted = []
    X32 = ref.scale(a, X).astype(np.float32)
    trees = [t for t in range(T - 1, -1, -1) if a["tree_offset"][t + 1] - a["tree_offset"][t] >= 5][:64]
    for t in trees:
        if len(planted) == 8:
            break
        o = int(a["tree_offset"][t])
        side = [s for s in ("left", "right") if a["left"][o + a[s][o]] >= 0]
        if not side:
            continue
        node = o + int(a[side[0]][o])
        f0 = int(a["feature"][o])
        f = 3 * int(rng.integers(0, (F + 2) // 3))
        if f == f0:
            continue
        went_left = X32[:, f0] <= a["threshold"][o]
        base = np.flatnonzero(went_left == (side[0] == "left"))
        base = base[(base < SLICE.start) | (base >= EDGE_ROW + 8)]
        if base.size == 0:
            continue
        a32 = np.float32(rng.normal(0, 1))
        if len(planted) < 4:  # float32(v) == thr < v
            thr, v = float(a32), float(np.nextafter(float(a32), np.inf))
        else:  # v == thr < float32(v): a midpoint whose upper neighbour has the even mantissa
            if (a32.view(np.uint32) & 1) == 0:
                a32 = np.nextafter(a32, np.float32(np.inf))
            b32 = np.nextafter(a32, np.float32(np.inf))
            thr = v = (float(a32) + float(b32)) / 2
            assert np.float32(v) == b32 and float(b32) > thr
        a["feature"][node], a["threshold"][node] = f, thr
        r = EDGE_ROW + len(planted)
        X[r] = X[base[0]]
        X[r, f] = v  # feature f is identity-scaled: the scaled value is v exactly
        planted.append(r)
    return tuple(planted)  # eight wherever the forest has eight trees to plant on


def plant_nan_rows(a, X, F, T, kind):
    if kind != "rf":
        X[NAN_ROW, F - 1] = np.nan
        return
    roots = a["feature"][a["tree_offset"][:-1]]
    low = [int(f) for f in roots if 0 <= f < THREADS] or [0]
    high = [int(f) for f in roots if f >= THREADS]
    for k in range(6):
        r = NAN_ROW + k
        if k % 3 != 1 or not high:
            X[r, low[k % len(low)]] = np.nan
        if k % 3 != 0 and high:
            X[r, high[k % len(high)]] = np.nan


def _base(kind, C, mean, scale):
    return {"kind": {"rf": ref.KIND_RF, "gb": ref.KIND_GB, "svc": ref.KIND_SVC}[kind],
            "classes": np.array([f"class_{c:02d}" for c in range(C)]), "mean": mean, "scale": scale}


def rf_case(name, T, F, C, seed, paths=()):
    rng = np.random.default_rng(seed)
    mean, scale = scaler(rng, F)
    X, y, X32 = cluster_rows(rng, F, C, mean, scale)

    def leaf_value(t, rows):
        counts = np.bincount(y[rows], minlength=C).astype(np.float64)
        if counts.sum() == 0:
            counts[rng.integers(0, C)] = 1.0
        if T == 1:  # one tree: a margin of 1 / T needs pure leaves
            counts = (np.arange(C) == np.argmax(counts)).astype(np.float64)
        return counts / counts.sum()

    a = _base("rf", C, mean, scale)
    a.update(grow(rng, X32, F, tree_shapes(rng, T), leaf_value))
    edge = plant_edge_rows(rng, a, X, F, T)
    plant_nan_rows(a, X, F, T, "rf")
    return Case(name, "rf", a, X, paths, edge_rows=edge)


def gb_case(name, C, stages, F, seed, paths=()):
    rng = np.random.default_rng(seed)
    K = 1 if C == 2 else C
    T = stages * K
    lr = 0.1
    vmax = 7.0 / (lr * stages)  # |raw| <= |init| + lr * stages * vmax <= 0.5 + 7
    mean, scale = scaler(rng, F)
    X, y, X32 = cluster_rows(rng, F, C, mean, scale)

    def leaf_value(t, rows):
        k = t % K if K > 1 else 1
        if len(rows) == 0:
            return rng.uniform(-vmax, vmax)
        share = np.mean(y[rows] == k)
        return vmax * (0.9 * (2 * share - 1) + 0.05 * rng.uniform(-1, 1))

    a = _base("gb", C, mean, scale)
    a.update(grow(rng, X32, F, tree_shapes(rng, T, 2, 8), leaf_value))
    a["learning_rate"], a["init"] = np.float64(lr), rng.uniform(-0.5, 0.5, K)
    edge = plant_edge_rows(rng, a, X, F, T)
    plant_nan_rows(a, X, F, T, "gb")
    return Case(name, "gb", a, X, paths, edge_rows=edge)


def svc_case(name, n_support, F, seed, paths=()):
    rng = np.random.default_rng(seed)
    ns = np.asarray(n_support, np.int32)
    C, S = len(ns), int(ns.sum())
    P = C * (C - 1) // 2
    cls = np.repeat(np.arange(C), ns)
    gamma = rng.uniform(0.4, 1.0)
    # a class of n vectors is spread so wide that a row inside it sees a kernel sum of about three, whatever n is (a fitted
    # model's decision values are O(1)): E exp(-gamma d^2) = (1 + 4 gamma sigma^2)^(-F/2) for two points of the blob
    sigma = np.sqrt(np.maximum((np.maximum(ns, 1) / 3.0) ** (2.0 / F) - 1, 0.3) / (4 * gamma))
    centres = rng.normal(0, 2.5 * sigma.mean(), (C, F))
    sv = centres[cls] + rng.normal(0, 1, (S, F)) * sigma[cls, None]
    coef = np.zeros((C - 1, S))
    for o in range(C):  # the coefficient of a class-c vector against class o: + on the pair's i side, - on its j side
        for c in range(C):
            if o != c:
                rows = o - 1 if o > c else o
                coef[rows, cls == c] = (1 if c < o else -1) * rng.uniform(0.1, 1.0, int(ns[c]))
    mean, scale = scaler(rng, F)
    a = _base("svc", C, mean, scale)
    a.update({"sv": sv, "dual_coef": coef, "intercept": rng.normal(0, 0.3, P), "n_support": ns,
              "gamma": np.float64(gamma), "prob_b": rng.normal(0, 0.3, P)})
    pick = rng.integers(0, S, ROWS)
    pick[:min(S, ROWS)] = np.linspace(0, S - 1, min(S, ROWS)).astype(np.int64)  # every class with vectors is queried
    Xs = sv[pick] + rng.normal(0, 0.3, (ROWS, F))
    X = Xs * scale + mean
    # Platt slopes sized to the decision values: a typical |A * dec| of one or two
    dec = ref.svc_decision_seq(a, ref.scale(a, X))
    a["prob_a"] = -rng.uniform(1.0, 3.0, P) / np.median(np.abs(dec))
    plant_nan_rows(a, X, F, 0, "svc")
    return Case(name, "svc", a, X, paths)


def _split(S, C):
    return [S // C + (1 if c < S % C else 0) for c in range(C)]


# ------------------------------------------------------------------ float32 subnormals (identity scaler)
def subnormal_case(name, kind, seed):
    """Thresholds ``(k + 0.5) * 2^-149`` (midpoints of two subnormals) against rows ``(k' + q / 4) * 2^-149``."""
    rng = np.random.default_rng(seed)
    F, C, n_rows = 4, 4 if kind == "rf" else 3, 64
    k_rows = rng.integers(-64, 65, (n_rows, F))
    X = (k_rows + rng.integers(0, 4, (n_rows, F)) / 4.0) * SUB
    X32 = X.astype(np.float32)
    K = 1 if kind == "rf" else C
    T = 1 if kind == "rf" else 4 * K
    leaf = iter(range(10 ** 6))

    def leaf_value(t, rows):
        if kind == "rf":
            return (np.arange(C) == next(leaf) % C).astype(np.float64)
        return rng.uniform(-2, 2)

    a = _base(kind, C, np.zeros(F), np.ones(F))
    a.update(grow(rng, X32, F, [("random", 9)] * T, leaf_value))
    internal = a["left"] >= 0
    a["threshold"][internal] = (rng.integers(-48, 48, int(internal.sum())) + 0.5) * SUB
    # rows 0 .. 7 sit on a root's threshold (k + 0.5) * 2^-149 with k odd: the cast rounds to the even k + 1 and goes right
    # where the float64 value would go left
    roots = a["tree_offset"][:-1]
    a["threshold"][roots] = (2 * rng.integers(-24, 24, T) + 1.5) * SUB
    for r in range(8):
        X[r, a["feature"][roots[r % T]]] = a["threshold"][roots[r % T]]
    if kind == "gb":
        a["learning_rate"], a["init"] = np.float64(0.1), np.zeros(K)
    return Case(name, kind, a, X, exact=False)


# ------------------------------------------------------------------ exact cases
def _stumps(F, feats, thrs, values, C=None):
    """One stump per (feature, threshold, (left value, right value))."""
    T = len(feats)
    a = {"tree_offset": np.arange(0, 3 * T + 1, 3, dtype=np.int32), "left": np.tile(np.int32([1, -1, -1]), T),
         "right": np.tile(np.int32([2, -1, -1]), T), "feature": np.zeros(3 * T, np.int32), "threshold": np.zeros(3 * T),
         "missing_left": np.zeros(3 * T, np.uint8)}
    a["feature"][0::3], a["threshold"][0::3] = feats, thrs
    v = np.zeros((3 * T,) + np.shape(values[0][0]))
    for t, (lv, rv) in enumerate(values):
        v[3 * t + 1], v[3 * t + 2] = lv, rv
    a["value"] = v
    return a


def _grid_rows(F, n=12):
    g = np.linspace(-1.1, 1.1, n)
    return np.stack([np.roll(g, f) for f in range(F)], axis=1)


def exact_rf_tie():
    """T = 4 stumps, dyadic fractions: classes 1 and 2 tie at every row (class 0 stays below): the first maximum, 1, wins."""
    def swap(v):
        return [v[0], v[2], v[1]]

    l0, r0, l1, r1 = [0.25, 0.5, 0.25], [0.0, 0.25, 0.75], [0.125, 0.75, 0.125], [0.25, 0.0, 0.75]
    # trees 0 / 2 and 1 / 3 split alike with classes 1 and 2 exchanged: the two classes' sums are equal on either side
    values = [(l0, r0), (l1, r1), (swap(l0), swap(r0)), (swap(l1), swap(r1))]
    a = _base("rf", 3, np.zeros(2), np.ones(2))
    a.update(_stumps(2, [0, 1, 0, 1], [0.25, -0.5, 0.25, -0.5], values))
    return Case("exact_rf_tie", "rf", a, _grid_rows(2), exact=True, note={"label": 1})


def exact_gb_tie():
    """Classes 1 and 2 have equal trees and init, class 0 lies 800 below: exp underflows to 0, proba is [0, 0.5, 0.5]."""
    feats, thrs, values = [], [], []
    for s, (f, th, v) in enumerate([(0, 0.0, 0.75), (1, 0.5, -0.5), (0, -0.25, 1.25)]):
        for k in range(3):
            feats.append(f)
            thrs.append(th)
            values.append((v, -v) if k else (0.125, -0.125))
    a = _base("gb", 3, np.zeros(2), np.ones(2))
    a.update(_stumps(2, feats, thrs, values))
    a["learning_rate"], a["init"] = np.float64(0.1), np.array([-800.0, 0.25, 0.25])
    return Case("exact_gb_tie", "gb", a, _grid_rows(2), exact=True, note={"label": 1, "proba": [0.0, 0.5, 0.5]})


def exact_gb_zero():
    """Binary, learning_rate 0.5, two equal stumps with leaves +v / -v and -v / +v: raw = 0 + 0.5 v - 0.5 v = 0 exactly."""
    a = _base("gb", 2, np.zeros(2), np.ones(2))
    a.update(_stumps(2, [1, 1], [0.125, 0.125], [(0.75, -1.5), (-0.75, 1.5)]))
    a["learning_rate"], a["init"] = np.float64(0.5), np.array([0.0])
    return Case("exact_gb_zero", "gb", a, _grid_rows(2), exact=True, note={"label": 1, "proba": [0.5, 0.5]})


def _zero_coef_svc(name, C, intercept, note):
    rng = np.random.default_rng(C)
    ns = np.full(C, 2, np.int32)
    P = C * (C - 1) // 2
    a = _base("svc", C, np.zeros(3), np.ones(3))
    icpt = np.asarray(intercept, np.float64)
    # A * dec + B = -dec + dec = 0 exactly: every pairwise probability is 0.5 and proba is 1 / C
    a.update({"sv": rng.normal(0, 1, (2 * C, 3)), "dual_coef": np.zeros((C - 1, 2 * C)), "intercept": icpt, "n_support": ns,
              "gamma": np.float64(0.5), "prob_a": np.full(P, -1.0), "prob_b": icpt.copy()})
    return Case(name, "svc", a, _grid_rows(3), exact=True, note=note)


def exact_svc_zero():
    """dual_coef = 0 and intercept = 0: every decision value is 0, every pair votes j, class C - 1 collects C - 1 votes."""
    return _zero_coef_svc("exact_svc_zero", 6, np.zeros(15), {"label": 5, "proba": [1 / 6] * 6})


def exact_svc_cycle():
    """dec(0,1) = 1 > 0, dec(0,2) = -1, dec(1,2) = 1: one vote each, the first maximum, 0, wins."""
    return _zero_coef_svc("exact_svc_cycle", 3, [1.0, -1.0, 1.0], {"label": 0, "proba": [1 / 3] * 3})


# ------------------------------------------------------------------ the table
# seeds at which every |decision value| >= 1e-5, no row's vote ties, and no max_error comes within 1e-8 of the stopping
# bound (tests/test_classifier_cases.py asserts the issue's 1e-6 / 1e-9); found by counting upwards in steps of 10000
SVC_SEEDS = {"svc_S5": 505005, "svc_S1023": 616023, "svc_S1024": 86024, "svc_S1025": 316025, "svc_S2049": 757049,
             "svc_straddle": 775101, "svc_three_chunks": 115102, "svc_empty_class": 155103, "svc_C23": 195323,
             "svc_C24": 275324, "svc_C25": 145325, "svc_C32": 615332}


def _svc_wide(C, per, seed):
    rng = np.random.default_rng(seed)
    return [int(v) for v in rng.integers(per - per // 4, per + per // 4 + 1, C)]


BUILDERS = {}
for _T in (1, 255, 256, 257, 513):
    BUILDERS[f"rf_T{_T}"] = functools.partial(rf_case, f"rf_T{_T}", _T, 79, 5, 1000 + _T, ("tree256",) if _T > 256 else ())
for _F in (1, 255, 256, 257, 1024):
    BUILDERS[f"rf_F{_F}"] = functools.partial(rf_case, f"rf_F{_F}", 200, _F, 5, 2000 + _F, ("feat256",) if _F > 256 else ())
BUILDERS["rf_T4096_F1024_C32"] = functools.partial(rf_case, "rf_T4096_F1024_C32", 4096, 1024, 32, 3000, ("tree256", "feat256"))
BUILDERS["gb_C2_T300_F257"] = functools.partial(gb_case, "gb_C2_T300_F257", 2, 300, 257, 4002, ("tree256", "feat256"))
BUILDERS["gb_C3_T300"] = functools.partial(gb_case, "gb_C3_T300", 3, 100, 79, 4003, ("tree256",))
# (seed: of 4032, 4132, ... the first at which all 32 labels occur and np.sum's pairwise softmax sum, which at K = 32 is a
# last bit or two away from the sequential sum, leaves proba within 1e-16 of the sequential statement: 8.3e-17; the seeds
# before it gave 1.1e-16 or fewer labels)
BUILDERS["gb_C32_T1280_F257"] = functools.partial(gb_case, "gb_C32_T1280_F257", 32, 40, 257, 4532, ("tree256", "feat256"))
for _S in (5, 1023, 1024, 1025, 2049):
    BUILDERS[f"svc_S{_S}"] = functools.partial(svc_case, f"svc_S{_S}", _split(_S, 5), 3 + _S % 4, SVC_SEEDS[f"svc_S{_S}"],
                                               ("sv1024",) if _S > 1024 else ())
BUILDERS["svc_straddle"] = functools.partial(svc_case, "svc_straddle", [500, 900, 300, 200, 100], 4, SVC_SEEDS["svc_straddle"], ("sv1024",))
BUILDERS["svc_three_chunks"] = functools.partial(svc_case, "svc_three_chunks", [300, 2500, 200, 100, 100], 3, SVC_SEEDS["svc_three_chunks"], ("sv1024",))
BUILDERS["svc_empty_class"] = functools.partial(svc_case, "svc_empty_class", [40, 0, 50, 30, 30], 5, SVC_SEEDS["svc_empty_class"])
for _C, _per in ((23, 50), (24, 50), (25, 50), (32, 75)):
    BUILDERS[f"svc_C{_C}"] = functools.partial(svc_case, f"svc_C{_C}", _svc_wide(_C, _per, 5200 + _C), 6, SVC_SEEDS[f"svc_C{_C}"],
                                               ("sv1024",) + (("pair256",) if _C >= 24 else ()))
BUILDERS["rf_subnormal"] = functools.partial(subnormal_case, "rf_subnormal", "rf", 6001)
BUILDERS["gb_subnormal"] = functools.partial(subnormal_case, "gb_subnormal", "gb", 6002)
for _fn in (exact_rf_tie, exact_gb_tie, exact_gb_zero, exact_svc_zero, exact_svc_cycle):
    BUILDERS[_fn.__name__] = _fn

NAMES = list(BUILDERS)
LARGE = {"rf": "rf_T4096_F1024_C32", "gb": "gb_C32_T1280_F257", "svc": "svc_C32"}  # one model of each kind from the large end


def kind_of(name) -> str:
    """ "rf" | "gb" | "svc", read off the name (so that a test module can sort the table without building it)."""
    return name.replace("exact_", "").split("_")[0]


@functools.lru_cache(maxsize=None)
def case(name) -> Case:
    c = BUILDERS[name]()
    assert c.kind == kind_of(name) and c.exact == name.startswith("exact_")
    for v in c.arrays.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    c.X.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def reference(name):
    """(labels, proba) of ``ref.predict_seq``, read-only."""
    c = case(name)
    labels, proba = ref.predict_seq(c.arrays, c.X)
    labels.setflags(write=False)
    proba.setflags(write=False)
    return labels, proba


def counts(c: Case) -> dict:
    """How much of the model lies on each of the kernel's later trips."""
    a = c.arrays
    out = {"feat256": 0, "tree256": 0, "pair256": 0, "sv1024": 0}
    C = len(a["classes"])
    if c.kind == "svc":
        out["pair256"] = max(0, C * (C - 1) // 2 - THREADS)
        out["sv1024"] = max(0, len(a["sv"]) - CHUNK)
    else:
        out["feat256"] = int(np.count_nonzero((a["left"] >= 0) & (a["feature"] >= THREADS)))
        out["tree256"] = max(0, len(a["tree_offset"]) - 1 - THREADS)
        out["internal"] = int(np.count_nonzero(a["left"] >= 0))
    return out
