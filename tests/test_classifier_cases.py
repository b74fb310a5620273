"""What the models and rows of tests/classifier_cases.py are for, proven on the NumPy statement of the contract
(tests/classifier_ref.py) alone: no device.  tests/test_gpu_classifier_limits.py then holds csrc/k_classify.hip to the same
statement on the same cases."""
import ctypes
import functools

import numpy as np
import pytest

import classifier_cases as K
import classifier_ref as ref
import underwater_image_enhancement_amd as uw
from underwater_image_enhancement_amd.classifier import model_check, model_desc

BOUND = {"rf": 0.0, "gb": 1e-15, "svc": 1e-9}  # include/uwie.h: bit for bit, the device's exp, multiclass_probability
TABLE = [n for n in K.NAMES if not n.startswith("exact_")]  # (nothing is built at import: K.kind_of reads the name)
EXACT = [n for n in K.NAMES if n.startswith("exact_")]
TREES = [n for n in TABLE if K.kind_of(n) != "svc"]
SVCS = [n for n in TABLE if K.kind_of(n) == "svc"]


def n_trees(a):
    return len(a["tree_offset"]) - 1


@functools.lru_cache(maxsize=None)
def scaled(name):
    """(scaled rows with GB / SVC NaN rows zeroed as ``ref.predict`` does, the NaN-row mask)."""
    c = K.case(name)
    Xs = ref.scale(c.arrays, c.X)
    bad = np.isnan(Xs).any(axis=1) if c.kind != "rf" else np.zeros(len(Xs), bool)
    return np.where(bad[:, None], 0.0, Xs), bad


# ------------------------------------------------------------------ uwie_model_check
def test_model_check_accepts_the_whole_table():
    lib = uw.load()
    for name in K.NAMES:
        assert model_check(K.case(name).arrays) == 0, (name, lib.uwie_last_error())


def test_model_check_rejects_one_past_each_limit():
    """The counts are checked before any array is read at them, so the arrays of a small model stand under the larger
    count: F = 1025, C = 33, T = 4097, S = 65537, and for contrast the limits themselves over the table's own models."""
    lib = uw.load()
    for name, fld, value, word in (("exact_rf_tie", "n_features", 1025, "n_features"), ("exact_rf_tie", "n_classes", 33, "n_classes"),
                                   ("exact_rf_tie", "n_trees", 4097, "n_trees"), ("exact_svc_zero", "n_sv", 65537, "n_sv")):
        m, _keep = model_desc(K.case(name).arrays)
        assert lib.uwie_model_check(ctypes.byref(m)) == 0
        setattr(m, fld, value)
        assert lib.uwie_model_check(ctypes.byref(m)) == -1, fld
        assert word in lib.uwie_last_error().decode(), (fld, lib.uwie_last_error())
    big = K.case("rf_T4096_F1024_C32").arrays
    assert (n_trees(big), big["mean"].size, big["classes"].size) == (4096, 1024, 32)


# ------------------------------------------------------------------ the builder's claims
@pytest.mark.parametrize("name", [n for n in K.NAMES if K.kind_of(n) != "svc"])
def test_trees_are_what_the_docstring_says(name):
    a = K.case(name).arrays
    F = a["mean"].size
    internal = a["left"] >= 0
    for t in range(n_trees(a)):
        o, e = int(a["tree_offset"][t]), int(a["tree_offset"][t + 1])
        idx = np.arange(e - o)
        inner = internal[o:e]
        assert (a["left"][o:e][inner] > idx[inner]).all() and (a["right"][o:e][inner] > idx[inner]).all()
        assert (a["left"][o:e][inner] < e - o).all() and (a["right"][o:e][inner] < e - o).all()
        assert (a["right"][o:e][~inner] == -1).all()
    feat, thr = a["feature"][internal], a["threshold"][internal]
    assert feat.min() >= 0 and feat.max() < F
    lo = thr.astype(np.float32)
    lo = np.where(lo.astype(np.float64) > thr, np.nextafter(lo, np.float32(-np.inf)), lo)
    mid = (lo.astype(np.float64) + np.nextafter(lo, np.float32(np.inf)).astype(np.float64)) / 2
    assert ((thr == lo) | (thr == mid)).all()  # a float32 value or a midpoint of two neighbours
    if name in TABLE and internal.sum() >= 50 and not name.endswith("subnormal"):
        assert set(a["missing_left"][internal].tolist()) == {0, 1}
        assert (thr == lo).any() and (thr == mid).any()
    if F > K.THREADS:
        assert 3 * np.count_nonzero(feat >= K.THREADS) >= feat.size, name
        assert feat.max() == F - 1 or F > 300
    if name in TABLE and F >= 255:
        assert feat.min() == 0 and feat.max() >= F - 8


@pytest.mark.parametrize("name", ["rf_T255", "rf_T513", "rf_F1024", "rf_T4096_F1024_C32", "gb_C2_T300_F257", "gb_C32_T1280_F257"])
def test_tree_shapes_include_the_leaf_the_stump_and_both_chains(name):
    a = K.case(name).arrays
    sizes = np.diff(a["tree_offset"])
    assert (sizes == 1).any() and (sizes == 3).any()
    chains = np.flatnonzero(sizes == 601)
    assert len(chains) == 2
    kinds = set()
    for t in chains:
        o = int(a["tree_offset"][t])
        left, right = a["left"][o:o + 601], a["right"][o:o + 601]
        inner = np.flatnonzero(left >= 0)
        assert len(inner) == 300
        if (left[right[inner]] < 0).all():
            kinds.add("left")  # every right child is a leaf
        if (left[left[inner]] < 0).all():
            kinds.add("right")
    assert kinds == {"left", "right"}
    # and the query rows leave the chains at many depths, the deepest leaf included
    L = ref.leaf_table(a, scaled(name)[0])
    for t in chains:
        depth = np.unique(L[t])
        o = int(a["tree_offset"][t])
        deepest = o + (300 if a["left"][o + 1] >= 0 else 600)  # pre-order: a left chain's last leaf follows its last split
        assert len(depth) >= 10 and deepest in depth, (name, t, len(depth))


@pytest.mark.parametrize("name", [n for n in TABLE if K.kind_of(n) == "rf" and not n.endswith("subnormal")])
def test_rf_fractions_sum_to_one(name):
    a = K.case(name).arrays
    leaf = a["left"] < 0
    assert (a["value"][leaf] >= 0).all()
    np.testing.assert_allclose(a["value"][leaf].sum(axis=1), 1.0, rtol=0, atol=4e-16)


@pytest.mark.parametrize("name", [n for n in TABLE if K.kind_of(n) == "gb" and not n.endswith("subnormal")])
def test_gb_raw_stays_within_eight(name):
    a = K.case(name).arrays
    assert float(a["learning_rate"]) == 0.1
    raw = ref.gb_raw_from_leaves(a, ref.leaf_table(a, scaled(name)[0]))
    print(f"{name}: max |raw| {np.abs(raw).max():.3f}")
    assert np.abs(raw).max() <= 8


@pytest.mark.parametrize("name", SVCS)
def test_svc_models_are_platt_shaped_and_their_kernel_values_alive(name):
    a = K.case(name).arrays
    assert (a["prob_a"] < 0).all() and np.abs(a["intercept"]).max() < 2 and np.abs(a["dual_coef"]).max() <= 1
    assert 0.4 <= float(a["gamma"]) <= 1.0 and 3 <= a["sv"].shape[1] <= 6
    k = ref.svc_kernel_seq(a, scaled(name)[0])
    assert (k.max(axis=1) > 0.2).mean() > 0.9  # the rows sit near support vectors


def test_svc_class_ranges_cross_the_chunks_as_claimed():
    start = lambda n: np.concatenate([[0], np.cumsum(K.case(n).arrays["n_support"])])  # noqa: E731
    s = start("svc_straddle")
    assert 0 < s[1] < K.CHUNK < s[2] < 2 * K.CHUNK  # class 1 starts strictly inside the first chunk and ends inside the second
    s = start("svc_three_chunks")
    assert s[2] - s[1] > 2 * K.CHUNK and s[1] < K.CHUNK and s[2] > 2 * K.CHUNK
    assert K.case("svc_empty_class").arrays["n_support"][1] == 0
    assert K.case("svc_S5").arrays["n_support"].tolist() == [1] * 5
    assert [len(K.case(f"svc_S{S}").arrays["sv"]) for S in (1023, 1024, 1025, 2049)] == [1023, 1024, 1025, 2049]
    assert [len(K.case(f"svc_C{C}").arrays["n_support"]) for C in (23, 24, 25, 32)] == [23, 24, 25, 32]
    assert 2300 <= len(K.case("svc_C32").arrays["sv"]) <= 2500


# ------------------------------------------------------------------ coverage counts
@pytest.mark.parametrize("name", TABLE)
def test_each_model_reaches_the_path_it_is_there_for(name):
    c = K.case(name)
    n = K.counts(c)
    print(name, n)
    for path in c.paths:
        assert n[path] > 0, (name, path)
    a = c.arrays
    if c.kind != "svc":
        assert ("feat256" in c.paths) == (a["mean"].size > K.THREADS) and ("tree256" in c.paths) == (n_trees(a) > K.THREADS)
    else:
        C = len(a["n_support"])
        assert ("pair256" in c.paths) == (C * (C - 1) // 2 > K.THREADS) and ("sv1024" in c.paths) == (len(a["sv"]) > K.CHUNK)
    if "feat256" in c.paths:  # and the rows walk through such nodes: reading those features as 0 moves leaves
        Xs, _ = scaled(name)
        Z = Xs.copy()
        Z[:, K.THREADS:] = 0.0
        assert (ref.leaf_table(a, Z) != ref.leaf_table(a, Xs)).any(axis=0).sum() >= len(Xs) // 2


def test_the_table_holds_every_size_the_issue_lists():
    sizes = {(K.case(n).kind, n_trees(K.case(n).arrays), K.case(n).arrays["mean"].size, K.case(n).arrays["classes"].size)
             for n in TREES}
    for T in (1, 255, 256, 257, 513):
        assert ("rf", T, 79, 5) in sizes
    for F in (1, 255, 256, 257, 1024):
        assert ("rf", 200, F, 5) in sizes
    assert ("rf", 4096, 1024, 32) in sizes
    assert {("gb", 300, 257, 2), ("gb", 300, 79, 3), ("gb", 1280, 257, 32)} <= sizes
    assert [C * (C - 1) // 2 for C in (23, 24, 25, 32)] == [253, 276, 300, 496]


# ------------------------------------------------------------------ rows
@pytest.mark.parametrize("name", [n for n in TABLE if not n.endswith("subnormal")])
def test_row_batches_and_nan_rows(name):
    c = K.case(name)
    a, X = c.arrays, c.X
    F = a["mean"].size
    assert X.shape == (K.ROWS, F) and K.SLICE.start <= K.NAN_ROW < K.SLICE.stop
    nan = np.isnan(X)
    if c.kind != "rf":
        assert nan.sum() == 1 and nan[K.NAN_ROW, F - 1]
        return
    rows = np.flatnonzero(nan.any(axis=1))
    assert rows.tolist() == list(range(K.NAN_ROW, K.NAN_ROW + 6))
    cols = np.flatnonzero(nan.any(axis=0))
    assert (cols < K.THREADS).any() and ((cols >= K.THREADS).any() or F <= K.THREADS)
    # the NaN is met on the way down: sending it the other way moves a leaf of every such row
    flipped = dict(a, missing_left=(1 - a["missing_left"]).astype(np.uint8))
    Xs = ref.scale(a, X)
    assert (ref.leaf_table(flipped, Xs[rows]) != ref.leaf_table(a, Xs[rows])).any(axis=0).all()


def walk(a, Xs, lt=False, nan_right=False, ftz=False, f64=False):
    """``ref.leaf_table`` with one rule changed: ``<`` for ``<=``, NaN always right, float32 subnormals flushed to zero
    before the comparison, or the comparison made on the float64 value (no cast)."""
    X = Xs if f64 else Xs.astype(np.float32)
    if ftz:
        X = np.where(np.abs(X) < np.float32(2.0 ** -126), np.float32(0), X)
    out = []
    for t in range(n_trees(a)):
        o0 = int(a["tree_offset"][t])
        left, right = a["left"][o0:], a["right"][o0:]
        feat, thr, miss = a["feature"][o0:], a["threshold"][o0:], a["missing_left"][o0:]
        node = np.zeros(len(X), np.int64)
        live = left[node] >= 0
        while live.any():
            n = node[live]
            x = X[np.flatnonzero(live), feat[n]].astype(np.float64)
            cmp = (x < thr[n]) if lt else (x <= thr[n])
            go_left = np.where(np.isnan(x), (miss[n] != 0) & (not nan_right), cmp)
            node[live] = np.where(go_left, left[n], right[n])
            live = left[node] >= 0
        out.append(o0 + node)
    return np.stack(out)


def test_walk_without_a_change_is_the_reference_walk():
    for name in ("rf_F257", "gb_subnormal"):
        a, (Xs, _) = K.case(name).arrays, scaled(name)
        assert np.array_equal(walk(a, Xs), ref.leaf_table(a, Xs))


@pytest.mark.parametrize("name", [n for n in TREES if n != "rf_F1" and not n.endswith("subnormal")])
def test_planted_rows_sit_where_the_cast_decides(name):
    """Four rows with float32(v) == thr < v (the cast goes left where float64 would go right) and four with
    v == thr < float32(v), each on a node one below a root, in trees taken from the end of the forest."""
    c = K.case(name)
    a = c.arrays
    assert len(c.edge_rows) >= (8 if n_trees(a) >= 64 else 1), (name, c.edge_rows)
    Xs = ref.scale(a, c.X)[list(c.edge_rows)]
    cast, exact = walk(a, Xs), walk(a, Xs, f64=True)
    moved = (cast != exact)
    assert moved.any(axis=0).all(), name  # every planted row takes another leaf under the float64 comparison
    trees = np.flatnonzero(moved.any(axis=1))
    if n_trees(a) > K.THREADS:  # trees of the second trip, as far as there are eight of them
        assert (trees >= K.THREADS).all() if n_trees(a) >= K.THREADS + 64 else (trees >= K.THREADS).any()
    # both directions occur: the first four rows go left under the cast, the others right
    for k, r in enumerate(c.edge_rows):
        t = np.flatnonzero(moved[:, k])[0]
        o = int(a["tree_offset"][t])
        child = a["left"][o] if a["left"][o + a["left"][o]] >= 0 else a["right"][o]
        node = o + int(child)
        v = Xs[k, a["feature"][node]]
        thr = a["threshold"][node]
        if k < 4:
            assert float(np.float32(v)) == thr < v
        else:
            assert v == thr < float(np.float32(v))


@pytest.mark.parametrize("name", ["rf_subnormal", "gb_subnormal"])
def test_subnormal_rows_and_thresholds(name):
    c = K.case(name)
    a = c.arrays
    assert (a["mean"] == 0).all() and (a["scale"] == 1).all()
    tiny = float(np.finfo(np.float32).tiny)
    assert np.abs(c.X).max() < tiny and (c.X != 0).mean() > 0.9
    thr = a["threshold"][a["left"] >= 0] / K.SUB
    assert (np.abs(thr) < 2 ** 23).all() and (thr - np.floor(thr) == 0.5).all()  # midpoints of two subnormals
    # the cast itself decides rows: quarter steps round to the nearest subnormal
    assert (walk(a, c.X) != walk(a, c.X, f64=True)).any(axis=0).sum() >= 3


# ------------------------------------------------------------------ labels and margins
@pytest.mark.parametrize("name", TABLE)
def test_labels_spread_and_the_winner_is_clear(name):
    c = K.case(name)
    a = c.arrays
    labels, proba = K.reference(name)
    Xs, bad = scaled(name)
    C = len(a["classes"])
    assert len(set(labels[~bad].tolist())) >= min(C, 4), (name, np.unique(labels))
    if c.kind == "rf":
        s = np.sort(proba, axis=1)
        gap = (s[:, -1] - s[:, -2]).min()
        print(f"{name}: smallest top-two gap {gap:.4g} = {gap * n_trees(a):.3g} / T")
        assert gap >= 1.0 / n_trees(a)
    elif c.kind == "gb":
        raw = ref.gb_raw_from_leaves(a, ref.leaf_table(a, Xs))[~bad]
        s = np.sort(raw, axis=1)
        gap = np.abs(raw).min() if raw.shape[1] == 1 else (s[:, -1] - s[:, -2]).min()
        print(f"{name}: smallest raw gap {gap:.4g}")
        assert gap >= 1e-6
    else:
        dec = ref.svc_decision_seq(a, Xs)[~bad]
        votes = svc_votes(dec, C)
        s = np.sort(votes, axis=1)
        print(f"{name}: smallest |dec| {np.abs(dec).min():.4g}, smallest vote lead {(s[:, -1] - s[:, -2]).min()}")
        assert np.abs(dec).min() >= 1e-6 and (s[:, -1] > s[:, -2]).all()


@pytest.mark.parametrize("name", EXACT)
def test_exact_cases_give_what_they_are_built_for(name):
    c = K.case(name)
    assert len(c.X) >= 3
    for labels, proba in (K.reference(name), ref.predict(c.arrays, c.X)):
        assert (labels == c.note["label"]).all(), name
        if "proba" in c.note:
            assert (proba == np.asarray(c.note["proba"])).all(), name
    a = c.arrays
    if name == "exact_rf_tie":
        proba = K.reference(name)[1]
        assert (proba[:, 1] == proba[:, 2]).all() and (proba[:, 0] < proba[:, 1]).all() and len(np.unique(proba[:, 1])) >= 3
        assert n_trees(a) == 4 and (np.modf(a["value"] * 8)[0] == 0).all()
    if name == "exact_gb_tie":
        raw = ref.gb_raw(a, ref.scale(a, c.X))
        assert (raw[:, 1] == raw[:, 2]).all() and len(np.unique(raw[:, 1])) >= 3
    if name == "exact_gb_zero":
        assert (ref.gb_raw(a, ref.scale(a, c.X)) == 0).all() and float(a["learning_rate"]) == 0.5
    if name.startswith("exact_svc"):
        for dec in (ref.svc_decision(a, ref.scale(a, c.X)), ref.svc_decision_seq(a, ref.scale(a, c.X))):
            assert (dec == a["intercept"]).all()  # bit for bit
        votes = svc_votes(dec, len(a["n_support"]))
        assert (votes == (np.arange(6) if name == "exact_svc_zero" else [1, 1, 1])).all()


def svc_votes(dec, C, ge=False):
    votes = np.zeros((len(dec), C), np.int64)
    p = 0
    for i in range(C):
        for j in range(i + 1, C):
            win = (dec[:, p] >= 0) if ge else (dec[:, p] > 0)
            votes[win, i] += 1
            votes[~win, j] += 1
            p += 1
    return votes


# ------------------------------------------------------------------ SVC iteration conditions
@pytest.mark.parametrize("name", SVCS)
def test_no_stopping_check_is_decided_by_a_last_bit(name):
    """In no check of multiclass_probability does max_error lie within 1e-9 of 0.005 / k (a last-bit difference in the
    decision values could otherwise change the iteration count and move proba by 1e-4); the models with C >= 23 have rows
    that take three or more iterations."""
    a = K.case(name).arrays
    Xs, bad = scaled(name)
    C = len(a["n_support"])
    r = ref.pairwise_r(a, ref.svc_decision_seq(a, Xs[~bad]))
    _, iters, errors = ref.multiclass_probability_rows(r)
    near = min(np.nanmin(np.abs(e - 0.005 / C)) for e in errors)
    print(f"{name}: iterations {np.bincount(iters).tolist()}, nearest max_error to the bound {near:.3g}")
    assert near >= 1e-9
    assert iters.max() < max(100, C)
    if C >= 23:
        assert (iters >= 3).any()
    assert ((r > 1e-7) & (r < 1 - 1e-7)).sum(axis=(1, 2)).min() > 0  # not every pair sits on the clamp


def test_search_for_a_row_that_runs_to_max_iter():
    """No row of the table runs to max_iter (its largest count is 6 of 100, at C = 32), and this seeded search over 7200
    pairwise matrices (k = 3 ... 32; entries on the clamp in random tournaments, uniform, and mixed) finds none either: the
    largest count it meets is 4.  So the max_iter exit of the kernel's loop is not covered by a device test."""
    rng = np.random.default_rng(0)
    most = 0
    for k in (3, 4, 5, 8, 24, 32):
        for mode in range(3):
            B = 400
            r = np.zeros((B, k, k))
            for i in range(k):
                for j in range(i + 1, k):
                    clamp = np.where(rng.random(B) < 0.5, 1e-7, 1 - 1e-7)
                    free = rng.uniform(1e-7, 1 - 1e-7, B)
                    v = clamp if mode == 0 else free if mode == 1 else np.where(rng.random(B) < 0.7, clamp, free)
                    r[:, i, j], r[:, j, i] = v, 1 - v
            _, iters, _ = ref.multiclass_probability_rows(r)
            most = max(most, int(iters.max()))
    print(f"largest iteration count met: {most}")
    assert most < 100


def test_rows_version_of_multiclass_probability_is_the_per_row_one():
    for name in ("svc_S5", "svc_C23"):
        a = K.case(name).arrays
        Xs, bad = scaled(name)
        r = ref.pairwise_r(a, ref.svc_decision_seq(a, Xs[~bad][:24]))
        p = ref.multiclass_probability_rows(r)[0]
        for b in range(len(r)):
            assert np.array_equal(p[b], ref.multiclass_probability(r[b])), (name, b)


# ------------------------------------------------------------------ the two statements of the reference, and scikit-learn
@pytest.mark.parametrize("name", K.NAMES)
def test_both_statements_of_the_reference_agree(name):
    """``predict`` (np.sum, @, einsum) against ``predict_seq`` (the header's orders), within a tenth of the header's bounds:
    RF bit for bit, GB proba 1e-16, SVC decision values 1e-13 and proba 1e-10, on every row.  Measured: GB 8.3e-17 at K = 32
    and 0 elsewhere, decision values at most 1.9e-14, SVC proba at most 3.8e-15."""
    c = K.case(name)
    a = c.arrays
    rows = np.arange(len(c.X))
    l_seq, p_seq = K.reference(name)
    l_old, p_old = ref.predict(a, c.X[rows])
    assert np.array_equal(l_old, l_seq[rows])
    assert np.array_equal(np.isnan(p_old), np.isnan(p_seq[rows]))
    dist = np.nanmax(np.abs(p_old - p_seq[rows]))
    print(f"{name}: proba distance between the statements {dist:.3g}")
    if c.kind == "rf":
        assert np.array_equal(p_old.view(np.uint64), p_seq[rows].view(np.uint64))
    elif c.kind == "gb":
        assert dist <= 1e-16
    else:
        Xs, bad = scaled(name)
        d = np.abs(ref.svc_decision(a, Xs[rows]) - ref.svc_decision_seq(a, Xs[rows])).max()
        print(f"{name}: decision value distance {d:.3g}")
        assert d <= 1e-13 and dist <= 1e-10


@pytest.fixture(scope="module")
def sk_rows():
    rng = np.random.default_rng(77)
    C, F, n = 25, 12, 1500
    y = np.arange(n) % C
    centres = rng.normal(0, 2.0, (C, F))
    X = centres[y] + rng.normal(0, 1.0, (n, F))
    Q = centres[y[:200]] + rng.normal(0, 1.2, (200, F))
    return X * 3.0 + 1.0, y, Q * 3.0 + 1.0


@pytest.mark.parametrize("kind", ["svc", "rf", "gb"])
def test_restatements_against_live_sklearn_at_larger_sizes(sk_rows, kind):
    """A 25-class SVC (P = 300 pairs), a 300-tree forest and a multiclass GB, fitted here: both statements of the reference
    against scikit-learn with the bounds of tests/test_classifier_ref.py (labels equal, RF bit for bit, GB 1e-15, SVC
    1e-9)."""
    pytest.importorskip("sklearn")
    from sklearn.ensemble import GradientBoostingClassifier, RandomForestClassifier
    from sklearn.preprocessing import StandardScaler
    from sklearn.svm import SVC

    from underwater_image_enhancement_amd.classifier import export_sklearn

    X, y, Q = sk_rows
    if kind == "gb":
        keep = y < 6
        X, y = X[keep][:240], y[keep][:240]
    sc = StandardScaler().fit(X)
    model = {"svc": SVC(kernel="rbf", probability=True, random_state=0),
             "rf": RandomForestClassifier(n_estimators=300, max_depth=8, random_state=0),
             "gb": GradientBoostingClassifier(n_estimators=20, max_depth=3, random_state=0)}[kind].fit(sc.transform(X), y)
    a = export_sklearn(model, sc)
    assert model_check(a) == 0
    Qs = sc.transform(Q)
    want_l, want_p = np.searchsorted(model.classes_, model.predict(Qs)), model.predict_proba(Qs)
    if kind == "svc":
        assert len(a["n_support"]) == 25 and a["intercept"].size == 300
    if kind == "rf":
        assert n_trees(a) == 300
    for fn in (ref.predict_seq, ref.predict):
        labels, proba = fn(a, Q)
        dist = np.abs(proba - want_p).max()
        print(f"{kind} {fn.__name__}: proba distance to scikit-learn {dist:.3g}")
        assert np.array_equal(labels, want_l)
        if kind == "rf":
            assert np.array_equal(proba, want_p)
        else:
            assert dist <= (1e-15 if kind == "gb" else 1e-9)


# ------------------------------------------------------------------ mutations, stated in NumPy
def last_argmax(x, axis=1):
    return x.shape[1] - 1 - np.argmax(x[:, ::-1], axis=axis)


def from_leaves(c, L, bad, argmax=np.argmax, divide_by=None):
    a = c.arrays
    if c.kind == "rf":
        acc = np.zeros((L.shape[1], a["value"].shape[1]))
        for t in range(len(L)):
            acc += a["value"][L[t]]
        proba = acc / (divide_by or len(L))
        return argmax(proba, axis=1), proba
    raw = ref.gb_raw_from_leaves(a, L)
    labels = (raw[:, 0] >= 0).astype(np.int64) if raw.shape[1] == 1 else argmax(raw, axis=1)
    proba = ref.gb_proba_seq(raw)
    proba[bad] = np.nan
    return np.where(bad, -1, labels), proba


def from_dec(c, dec, bad, argmax=np.argmax, ge=False):
    a = c.arrays
    labels = argmax(svc_votes(dec, len(a["n_support"]), ge), axis=1)
    proba = ref.svc_proba_seq(a, dec)
    proba[bad] = np.nan
    return np.where(bad, -1, labels), proba


def m_tree_rule(**rule):
    def run(c, Xs, bad):
        return from_leaves(c, walk(c.arrays, Xs, **rule), bad)
    return run


def m_trees_dropped(c, Xs, bad):
    L = ref.leaf_table(c.arrays, Xs)
    return from_leaves(c, L[:K.THREADS], bad, divide_by=len(L))


def m_leaves_wrapped(c, Xs, bad):
    L = ref.leaf_table(c.arrays, Xs)
    L[K.THREADS:] = L[:len(L) - K.THREADS]
    return from_leaves(c, L, bad)


def m_features_zero(c, Xs, bad):
    Z = Xs.copy()
    Z[:, K.THREADS:] = 0.0
    return from_leaves(c, ref.leaf_table(c.arrays, Z), bad)


def m_last_maximum(c, Xs, bad):
    if c.kind == "svc":
        return from_dec(c, ref.svc_decision_seq(c.arrays, Xs), bad, argmax=last_argmax)
    return from_leaves(c, ref.leaf_table(c.arrays, Xs), bad, argmax=last_argmax)


def m_pairs_left_at_rho(c, Xs, bad):
    dec = ref.svc_decision_seq(c.arrays, Xs)
    dec[:, K.THREADS:] = c.arrays["intercept"][K.THREADS:]
    return from_dec(c, dec, bad)


def m_first_chunk_only(c, Xs, bad):
    k = ref.svc_kernel_seq(c.arrays, Xs)
    k[:, K.CHUNK:] = 0.0
    return from_dec(c, ref.svc_decision_from_kernel(c.arrays, k), bad)


def m_range_not_clipped(c, Xs, bad):
    a = c.arrays
    chunks = -(-len(a["sv"]) // K.CHUNK)
    rho = -a["intercept"]
    total = ref.svc_decision_seq(a, Xs) + rho  # the sum over both classes' vectors, which every chunk adds again
    return from_dec(c, total * chunks - rho, bad)


def m_vote_ge(c, Xs, bad):
    return from_dec(c, ref.svc_decision_seq(c.arrays, Xs), bad, ge=True)


MUTANTS = {  # name: (the mutated restatement, the cases it is run on)
    "trees with index >= 256 dropped": (m_trees_dropped, ["rf_T257", "rf_T513", "rf_T4096_F1024_C32"]),
    "leaves from tree 256 on taken from tree t - 256": (m_leaves_wrapped, ["rf_T257", "rf_T513", "rf_T4096_F1024_C32"]),
    "features >= 256 read as 0": (m_features_zero, ["rf_F257", "rf_F1024", "rf_T4096_F1024_C32", "gb_C2_T300_F257", "gb_C32_T1280_F257"]),
    "pairs >= 256 left at -rho": (m_pairs_left_at_rho, ["svc_C24", "svc_C25", "svc_C32"]),
    "only the first chunk of support vectors summed": (m_first_chunk_only, ["svc_S1025", "svc_S2049", "svc_straddle", "svc_three_chunks", "svc_C32"]),
    "a class's range not clipped to the chunk": (m_range_not_clipped, ["svc_S1025", "svc_straddle", "svc_three_chunks", "svc_C23"]),
    "< for <= at a node": (m_tree_rule(lt=True), ["rf_T513", "rf_F257", "gb_C3_T300", "gb_C32_T1280_F257"]),
    "NaN always right": (m_tree_rule(nan_right=True), ["rf_T256", "rf_F1024", "rf_T4096_F1024_C32"]),
    "subnormals flushed to zero before the comparison": (m_tree_rule(ftz=True), ["rf_subnormal", "gb_subnormal"]),
    "last maximum for first": (m_last_maximum, ["exact_rf_tie", "exact_gb_tie", "exact_svc_cycle"]),
    "dec >= 0 for dec > 0 in the vote": (m_vote_ge, ["exact_svc_zero"]),
}


@pytest.mark.parametrize("mutant", list(MUTANTS))
def test_mutant_is_caught_on_every_case_it_is_aimed_at(mutant):
    """On each of its cases the mutated restatement differs from the true one by a changed label or by >= 1000 x the bound
    (RF: by any bit) on at least three rows; so a device that made this mistake fails tests/test_gpu_classifier_limits.py."""
    fn, names = MUTANTS[mutant]
    for name in names:
        c = K.case(name)
        Xs, bad = scaled(name)
        if c.kind == "rf":
            Xs = ref.scale(c.arrays, c.X)
        labels, proba = fn(c, Xs.copy(), bad)
        want_l, want_p = K.reference(name)
        with np.errstate(invalid="ignore"):
            off = np.abs(proba - want_p).max(axis=1)
        off = np.where(np.isnan(off), 0.0, off)
        caught = (labels != want_l) | (off > 0 if c.kind == "rf" else off >= 1000 * BOUND[c.kind])
        print(f"{mutant} on {name}: {int(caught.sum())} rows of {len(caught)} ({int((labels != want_l).sum())} labels)")
        assert caught.sum() >= 3, (mutant, name)


def test_the_true_restatement_run_through_the_mutation_harness_is_unchanged():
    for name, fn in (("rf_T257", m_tree_rule()), ("gb_C3_T300", m_tree_rule()), ("svc_S1025", lambda c, Xs, bad: from_dec(
            c, ref.svc_decision_seq(c.arrays, Xs), bad))):
        c = K.case(name)
        Xs, bad = scaled(name)
        Xs = ref.scale(c.arrays, c.X) if c.kind == "rf" else Xs
        labels, proba = fn(c, Xs, bad)
        want_l, want_p = K.reference(name)
        assert np.array_equal(labels, want_l) and np.array_equal(proba, want_p, equal_nan=True)
