"""csrc/k_classify.hip at the sizes uwie_model_check admits (tests/classifier_cases.py; what each case is for is proven on the
CPU in tests/test_classifier_cases.py): every model goes through classifier.model_desc -> uwie_model_create ->
uwie_classify_f64 -> uwie_model_destroy and is held to the sequential-order NumPy statement of include/uwie.h
(classifier_ref.predict_seq) with the header's own bounds: labels equal, RF proba bit for bit, GB proba 1e-15, SVC proba 1e-9,
the exact cases equal."""
import ctypes

import numpy as np
import pytest
import torch

import classifier_cases as K
import classifier_ref as ref
import underwater_image_enhancement_amd as uw
from underwater_image_enhancement_amd.classifier import model_desc

pytestmark = pytest.mark.gpu

NAN_BIT = uw._lib.STATUS_CLASSIFY_NAN
TABLE = [n for n in K.NAMES if not n.startswith("exact_")]
EXACT = [n for n in K.NAMES if n.startswith("exact_")]


class Models:
    """One upload per model for the whole module, counted."""

    def __init__(self, dev):
        self.dev, self.handles, self.uploads = dev, {}, {}

    def handle(self, name):
        if name not in self.handles:
            m, _keep = model_desc(K.case(name).arrays)
            h = ctypes.c_void_p()
            uw._lib.check(self.dev.lib.uwie_model_create(self.dev._ctx, ctypes.byref(m), ctypes.byref(h)))
            self.handles[name] = h
            self.uploads[name] = self.uploads.get(name, 0) + 1
        return self.handles[name]

    def classify(self, name, X):
        """(labels, proba, status bits) of uwie_classify_f64 on host rows ``X``."""
        dev = self.dev
        X = np.array(X, np.float64, order="C").reshape(-1, K.case(name).arrays["mean"].size)  # a copy: the table is read-only
        t = torch.from_numpy(X).to(dev.torch_device)
        label = dev.empty((len(X),), torch.int32)
        proba = dev.empty((len(X), len(K.case(name).arrays["classes"])), torch.float64)
        uw._lib.check(dev.lib.uwie_classify_f64(dev._ctx, self.handle(name), ctypes.c_void_p(t.data_ptr()), len(X), X.shape[1],
                                                ctypes.c_void_p(label.data_ptr()), ctypes.c_void_p(proba.data_ptr()), dev.stream()))
        lh, ph = label.cpu().numpy(), proba.cpu().numpy()
        return lh, ph, dev.check_status(allow=NAN_BIT)


@pytest.fixture(scope="module")
def models():
    dev = uw.get_device()
    ms = Models(dev)
    yield ms
    torch.cuda.synchronize(dev.index)
    for h in ms.handles.values():
        dev.lib.uwie_model_destroy(h)
    assert dev.check_status() == 0
    assert ms.uploads and all(n == 1 for n in ms.uploads.values()), ms.uploads  # no model was uploaded twice


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.mark.parametrize("name", TABLE)
def test_table_model_against_the_sequential_statement(models, name):
    c = K.case(name)
    want_l, want_p = K.reference(name)
    labels, proba, status = models.classify(name, c.X)
    bad = want_l < 0
    wrong = np.flatnonzero(labels != want_l)
    assert wrong.size == 0, (name, wrong[:8], labels[wrong[:8]], want_l[wrong[:8]])
    with np.errstate(invalid="ignore"):
        dist = np.nanmax(np.abs(proba - want_p))
    print(f"{name}: {len(c.X)} rows, max |proba - reference| {dist:.3g}, {int((bits(proba) != bits(want_p)).any(axis=1).sum())} "
          f"rows differ in a bit")
    if c.kind == "rf":
        assert not bad.any() and status == 0
        assert np.array_equal(bits(proba), bits(want_p))  # NaN rows (routed by missing_left) and planted rows included
        return
    # GB / SVC: a NaN row gets -1, NaN proba and the status bit, and leaves its neighbours untouched
    assert status == (NAN_BIT if bad.any() else 0)
    assert np.isnan(proba[bad]).all() and not np.isnan(proba[~bad]).any()
    assert dist <= (1e-15 if c.kind == "gb" else 1e-9), (name, dist)


@pytest.mark.parametrize("name", EXACT)
def test_exact_case_is_equal(models, name):
    c = K.case(name)
    want_l, want_p = K.reference(name)
    labels, proba, status = models.classify(name, c.X)
    assert status == 0
    assert (labels == c.note["label"]).all() and np.array_equal(labels, want_l)
    if "proba" in c.note:
        assert np.array_equal(bits(proba), bits(np.tile(c.note["proba"], (len(c.X), 1))))
    assert np.array_equal(bits(proba), bits(want_p))


@pytest.mark.parametrize("kind", ["rf", "gb", "svc"])
def test_nan_row_at_32_classes_leaves_its_neighbours_untouched(models, kind):
    """The slice around NAN_ROW alone, and with the NaN taken out: every other row keeps its bits."""
    name = K.LARGE[kind]
    c = K.case(name)
    assert len(c.arrays["classes"]) == 32
    X = c.X[K.SLICE].copy()
    k = K.NAN_ROW - K.SLICE.start
    l_nan, p_nan, s_nan = models.classify(name, X)
    X[np.isnan(X)] = 0.25
    l_ok, p_ok, s_ok = models.classify(name, X)
    assert s_ok == 0 and (l_ok >= 0).all() and not np.isnan(p_ok).any()
    others = np.ones(len(X), bool)
    others[k:k + (6 if kind == "rf" else 1)] = False
    assert np.array_equal(l_nan[others], l_ok[others]) and np.array_equal(bits(p_nan[others]), bits(p_ok[others]))
    if kind == "rf":
        assert s_nan == 0 and (l_nan >= 0).all() and not np.isnan(p_nan).any()
    else:
        assert s_nan == NAN_BIT and l_nan[k] == -1 and np.isnan(p_nan[k]).all()
        assert (l_nan[others] >= 0).all() and not np.isnan(p_nan[others]).any()


@pytest.mark.parametrize("kind", ["rf", "gb", "svc"])
def test_same_bits_in_every_batch_and_run(models, kind):
    """The 300-row batch, its 37-row slice, single rows, and a second run."""
    name = K.LARGE[kind]
    X = K.case(name).X
    l300, p300, _ = models.classify(name, X)
    again = models.classify(name, X)
    assert np.array_equal(again[0], l300) and np.array_equal(bits(again[1]), bits(p300))
    l37, p37, _ = models.classify(name, X[K.SLICE])
    assert np.array_equal(l37, l300[K.SLICE]) and np.array_equal(bits(p37), bits(p300[K.SLICE]))
    for i in (0, K.SLICE.start + 5, K.NAN_ROW, K.EDGE_ROW, len(X) - 1):
        l1, p1, _ = models.classify(name, X[i])
        assert l1[0] == l300[i] and np.array_equal(bits(p1[0]), bits(p300[i])), i


def test_reference_is_the_sequential_statement():
    """The shared reference is ``predict_seq`` and was left as computed."""
    for name in ("rf_T257", "gb_C3_T300", "svc_S1025"):
        c = K.case(name)
        want_l, want_p = K.reference(name)
        assert not want_p.flags.writeable
        l, p = ref.predict_seq(c.arrays, c.X)
        assert np.array_equal(l, want_l) and np.array_equal(p, want_p, equal_nan=True)
