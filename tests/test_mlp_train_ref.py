"""tests/mlp_train_ref.py (the restatement of EndToEndTrainer's step the GPU tests lean on) against the real trainer's records
in tests/golden/mlp_train.npz, and the measured differences the device tolerances are made of."""
import numpy as np
import pytest

import gated_predictor_ref as R
import mlp_train_ref as T

A_STEPS, B_STEPS = 4, 2


@pytest.fixture(scope="module")
def gold():
    return T.load_golden()


@pytest.fixture(scope="module")
def state0():
    return R.small_state(R.load_golden())


def batch(gold, i):
    return gold[f"batch/{i}/u8"].astype(np.float32) / np.float32(255.0), gold[f"batch/{i}/reference"], gold[f"batch/{i}/features"]


def with_grad(state):
    return [k for k in state if k not in T.FREE]


def snapshot(gold, tag, state0):
    """(params, exp_avg, exp_avg_sq) of a golden snapshot; the gradient-free heads' moments are zeros"""
    p = {k: gold[f"{tag}/param/{k}"].copy() for k in state0}
    m = {k: gold[f"{tag}/exp_avg/{k}"].copy() if k not in T.FREE else np.zeros_like(state0[k]) for k in state0}
    v = {k: gold[f"{tag}/exp_avg_sq/{k}"].copy() if k not in T.FREE else np.zeros_like(state0[k]) for k in state0}
    return p, m, v


def zeros_like(state):
    return {k: np.zeros_like(v) for k, v in state.items()}


def test_the_fixture_is_what_it_is_for(gold, state0):
    assert tuple(gold["dims"]) == (79, 64, 1) and [k for k, _ in R.layout(79, 64, 1)] == list(state0)
    n = 16 * 20
    for tag in [f"a/{s}" for s in range(A_STEPS)] + [f"b/{s}" for s in range(B_STEPS)]:
        assert gold[f"{tag}/masks"].shape == (3, 4, 64) and set(np.unique(gold[f"{tag}/masks"])) <= {0, 1}
        for k in ("L_low", "L_high"):
            pos = gold[f"{tag}/{k}"].astype(np.float64) / 100.0 * n
            assert np.abs(pos - np.round(pos)).min() >= 1e-3
        zeros = [float((gold[f"{tag}/grad/{k}"] == 0).mean()) for k in with_grad(state0)]
        assert max(zeros) > 0.2  # dead ReLUs and dropped units: many exact zeros
        assert not any(f"{tag}/grad/{k}" in gold for k in T.FREE)
    assert all(float(gold[f"a/{s}/norm"]) < 1.0 for s in range(A_STEPS))
    assert all(float(gold[f"b/{s}/norm"]) > float(gold["b/max_norm"]) for s in range(B_STEPS))
    assert float(gold["a/after1/step"]) == 1.0 and float(gold["a/after4/step"]) == 4.0 and float(gold["b/after2/step"]) == 2.0
    for k in T.FREE:  # no gradient, no update
        assert np.array_equal(gold[f"a/after4/param/{k}"], state0[k]) and f"a/after4/exp_avg/{k}" not in gold


def test_gradients_against_the_real_trainer(gold, state0):
    """Case A's first step and case B's first step start from the stored weights; the later ones from weights the fixture
    holds only after steps 1 and 4, so the restatement's own Adam carries them there (its error is far below the
    gradients')."""
    worst = 0.0
    for case, steps, max_norm in (("a", A_STEPS, 1.0), ("b", B_STEPS, float(gold["b/max_norm"]))):
        p = {k: v.copy() for k, v in state0.items()}
        m, v = zeros_like(p), zeros_like(p)
        for s in range(steps):
            img, ref, feat = batch(gold, s)
            loss, l1, l2, out, g64 = T.step_grads64(p, img, ref, feat, gold[f"{case}/{s}/masks"])
            for k in with_grad(p):
                want = gold[f"{case}/{s}/grad/{k}"]
                assert np.array_equal(want == 0, g64[k] == 0), (case, s, k)
                worst = max(worst, T.grad_error(g64[k], want))
            assert all(not g64[k].any() for k in T.FREE)
            assert abs(T.total_norm64(g64) - float(gold[f"{case}/{s}/norm"])) <= 1e-5 * float(gold[f"{case}/{s}/norm"])
            assert R.worst_fraction(out, {k: gold[f"{case}/{s}/{k}"] for k in R.HEADS}) <= R.REF_F32_ERROR
            T.adam32(p, {k: gold[f"{case}/{s}/grad/{k}"] if k not in T.FREE else g64[k] for k in p}, m, v, s + 1, max_norm)
    print(f"REF_GRAD_ERROR measured {worst:.4g}")
    assert 0.5 * T.REF_GRAD_ERROR <= worst <= T.REF_GRAD_ERROR


def test_adam_against_the_real_trainer(gold, state0):
    worst = 0.0
    for case, steps, max_norm, marks in (("a", A_STEPS, 1.0, {1: "a/after1", 4: "a/after4"}),
                                         ("b", B_STEPS, float(gold["b/max_norm"]), {2: "b/after2"})):
        p = {k: v.copy() for k, v in state0.items()}
        m, v = zeros_like(p), zeros_like(p)
        for s in range(steps):
            grads = {k: gold[f"{case}/{s}/grad/{k}"] if k not in T.FREE else np.zeros_like(p[k]) for k in p}
            norm, coef = T.adam32(p, grads, m, v, s + 1, max_norm)
            assert (coef < 1.0) == (case == "b")
            if s + 1 in marks:
                wp, wm, wv = snapshot(gold, marks[s + 1], state0)
                for k in p:
                    worst = max(worst, T.ulps(p[k], wp[k]), T.ulps(m[k], wm[k]), T.ulps(v[k], wv[k]))
                    if k in T.FREE:
                        assert np.array_equal(p[k], state0[k])
    print(f"REF_ADAM_ERROR measured {worst:.4g} ulp")
    assert 0.5 * T.REF_ADAM_ERROR <= worst <= T.REF_ADAM_ERROR


def test_free_trajectory_against_the_real_trainer(gold, state0):
    p = {k: v.copy() for k, v in state0.items()}
    m, v = zeros_like(p), zeros_like(p)
    worst_loss = 0.0
    for s in range(A_STEPS):
        img, ref, feat = batch(gold, s)
        loss, l1, l2, _, g64 = T.step_grads64(p, img, ref, feat, gold[f"a/{s}/masks"])
        worst_loss = max(worst_loss, abs(loss - float(gold[f"a/{s}/loss"])), abs(l1 - float(gold[f"a/{s}/l1"])),
                         abs(l2 - float(gold[f"a/{s}/l2"])))
        T.adam32(p, g64, m, v, s + 1, 1.0)
    wp, _, _ = snapshot(gold, "a/after4", state0)
    worst_param = max(float(np.abs(p[k].astype(np.float64) - wp[k]).max()) for k in p)
    print(f"REF_TRAJ_ERROR measured ({worst_param:.4g}, {worst_loss:.4g})")
    assert 0.5 * T.REF_TRAJ_ERROR[0] <= worst_param <= T.REF_TRAJ_ERROR[0]
    assert 0.5 * T.REF_TRAJ_ERROR[1] <= worst_loss <= T.REF_TRAJ_ERROR[1]
