"""tests/gated_predictor_ref.py (the float64 evaluation of ParameterPredictor the GPU tests lean on) against the real module's
outputs in tests/golden/gated_predictor.npz, and the measured float32-against-float64 difference the device tolerance is
made of."""
import numpy as np

import gated_predictor_ref as R


def test_the_seeded_state_is_the_generators():
    g = R.load_golden()
    assert tuple(g["dims"]) == (79, 256, 3)
    state = R.seeded_state(int(g["seed"]))
    assert [k for k in state] == [k for k, _ in R.layout()] and R.checksum(state) == float(g["checksum"])
    small = R.small_state(g)
    assert small["input_proj.0.weight"].shape == (64, 79) and "res_blocks.1.block.0.weight" not in small


def test_float64_evaluation_against_the_real_module():
    g = R.load_golden()
    state = R.seeded_state(int(g["seed"]))
    worst = {}
    for tag in ("unit", "large", "one"):
        want = {k: g[f"{tag}/{k}"] for k in R.HEADS}
        assert all(v.shape == (g[f"{tag}/rows"].shape[0], 1) and v.dtype == np.float32 for v in want.values())
        worst[tag] = R.worst_fraction(R.forward64(state, g[f"{tag}/rows"]), want)
    worst["small"] = R.worst_fraction(R.forward64(R.small_state(g), g["small/rows"]), {k: g[f"small/{k}"] for k in R.HEADS})
    print({k: f"{v:.3g}" for k, v in worst.items()})
    # the recorded measurement holds, and is not slack: the device tolerance is REF_F32_ERROR * DEVICE_MARGIN
    assert 0.9 * R.REF_F32_ERROR <= max(worst.values()) <= R.REF_F32_ERROR
    assert g["one/rows"].shape == (1, 79)


def test_the_cases_are_what_they_are_for():
    g = R.load_golden()
    assert np.abs(g["unit/rows"]).mean() < 1.0 < 20.0 < np.abs(g["large/rows"]).mean()
    # saturated sigmoids at both ends among the large rows, none among the unit rows
    lo, hi = g["large/use_gamma"].min(), g["large/L_low"].max()
    assert lo == 0.0 and hi == 20.0
    assert 0.0 < g["unit/use_gamma"].min() and g["unit/L_low"].max() < 20.0
    # the heads' ranges (deep_learning_parameters.py:158-161)
    for tag in ("unit", "large", "one", "small"):
        assert np.all((g[f"{tag}/gamma"] >= 1.0) & (g[f"{tag}/gamma"] <= 1.5))
        assert np.all((g[f"{tag}/L_low"] >= 5.0) & (g[f"{tag}/L_low"] <= 20.0))
        assert np.all((g[f"{tag}/L_high"] >= 85.0) & (g[f"{tag}/L_high"] <= 98.0))
        assert np.all((g[f"{tag}/use_gamma"] >= 0.0) & (g[f"{tag}/use_gamma"] <= 1.0))
    # validate's average is the mean of its two batches
    assert abs((float(g["validate/0/loss"]) + float(g["validate/1/loss"])) / 2 - float(g["validate/loss"])) < 1e-12
    assert g["validate/0/image"].shape == (2, 3, 16, 20)
