"""deep_learning_parameters.ParameterPredictor (:114-163) for the tests: its state-dict layout, a seeded state, and a float64
NumPy evaluation of the eval-mode forward.

Written from the contract, not from the reference's code.  Pinned against the real module by
tests/test_gated_predictor_ref.py (tests/golden/gated_predictor.npz); the GPU tests use it for batches no fixture holds.
"""
from __future__ import annotations

import numpy as np

HEADS = ("gamma", "L_low", "L_high", "use_gamma")            # param_heads order, the keys of the module's result
GATED_ORDER = ("L_low", "L_high", "use_gamma", "gamma")      # the device's columns (GatedDifferentiableEnhancement.KEYS)
RANGES = {"gamma": (0.5, 1.0), "L_low": (15.0, 5.0), "L_high": (13.0, 85.0), "use_gamma": (1.0, 0.0)}  # sigmoid * a + b
SPAN = {k: a for k, (a, _) in RANGES.items()}
# The largest difference between the real module (torch CPU, float32) and forward64 over the goldens, as a fraction of the
# head's range: measured 1.77e-6 (an L_high near 87 among the magnitude-30 rows; 3.3e-7 for rows of magnitude 1), asserted by
# tests/test_gated_predictor_ref.py.  The device sums each neuron's float32 products in another fixed order than torch's
# GEMM, so it may be as far from float64 on the other side: twice this, and twice again for rows other than the measured
# ones.  DEVICE_TOL is what the GPU tests allow between the device and forward64 or the goldens.
REF_F32_ERROR = 1.8e-6
DEVICE_MARGIN = 4.0
DEVICE_TOL = REF_F32_ERROR * DEVICE_MARGIN


def load_golden():
    import os

    with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gated_predictor.npz"), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def small_state(gold):
    """the stored (79, 64, 1) network, in state_dict() order"""
    return {k: gold["small/state/" + k] for k, _ in layout(79, 64, 1)}


def layout(feature_dim=79, hidden_dim=256, num_blocks=3):
    """(key, shape) in state_dict() order."""
    h = hidden_dim
    out = [("input_proj.0.weight", (h, feature_dim)), ("input_proj.0.bias", (h,))]
    for i in range(num_blocks):
        out += [(f"res_blocks.{i}.block.0.weight", (h, h)), (f"res_blocks.{i}.block.0.bias", (h,)),
                (f"res_blocks.{i}.block.3.weight", (h, h)), (f"res_blocks.{i}.block.3.bias", (h,))]
    out += [("output_proj.0.weight", (h // 2, h)), ("output_proj.0.bias", (h // 2,))]
    for k in HEADS:
        out += [(f"param_heads.{k}.weight", (1, h // 2)), (f"param_heads.{k}.bias", (1,))]
    return out


def seeded_state(seed, feature_dim=79, hidden_dim=256, num_blocks=3):
    """float32 weights from numpy.random.default_rng(seed), drawn in layout order: w ~ N(0, 1 / fan_in), b ~ N(0, 0.1);
    the heads' weights ~ N(0, 4 / fan_in), so that their sigmoids leave the middle of their ranges."""
    rng = np.random.default_rng(seed)
    state = {}
    for key, shape in layout(feature_dim, hidden_dim, num_blocks):
        if key.endswith("weight"):
            v = rng.standard_normal(shape) * np.sqrt((4.0 if key.startswith("param_heads") else 1.0) / shape[1])
        else:
            v = rng.standard_normal(shape) * 0.1
        state[key] = v.astype(np.float32)
    return state


def checksum(state):
    """float64 sum of |w| * (1 + index mod 7) over the tensors in their order: detects a different generator or rule."""
    s = 0.0
    for v in state.values():
        flat = np.abs(np.asarray(v, dtype=np.float64).reshape(-1))
        s += float((flat * (1 + np.arange(flat.size) % 7)).sum())
    return s


def forward64(state, rows):
    """The eval-mode forward in float64 of the float32-rounded ``rows`` [B, F] -> dict of (B, 1) float64 (HEADS' keys)."""
    w = {k: np.asarray(v, dtype=np.float64) for k, v in state.items()}
    x = np.asarray(rows).astype(np.float32).astype(np.float64)
    relu = lambda v: np.maximum(v, 0.0)  # noqa: E731
    x = relu(x @ w["input_proj.0.weight"].T + w["input_proj.0.bias"])
    i = 0
    while f"res_blocks.{i}.block.0.weight" in w:
        p = f"res_blocks.{i}.block."
        t = relu(x @ w[p + "0.weight"].T + w[p + "0.bias"])
        x = relu(t @ w[p + "3.weight"].T + w[p + "3.bias"] + x)
        i += 1
    f = relu(x @ w["output_proj.0.weight"].T + w["output_proj.0.bias"])
    out = {}
    for k in HEADS:
        z = f @ w[f"param_heads.{k}.weight"].T + w[f"param_heads.{k}.bias"]
        a, b = RANGES[k]
        out[k] = 1.0 / (1.0 + np.exp(-z)) * a + b
    return out


def columns(params):
    """dict of (B, 1) -> [B, 4] in the device's order."""
    return np.concatenate([np.asarray(params[k]).reshape(-1, 1) for k in GATED_ORDER], axis=1)


def worst_fraction(got, want):
    """max over heads and rows of |got - want| / the head's range; got, want: dicts of (B, 1)."""
    return max(float(np.abs(np.asarray(got[k], np.float64) - np.asarray(want[k], np.float64)).max()) / SPAN[k] for k in HEADS)
