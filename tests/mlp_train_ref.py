"""EndToEndTrainer.train_epoch's step (deep_learning_parameters.py:265-306) for the tests: the train-mode forward of
ParameterPredictor with given dropout masks and its backward in float64 NumPy, the gated enhancement and ReferenceLoss with
their gradient, clip_grad_norm_, and torch.optim.Adam in float32 with torch's operation order.

Written from the contract, not from the reference's code.  Pinned against the real trainer by
tests/test_mlp_train_ref.py (tests/golden/mlp_train.npz, written by tests/gen_golden_mlp_train.py); the GPU tests use it for
shapes no fixture holds.
"""
from __future__ import annotations

import os

import numpy as np

import gated_predictor_ref as R

P_DROP = 0.3  # every Dropout's rate; torch scales a kept value by float32(1 / (1 - p)) = 1.4285715
LR, BETAS, EPS = 1e-4, (0.9, 0.999), 1e-8
FREE = ("param_heads.L_low.weight", "param_heads.L_low.bias", "param_heads.L_high.weight", "param_heads.L_high.bias")

# Measured by tests/test_mlp_train_ref.py over tests/golden/mlp_train.npz, which asserts each bound and that it is not slack.
# REF_GRAD_ERROR: per tensor max|g_real - g_64| / max|g_real|, the real trainer's float32 autograd against backward64, the
#   largest over the tensors and steps of cases A and B.
# REF_ADAM_ERROR: adam32 fed the golden gradients against the real parameters, exp_avg and exp_avg_sq after one and four
#   steps, per tensor in ulps of its largest magnitude (measured 2.0: exp_avg and exp_avg_sq of case B; the parameters
#   0.5.  Per element the same differences are up to 1182 ulps of an exp_avg that cancelled to near zero.)
# REF_TRAJ_ERROR: the restatement run freely for four steps from the golden masks and inputs: (largest parameter
#   difference, largest difference of loss, l1 or l2), absolute: measured (2.086e-7, 1.967e-8).  REF_GRAD_ERROR measured
#   1.345e-5 (the float32 sums over the pixels behind dL/d(gamma)).
# The device sums in another fixed order than torch, so it may stand as far from float64 on the other side, and the GPU
# tests hold shapes beyond the measured ones: they allow DEVICE_MARGIN times each (the rule of gated_predictor_ref.py).
REF_GRAD_ERROR = 1.4e-5
REF_ADAM_ERROR = 2.0
REF_TRAJ_ERROR = (2.1e-7, 2.0e-8)
DEVICE_MARGIN = 4.0


def load_golden():
    with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mlp_train.npz"), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def sites(num_blocks):
    return 1 + 2 * num_blocks


def blocks_of(state):
    i = 0
    while f"res_blocks.{i}.block.0.weight" in state:
        i += 1
    return i


def forward64(state, rows, masks, p=P_DROP):
    """The train-mode forward in float64.  masks: [sites][B][hidden] of 0 / 1 in call order (input_proj.2, then per block
    block.2 and the outer dropout, which acts on block(x) + x before the ReLU).  Returns (dict of (B, 1) by head, cache)."""
    w = {k: np.asarray(v, dtype=np.float64) for k, v in state.items()}
    scale = 0.0 if p >= 1 else float(np.float32(1.0 / (1.0 - p))) if p > 0 else 1.0
    keep = [np.asarray(m, dtype=np.float64) * scale if p > 0 else np.ones_like(np.asarray(m, dtype=np.float64)) for m in masks]
    x = np.asarray(rows).astype(np.float32).astype(np.float64)
    cache = {"rows": x, "keep": keep, "xs": [], "ts": []}
    x = np.maximum(x @ w["input_proj.0.weight"].T + w["input_proj.0.bias"], 0.0) * keep[0]
    cache["xs"].append(x)
    for i in range(blocks_of(w)):
        q = f"res_blocks.{i}.block."
        t = np.maximum(x @ w[q + "0.weight"].T + w[q + "0.bias"], 0.0) * keep[1 + 2 * i]
        x = np.maximum((t @ w[q + "3.weight"].T + w[q + "3.bias"] + x) * keep[2 + 2 * i], 0.0)
        cache["ts"].append(t)
        cache["xs"].append(x)
    f = np.maximum(x @ w["output_proj.0.weight"].T + w["output_proj.0.bias"], 0.0)
    cache["f"] = f
    out, cache["sig"] = {}, {}
    for k in R.HEADS:
        z = f @ w[f"param_heads.{k}.weight"].T + w[f"param_heads.{k}.bias"]
        a, b = R.RANGES[k]
        cache["sig"][k] = 1.0 / (1.0 + np.exp(-z))
        out[k] = cache["sig"][k] * a + b
    return out, cache


def backward64(state, cache, grad_heads):
    """grad_heads: {'use_gamma': (B, 1), 'gamma': (B, 1)} = dL/d(head output).  Returns the gradients by key, float64; the
    L_low and L_high heads (reached only through int()) get zeros."""
    w = {k: np.asarray(v, dtype=np.float64) for k, v in state.items()}
    g = {k: np.zeros_like(v) for k, v in w.items()}
    f = cache["f"]
    df = np.zeros_like(f)
    for k in ("gamma", "use_gamma"):
        s = cache["sig"][k]
        dz = np.asarray(grad_heads[k], dtype=np.float64).reshape(-1, 1) * R.RANGES[k][0] * s * (1.0 - s)
        g[f"param_heads.{k}.weight"] = dz.T @ f
        g[f"param_heads.{k}.bias"] = dz.sum(axis=0)
        df += dz @ w[f"param_heads.{k}.weight"]
    xs, ts, keep = cache["xs"], cache["ts"], cache["keep"]
    dz = df * (f > 0)
    g["output_proj.0.weight"], g["output_proj.0.bias"] = dz.T @ xs[-1], dz.sum(axis=0)
    dx = dz @ w["output_proj.0.weight"]
    for i in reversed(range(len(ts))):
        q = f"res_blocks.{i}.block."
        du = dx * (xs[i + 1] > 0) * keep[2 + 2 * i]           # relu, then the outer dropout, of u = block(x) + x
        g[q + "3.weight"], g[q + "3.bias"] = du.T @ ts[i], du.sum(axis=0)
        dz1 = (du @ w[q + "3.weight"]) * keep[1 + 2 * i] * (ts[i] > 0)
        g[q + "0.weight"], g[q + "0.bias"] = dz1.T @ xs[i], dz1.sum(axis=0)
        dx = dz1 @ w[q + "0.weight"] + du
    dz0 = dx * keep[0] * (xs[0] > 0)
    g["input_proj.0.weight"], g["input_proj.0.bias"] = dz0.T @ cache["rows"], dz0.sum(axis=0)
    return g


def enhance_loss64(images, references, params):
    """The gated DifferentiableEnhancement (:32-90) and ReferenceLoss(0.5, 0.5) in float64 for images (B, 3, H, W):
    (loss, l1, l2, {'use_gamma', 'gamma'}: dL/d(parameter) (B, 1))."""
    x = np.asarray(images, dtype=np.float64)
    r = np.asarray(references, dtype=np.float64)
    B, C, H, W = x.shape
    n = H * W
    s = np.empty_like(x)
    for b in range(B):
        lo = int(float(params["L_low"][b, 0]) / 100.0 * n)
        hi = int(float(params["L_high"][b, 0]) / 100.0 * n)
        for c in range(C):
            srt = np.sort(x[b, c].reshape(-1))
            s[b, c] = np.clip((x[b, c] - srt[lo]) / (srt[hi] - srt[lo] + 1e-8), 0.0, 1.0)
    u = np.asarray(params["use_gamma"], dtype=np.float64).reshape(B, 1, 1, 1)
    gm = np.asarray(params["gamma"], dtype=np.float64).reshape(B, 1, 1, 1)
    pw = (s + 1e-8) ** (1.0 / gm)
    e = u * pw + (1.0 - u) * s
    o = np.clip(e, 0.0, 1.0)
    d = o - r
    l1, l2 = np.abs(d).mean(), (d * d).mean()
    de = (0.5 * np.sign(d) + 0.5 * 2.0 * d) / d.size * ((e >= 0.0) & (e <= 1.0))
    du = (de * (pw - s)).sum(axis=(1, 2, 3)).reshape(B, 1)
    dg = (de * u * pw * np.log(s + 1e-8) * (-1.0 / (gm * gm))).sum(axis=(1, 2, 3)).reshape(B, 1)
    return 0.5 * l1 + 0.5 * l2, l1, l2, {"use_gamma": du, "gamma": dg}


def step_grads64(state, images, references, rows, masks, p=P_DROP):
    """One step's forward and backward: (loss, l1, l2, the heads' outputs, the gradients by key)."""
    out, cache = forward64(state, rows, masks, p)
    loss, l1, l2, gh = enhance_loss64(images, references, out)
    return loss, l1, l2, out, backward64(state, cache, gh)


def total_norm64(grads):
    """clip_grad_norm_'s total norm over the tensors that have a gradient, in float64"""
    return float(np.sqrt(sum(float((np.asarray(v, dtype=np.float64) ** 2).sum()) for k, v in grads.items() if k not in FREE)))


def adam32(params, grads, exp_avg, exp_avg_sq, step, max_norm=1.0, lr=LR, betas=BETAS, eps=EPS):
    """clip_grad_norm_(max_norm) and one torch.optim.Adam step (single-tensor form) in float32, in place on the dicts of
    float32 arrays; ``step`` is the count after this step.  The tensors of FREE are left alone.  Returns (norm, coef)."""
    f32 = np.float32
    norm = total_norm64(grads)
    coef = f32(max_norm) / (f32(norm) + f32(1e-6))
    coef = f32(1.0) if coef > 1.0 else coef
    bc1, bc2 = 1.0 - betas[0] ** step, 1.0 - betas[1] ** step
    w1, b2, w2 = f32(1.0 - betas[0]), f32(betas[1]), f32(1.0 - betas[1])
    neg_step, bc2_sqrt = f32(-(lr / bc1)), f32(np.sqrt(bc2))
    with np.errstate(invalid="ignore"):
        for k in params:
            if k in FREE:
                continue
            g = np.asarray(grads[k], dtype=f32) * coef
            m, v = exp_avg[k], exp_avg_sq[k]
            m += w1 * (g - m)
            v *= b2
            v += (w2 * g) * g
            denom = np.sqrt(v) / bc2_sqrt + f32(eps)
            params[k] += neg_step * (m / denom)
    return norm, float(coef)


def ulps(got, want):
    """max |got - want| of one tensor in units of float32's spacing at the tensor's largest magnitude: an element that
    cancelled to near zero (exp_avg after a sign change) carries the absolute error of its operands, not its own ulp"""
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    top = np.abs(want).max()
    diff = float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max())
    return 0.0 if diff == 0.0 else diff / float(np.spacing(top)) if top > 0 else float("inf")


def grad_error(got, want):
    """max|got - want| / max|want| of one tensor (0 for an all-zero tensor that is matched)"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    top = np.abs(want).max()
    diff = np.abs(got - want).max()
    return 0.0 if diff == 0.0 else float(diff / top) if top > 0 else float("inf")
