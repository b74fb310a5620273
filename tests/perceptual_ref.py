"""Restatement of PerceptualLoss (vgg_16_UIE.py:257-269) on the CPU: mse_loss(F(pred), F(target)) with F =
vgg16().features[:16], in float32 and float64, and the float16 contract of torch.autocast with every rounding written out
(DESIGN.md section 14).  ``tensors``: the 14 weight / bias tensors in features.N order (convs 0, 2, 5, 7, 10, 12, 14)."""
import numpy as np
import torch
import torch.nn.functional as F

CONVS = ((0, 3, 64), (2, 64, 64), (5, 64, 128), (7, 128, 128), (10, 128, 256), (12, 256, 256), (14, 256, 256))
POOL_AFTER = (1, 3)  # pools follow conv1_2 and conv2_2 (positions in CONVS)


def seeded_weights(seed):
    """He-scaled float32 weights from numpy.random.default_rng(seed): w ~ N(0, 2 / (9 Cin)), b ~ N(0, 0.01), drawn in
    features.N order, weight before bias.  Returns the state dict of vgg16().features[:16]."""
    rng = np.random.default_rng(seed)
    state = {}
    for i, cin, cout in CONVS:
        state[f"{i}.weight"] = (rng.standard_normal((cout, cin, 3, 3)) * np.sqrt(2.0 / (9 * cin))).astype(np.float32)
        state[f"{i}.bias"] = (rng.standard_normal(cout) * 0.01).astype(np.float32)
    return state


def checksum(state):
    """float64 sum of |w| * (1 + index mod 7) over the 14 tensors in order: detects a different generator or rule."""
    s = 0.0
    for i, _, _ in CONVS:
        for n in ("weight", "bias"):
            a = np.asarray(state[f"{i}.{n}"], np.float64).reshape(-1)
            s += float(np.sum(np.abs(a) * (1.0 + np.arange(a.size) % 7)))
    return s


def tensors_of(state):
    return [torch.as_tensor(np.asarray(state[f"{i}.{n}"])) for i, _, _ in CONVS for n in ("weight", "bias")]


def features(x, tensors, dtype=torch.float32):
    """F(x) in ``dtype`` (float32 / float64), torch's own layer sequence."""
    h = x.to(dtype)
    for k in range(7):
        h = F.relu(F.conv2d(h, tensors[2 * k].to(dtype), tensors[2 * k + 1].to(dtype), padding=1))
        if k in POOL_AFTER:
            h = F.max_pool2d(h, 2, 2)
    return h


def features16(x, tensors):
    """autocast's float16 F(x): inputs, weights and biases rounded to float16; each conv accumulates in float32 and rounds
    its output (after the bias) to float16; ReLU and max-pool on float16.  Differentiable: the backward rounds each
    data-gradient to float16 where the casts sit (the conv accumulates its data-gradient in float32)."""
    h = x.half()
    for k in range(7):
        w = tensors[2 * k].half().float()
        b = tensors[2 * k + 1].half().float()
        h = (F.conv2d(h.float(), w, None, padding=1) + b[None, :, None, None]).half()
        h = F.relu(h)
        if k in POOL_AFTER:
            h = F.max_pool2d(h, 2, 2)
    return h


def loss_and_grad(pred, target, tensors, mode="f32", g=1.0):
    """(loss, dloss/dpred * g) as float64 numpy values of the restatement.  mode: 'f32', 'f64' or 'f16' (autocast's)."""
    p = torch.as_tensor(np.asarray(pred, np.float32)).clone()
    t = torch.as_tensor(np.asarray(target, np.float32))
    if mode == "f64":
        p = p.double()
    p.requires_grad_(True)
    with torch.no_grad():
        ft = features16(t, tensors) if mode == "f16" else features(t, tensors, p.dtype)
    fp = features16(p, tensors) if mode == "f16" else features(p, tensors, p.dtype)
    loss = F.mse_loss(fp.float(), ft.float()) if mode == "f16" else F.mse_loss(fp, ft)
    (loss * g).backward()
    return loss.detach().double().numpy(), p.grad.double().numpy()
