"""Restatement of ImprovedVGGParameterNet.forward (vgg_16_UIE.py:135-255) in eval mode, in float64 on the CPU (DESIGN.md
section 15), and the seeded stand-in weights of tests/gen_golden_param_net.py.  ``state``: the state dict (numpy or torch
values) under the reference's keys."""
import numpy as np
import torch
import torch.nn.functional as F

CONVS = ((0, 3, 64), (2, 64, 64), (5, 64, 128), (7, 128, 128), (10, 128, 256), (12, 256, 256), (14, 256, 256),
         (17, 256, 512), (19, 512, 512), (21, 512, 512))
POOL_AFTER = (1, 3, 6)  # pools follow conv1_2, conv2_2 and conv3_3 (positions in CONVS)
KEYS = ("omega", "gamma", "L_low", "L_high")
RANGES = {"omega": (0.3, 0.9), "gamma": (1.0, 1.5), "L_low": (2.0, 15.0), "L_high": (60.0, 95.0)}
H = 256  # hidden_dim


def layout(use_features=True):
    """(key, shape) of the float tensors in state-dict order (num_batches_tracked left out)."""
    out = []
    for i, cin, cout in CONVS:
        out += [(f"vgg_features.{i}.weight", (cout, cin, 3, 3)), (f"vgg_features.{i}.bias", (cout,))]
    bn = lambda p, c: [(f"{p}.{n}", (c,)) for n in ("weight", "bias", "running_mean", "running_var")]  # noqa: E731
    out += [("feature_fusion.0.weight", (2 * H, 1024 + (79 if use_features else 0))), ("feature_fusion.0.bias", (2 * H,))]
    out += bn("feature_fusion.1", 2 * H)
    out += [("feature_fusion.4.weight", (H, 2 * H)), ("feature_fusion.4.bias", (H,))] + bn("feature_fusion.5", H)
    out += [("attention.0.weight", (H // 4, H)), ("attention.0.bias", (H // 4,)), ("attention.2.weight", (H, H // 4)),
            ("attention.2.bias", (H,))]
    for k in KEYS:
        out += [(f"param_heads.{k}.0.weight", (H // 2, H)), (f"param_heads.{k}.0.bias", (H // 2,)),
                (f"param_heads.{k}.3.weight", (1, H // 2)), (f"param_heads.{k}.3.bias", (1,))]
    return out


def seeded_state(seed, use_features=True):
    """float32 weights from numpy.random.default_rng(seed), drawn in layout order: convs w ~ N(0, 2 / (9 Cin)),
    b ~ N(0, 0.01); Linear w ~ N(0, 1 / fan_in), b ~ N(0, 0.01); BatchNorm weight ~ U(0.5, 1.5), bias ~ N(0, 0.1),
    running_mean ~ N(0, 0.2), running_var ~ U(0.5, 2) (non-trivial, so that eval-mode BatchNorm is exercised)."""
    rng = np.random.default_rng(seed)
    state = {}
    for key, shape in layout(use_features):
        name = key.rsplit(".", 1)[1]
        bn = key.startswith(("feature_fusion.1.", "feature_fusion.5."))
        if bn and name == "weight":
            v = rng.uniform(0.5, 1.5, shape)
        elif bn and name == "bias":
            v = rng.standard_normal(shape) * 0.1
        elif name == "running_mean":
            v = rng.standard_normal(shape) * 0.2
        elif name == "running_var":
            v = rng.uniform(0.5, 2.0, shape)
        elif name == "weight" and len(shape) == 4:
            v = rng.standard_normal(shape) * np.sqrt(2.0 / (9 * shape[1]))
        elif name == "weight":
            v = rng.standard_normal(shape) * np.sqrt(1.0 / shape[1])
        else:
            v = rng.standard_normal(shape) * 0.01
        state[key] = v.astype(np.float32)
    return state


def checksum(state, use_features=True):
    """float64 sum of |w| * (1 + index mod 7) over the tensors in layout order: detects a different generator or rule."""
    s = 0.0
    for key, _ in layout(use_features):
        a = np.asarray(state[key], np.float64).reshape(-1)
        s += float(np.sum(np.abs(a) * (1.0 + np.arange(a.size) % 7)))
    return s


def forward(state, img, features=None, use_features=True, dtype=torch.float64):
    """(pooled [B,1024], params [B,4] in KEYS order) as float64 numpy values of the restatement in ``dtype``."""
    T = {k: torch.as_tensor(np.asarray(v)).to(dtype) for k, v in state.items() if not k.endswith("num_batches_tracked")}
    with torch.no_grad():
        h = torch.as_tensor(np.asarray(img)).to(dtype)
        for k, (i, _, _) in enumerate(CONVS):
            h = F.relu(F.conv2d(h, T[f"vgg_features.{i}.weight"], T[f"vgg_features.{i}.bias"], padding=1))
            if k in POOL_AFTER:
                h = F.max_pool2d(h, 2, 2)
        avg = h.mean(dim=(2, 3))
        pooled = torch.cat([avg, avg], dim=1)  # the reference's "maxpool" is an AdaptiveAvgPool2d as well
        x = pooled
        if use_features:
            x = torch.cat([pooled, torch.as_tensor(np.asarray(features, np.float32)).to(dtype)], dim=1)

        def bn(v, p):
            return (v - T[f"{p}.running_mean"]) / torch.sqrt(T[f"{p}.running_var"] + 1e-5) * T[f"{p}.weight"] + T[f"{p}.bias"]

        x = F.relu(bn(F.linear(x, T["feature_fusion.0.weight"], T["feature_fusion.0.bias"]), "feature_fusion.1"))
        x = F.relu(bn(F.linear(x, T["feature_fusion.4.weight"], T["feature_fusion.4.bias"]), "feature_fusion.5"))
        a = F.relu(F.linear(x, T["attention.0.weight"], T["attention.0.bias"]))
        x = x * torch.sigmoid(F.linear(a, T["attention.2.weight"], T["attention.2.bias"]))
        out = []
        for k in KEYS:
            r = F.linear(F.relu(F.linear(x, T[f"param_heads.{k}.0.weight"], T[f"param_heads.{k}.0.bias"])),
                         T[f"param_heads.{k}.3.weight"], T[f"param_heads.{k}.3.bias"])
            lo, hi = RANGES[k]
            out.append(torch.sigmoid(r) * (hi - lo) + lo)
        return pooled.double().numpy(), torch.cat(out, dim=1).double().numpy()
