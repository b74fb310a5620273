"""Generate tests/golden/perceptual.npz: the REAL vgg_16_UIE.PerceptualLoss and CombinedLoss (vgg_16_UIE.py:257-303) under
CPU autograd, float32.

TEST INFRASTRUCTURE, run by hand where the reference project is importable (its location: oracle/gen_golden.py's REF).
The module is imported with oracle/gen_golden.py's inert stand-ins for the libraries it does not use here, as in
tests/gen_golden_refloss.py.  torchvision.models.vgg16 is replaced by a stand-in that returns torchvision's vgg16 layer
list (`features`, all 31 layers) with the first 16 layers' weights drawn by tests/perceptual_ref.py's seeded_weights(SEED)
(He-scaled float32 from numpy.random.default_rng) and the later layers zero (the reference slices them away).  The weights
are not stored: the seed and a checksum of them are.

Stored per case: pred (= enhanced), target (= reference), the PerceptualLoss value and its gradient for pred, and
CombinedLoss's l1, l2, perceptual parts, total and gradient for enhanced.

Run:  python tests/gen_golden_perceptual.py
"""
from __future__ import annotations

import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "oracle"))
sys.path.insert(0, HERE)
import gen_golden as gg  # noqa: E402
import perceptual_ref as PR  # noqa: E402

OUT = os.path.join(HERE, "golden", "perceptual.npz")
SEED = 20261017
VGG16_CFG = [64, 64, "M", 128, 128, "M", 256, 256, 256, "M", 512, 512, 512, "M", 512, 512, 512, "M"]


def vgg16_stand_in(**_kwargs):
    """torchvision.models.vgg16(pretrained=True) with seeded weights: an object whose .features is torchvision's list."""
    import torch
    import torch.nn as nn

    layers, cin = [], 3
    for v in VGG16_CFG:
        if v == "M":
            layers.append(nn.MaxPool2d(kernel_size=2, stride=2))
        else:
            layers += [nn.Conv2d(cin, v, kernel_size=3, padding=1), nn.ReLU(inplace=True)]
            cin = v
    features = nn.Sequential(*layers)
    state = PR.seeded_weights(SEED)
    with torch.no_grad():
        for i, m in enumerate(features):
            if isinstance(m, nn.Conv2d):
                if f"{i}.weight" in state:
                    m.weight.copy_(torch.from_numpy(state[f"{i}.weight"]))
                    m.bias.copy_(torch.from_numpy(state[f"{i}.bias"]))
                else:
                    m.weight.zero_()
                    m.bias.zero_()
    return types.SimpleNamespace(features=features)


def cases(rng):
    f = np.float32
    out = {}
    for tag, shape in (("ragged_2x3x20x27", (2, 3, 20, 27)), ("small_1x3x9x13", (1, 3, 9, 13)), ("square_3x3x16x16", (3, 3, 16, 16))):
        out[tag] = (rng.random(shape, dtype=f), rng.random(shape, dtype=f))
    p, t = rng.random((1, 3, 12, 10), dtype=f), rng.random((1, 3, 12, 10), dtype=f)
    p[0, 1, 5, 4] = np.nan
    out["nan_1x3x12x10"] = (p, t)
    return out


def main():
    for name in ("torchvision", "torchvision.models", "torchvision.transforms"):
        mod = gg._Inert(name)
        mod.__path__ = []
        sys.modules[name] = mod
    models = sys.modules["torchvision.models"]
    models.vgg16 = vgg16_stand_in
    sys.modules["torchvision"].models = models
    sys.modules["torchvision"].transforms = sys.modules["torchvision.transforms"]
    gg.import_reference()
    sys.path.insert(0, gg.REF)
    import torch
    import vgg_16_UIE as V

    torch.set_num_threads(1)  # one summation order for the float32 convolutions
    out = {"seed": np.array(SEED), "checksum": np.array(PR.checksum(PR.seeded_weights(SEED)))}
    for tag, (pred, target) in cases(np.random.default_rng(SEED)).items():
        crit = V.PerceptualLoss(device="cpu")
        x = torch.from_numpy(pred.copy()).requires_grad_(True)
        perc = crit(x, torch.from_numpy(target))
        perc.backward()
        comb = V.CombinedLoss(device="cpu")
        e = torch.from_numpy(pred.copy()).requires_grad_(True)
        total, parts = comb(e, torch.from_numpy(target))
        total.backward()
        rec = {"pred": pred, "target": target, "perceptual": perc.detach().numpy(), "grad_perceptual": x.grad.numpy(),
               "l1": np.float32(parts["l1"]), "l2": np.float32(parts["l2"]), "perceptual_part": np.float32(parts["perceptual"]),
               "total": total.detach().numpy(), "grad_enhanced": e.grad.numpy()}
        for k, v in rec.items():
            out[f"{tag}/{k}"] = v
        print(f"{tag}: perceptual {perc.item():.6g} total {total.item():.6g}")
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
