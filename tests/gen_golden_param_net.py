"""Generate tests/golden/param_net.npz: the REAL vgg_16_UIE.ImprovedVGGParameterNet (vgg_16_UIE.py:135-255) in eval mode on
the CPU, float32, and the REAL use_trained_model.EnhancementPredictor on two small frames.

TEST INFRASTRUCTURE, run by hand where the reference project is importable (its location: oracle/gen_golden.py's REF).
The modules are imported with tests/gen_golden_train_batches.py's stand-ins (cv2's resize is tests/resize_ref.py's,
torchvision.transforms.Normalize the float32 sub / div).  torchvision.models.vgg16 is replaced by a stand-in that returns
torchvision's vgg16 layer list (all 31 layers, the later ones zero: the reference slices them away); the network is built
with pretrained=False and then given tests/param_net_ref.py's seeded_state(SEED): all ten convs, the head, and BatchNorm
running statistics that are not the identity.  The weights are not stored: the seed and a checksum of them are.

Stored per case: img, features (use_features cases), the pooled vector (forward hooks on avgpool and maxpool) and the four
parameters (B, 4) in param_heads order.  Predictor cases: the frame, predict_parameters' six values (in the reference's
key order) and enhance_image's output.

Run:  python tests/gen_golden_param_net.py
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
import gen_golden_train_batches as gt  # noqa: E402
import param_net_ref as PN  # noqa: E402
import resize_ref as RR  # noqa: E402

OUT = os.path.join(HERE, "golden", "param_net.npz")
SEED = 20261018
PRED_SIZE = 48  # EnhancementPredictor's input_size for the predictor cases (224 in the reference's default)
VGG16_CFG = [64, 64, "M", 128, 128, "M", 256, 256, 256, "M", 512, 512, 512, "M", 512, 512, 512, "M"]


def vgg16_stand_in(**_kwargs):
    """torchvision.models.vgg16(pretrained=False): an object whose .features is torchvision's layer list."""
    import torch.nn as nn

    layers, cin = [], 3
    for v in VGG16_CFG:
        if v == "M":
            layers.append(nn.MaxPool2d(kernel_size=2, stride=2))
        else:
            layers += [nn.Conv2d(cin, v, kernel_size=3, padding=1), nn.ReLU(inplace=True)]
            cin = v
    return types.SimpleNamespace(features=nn.Sequential(*layers))


def cases(rng):
    """tag -> (img, features or None, use_features)."""
    f = np.float32
    out = {}
    for tag, shape in (("ragged_2x3x20x27", (2, 3, 20, 27)), ("tiny_1x3x8x8", (1, 3, 8, 8)), ("square_3x3x32x32", (3, 3, 32, 32))):
        out[tag] = (rng.standard_normal(shape).astype(f), rng.random((shape[0], 79), dtype=f), True)
    out["nofeat_2x3x16x24"] = (rng.standard_normal((2, 3, 16, 24)).astype(f), None, False)
    big = (rng.standard_normal((2, 79)) * 30.0).astype(f)
    out["bigfeat_2x3x16x16"] = (rng.standard_normal((2, 3, 16, 16)).astype(f), big, True)
    return out


def main():
    import torch

    mods = gt.stand_ins()
    mods["torchvision.models"].vgg16 = vgg16_stand_in
    for name, m in mods.items():
        sys.modules[name] = m
    for name in ("tqdm",):
        sys.modules.setdefault(name, gg._Inert(name))
    sys.path.insert(0, gg.REF)
    import use_trained_model as U
    import vgg_16_UIE as V
    sys.path.remove(gg.REF)

    torch.set_num_threads(1)  # one summation order for the float32 convolutions

    def build(use_features):
        net = V.ImprovedVGGParameterNet(pretrained=False, hidden_dim=256, use_features=use_features)
        state = {k: torch.from_numpy(v) for k, v in PN.seeded_state(SEED, use_features).items()}
        missing, unexpected = net.load_state_dict(state, strict=False)
        assert not unexpected and all(k.endswith("num_batches_tracked") for k in missing), (missing, unexpected)
        return net.eval()

    out = {"seed": np.array(SEED), "checksum": np.array(PN.checksum(PN.seeded_state(SEED))),
           "checksum_nofeat": np.array(PN.checksum(PN.seeded_state(SEED, False), False))}
    nets = {True: build(True), False: build(False)}
    for tag, (img, feats, uf) in cases(np.random.default_rng(SEED)).items():
        net = nets[uf]
        got = {}
        hooks = [net.avgpool.register_forward_hook(lambda m, i, o: got.__setitem__("avg", o)),
                 net.maxpool.register_forward_hook(lambda m, i, o: got.__setitem__("max", o))]
        with torch.no_grad():
            p = net(torch.from_numpy(img), None if feats is None else torch.from_numpy(feats))
        for h in hooks:
            h.remove()
        B = img.shape[0]
        rec = {"img": img, "use_features": np.array(uf),
               "pooled": torch.cat([got["avg"].view(B, -1), got["max"].view(B, -1)], 1).numpy(),
               "params": torch.cat([p[k] for k in PN.KEYS], 1).numpy()}
        if feats is not None:
            rec["features"] = feats
        for k, v in rec.items():
            out[f"{tag}/{k}"] = v
        print(tag, rec["params"].tolist())
    # EnhancementPredictor on u8 / 255 frames (what process_single_image makes)
    pred = U.EnhancementPredictor.__new__(U.EnhancementPredictor)
    pred.device, pred.input_size, pred.model = "cpu", PRED_SIZE, nets[True]
    pred.enhancer = V.DifferentiableEnhancement().eval()
    pred.feature_extractor = V.vgg_features
    import torchvision.transforms as T
    pred.normalize = T.Normalize(mean=[0.485, 0.456, 0.406], std=[0.229, 0.224, 0.225])
    for name, (h, w, s) in (("pred_37x53", (37, 53, 1)), ("pred_30x20", (30, 20, 3))):
        frame = RR.synth_frame(h, w, s)
        img = frame.astype(np.float32) / 255.0
        params = pred.predict_parameters(img)
        out[f"{name}/frame"] = frame
        out[f"{name}/keys"] = np.array(list(params))
        out[f"{name}/values"] = np.array([params[k] for k in params], np.float64)
        out[f"{name}/enhanced"] = pred.enhance_image(img, params)
        print(name, params)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
