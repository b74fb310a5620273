"""Generate tests/golden/gated_predictor.npz: outputs of the REAL deep_learning_parameters.ParameterPredictor in eval mode
and of the real EndToEndTrainer.validate, on the CPU.

TEST INFRASTRUCTURE, run by hand where the reference project is importable (its location: oracle/gen_golden.py's REF).
The module is imported with oracle/gen_golden.py's inert stand-ins for the libraries it does not use here (and a
pass-through for its progress bar).  Only arrays travel: the (79, 256, 3) network is stored as its seed and a checksum
(tests/gated_predictor_ref.py draws it), the small (79, 64, 1) one with its weights.

Run:  python tests/gen_golden_gated_predictor.py   (torch CPU, float32)
"""
from __future__ import annotations

import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "oracle"))
sys.path.insert(0, HERE)
import gated_predictor_ref as R  # noqa: E402
import gen_golden as gg  # noqa: E402

OUT = os.path.join(HERE, "golden", "gated_predictor.npz")
SEED, SMALL_SEED = 20261018, 20261019


def main():
    gg.import_reference()
    if "tqdm" not in sys.modules:
        try:
            import tqdm  # noqa: F401
        except ImportError:
            bar = types.ModuleType("tqdm")
            bar.tqdm = lambda it, **kw: it
            sys.modules["tqdm"] = bar
    sys.path.insert(0, gg.REF)
    import torch
    import deep_learning_parameters as D

    rng = np.random.default_rng(20261018)
    out = {"seed": np.array(SEED), "dims": np.array([79, 256, 3])}

    def module(state, dims):
        net = D.ParameterPredictor(*dims).eval()
        assert [k for k, _ in net.state_dict().items()] == list(state), "state_dict() order"
        net.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()})
        return net

    state = R.seeded_state(SEED)
    out["checksum"] = np.array(R.checksum(state))
    net = module(state, (79, 256, 3))
    rows = {"unit": rng.standard_normal((6, 79)), "large": rng.standard_normal((5, 79)) * 30.0,
            "one": rng.standard_normal((1, 79))}
    for tag, r in rows.items():  # float64 rows, as FeatureExtractor gives them; the dataset's .float() rounds them
        with torch.no_grad():
            res = net(torch.from_numpy(r).float())
        assert list(res) == list(R.HEADS)
        out[f"{tag}/rows"] = r
        for k, v in res.items():
            assert tuple(v.shape) == (r.shape[0], 1) and v.dtype == torch.float32
            out[f"{tag}/{k}"] = v.numpy()
        print(tag, {k: v.numpy().ravel()[:3] for k, v in res.items()})

    small = R.seeded_state(SMALL_SEED, 79, 64, 1)
    for k, v in small.items():
        out[f"small/state/{k}"] = v
    snet = module(small, (79, 64, 1))
    r = rng.standard_normal((4, 79))
    with torch.no_grad():
        res = snet(torch.from_numpy(r).float())
    out["small/rows"] = r
    for k, v in res.items():
        out[f"small/{k}"] = v.numpy()

    # EndToEndTrainer.validate over two dict batches of 2 x 3 x 16 x 20
    trainer = D.EndToEndTrainer(snet, device="cpu")
    batches = []
    for i in range(2):
        img = rng.integers(0, 256, (2, 3, 16, 20)).astype(np.float32) / np.float32(255.0)
        ref = rng.random((2, 3, 16, 20), dtype=np.float32)
        feat = rng.standard_normal((2, 79)).astype(np.float32)
        batches.append({"image": torch.from_numpy(img), "reference": torch.from_numpy(ref), "features": torch.from_numpy(feat)})
        out[f"validate/{i}/image"], out[f"validate/{i}/reference"], out[f"validate/{i}/features"] = img, ref, feat
    loss, parts = trainer.validate(batches)
    out["validate/loss"], out["validate/l1"], out["validate/l2"] = np.array(loss), np.array(parts["l1"]), np.array(parts["l2"])
    # the per-batch values the average is made of (validate's loop body)
    crit, enh = D.ReferenceLoss(0.5, 0.5), D.DifferentiableEnhancement()
    for i, b in enumerate(batches):
        with torch.no_grad():
            l, p = crit(enh(b["image"], snet(b["features"])), b["reference"])
        out[f"validate/{i}/loss"], out[f"validate/{i}/l1"], out[f"validate/{i}/l2"] = np.array(l.item()), np.array(p["l1"]), np.array(p["l2"])
    assert abs(sum(float(out[f"validate/{i}/loss"]) for i in range(2)) / 2 - loss) < 1e-12
    print("validate:", loss, parts)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
