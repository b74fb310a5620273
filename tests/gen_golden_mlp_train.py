"""Generate tests/golden/mlp_train.npz: steps of the REAL deep_learning_parameters.EndToEndTrainer on the CPU.

TEST INFRASTRUCTURE, run by hand where the reference project is importable (its location: oracle/gen_golden.py's REF), in the
style of tests/gen_golden_gated_predictor.py.  Only arrays travel.  The network is the stored (79, 64, 1) one of
tests/golden/gated_predictor.npz; B = 4, images u8 / 255 of 3 x 16 x 20, uniform references, standard-normal features.

Case A: four consecutive calls of the real ``train_epoch`` (one batch each) under ``torch.manual_seed``.  Per step the
dropout masks (forward hooks on every ``nn.Dropout``, in call order), the four head outputs, the loss and its parts, and every
gradient after ``backward()`` (the clip coefficient is 1: the generator asserts the norm is below ``max_norm``); the
parameters and Adam's state after steps 1 and 4.
Case B: ``train_epoch``'s body written out here with ``max_norm = 0.005``, two steps on case A's first two batches: the same
records, the gradients before the clip, the parameters and Adam's state after step 2.

The generator reseeds until, at every step, every ``L / 100 * n`` lies at least 1e-3 from an integer (a rounding difference
cannot move a sorted position), the exact zeros of every golden gradient are the exact zeros of the float64 restatement
(tests/mlp_train_ref.py) and no others, case B's norm exceeds its ``max_norm`` and case A's is below 1.

Run:  python tests/gen_golden_mlp_train.py   (torch CPU, float32)
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
import mlp_train_ref as T  # noqa: E402

OUT = os.path.join(HERE, "golden", "mlp_train.npz")
DIMS = (79, 64, 1)
B_MAX_NORM = 0.005


class Unfit(Exception):
    pass


def batches(rng, count):
    out = []
    for _ in range(count):
        u8 = rng.integers(0, 256, (4, 3, 16, 20)).astype(np.uint8)
        out.append({"u8": u8, "image": u8.astype(np.float32) / np.float32(255.0),
                    "reference": rng.random((4, 3, 16, 20), dtype=np.float32),
                    "features": rng.standard_normal((4, 79)).astype(np.float32)})
    return out


def attempt(D, torch, state, seed):
    rng = np.random.default_rng(seed)
    data = batches(rng, 4)
    out = {"seed": np.array(seed), "dims": np.array(DIMS), "b/max_norm": np.array(B_MAX_NORM)}
    for i, b in enumerate(data):
        out[f"batch/{i}/u8"], out[f"batch/{i}/reference"], out[f"batch/{i}/features"] = b["u8"], b["reference"], b["features"]

    def fresh():
        net = D.ParameterPredictor(*DIMS)
        assert [k for k, _ in net.state_dict().items()] == list(state), "state_dict() order"
        net.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in state.items()})
        trainer = D.EndToEndTrainer(net, device="cpu")
        seen = {"masks": [], "heads": None}
        drops = [m for m in net.modules() if isinstance(m, torch.nn.Dropout)]
        assert len(drops) == T.sites(DIMS[2]) and all(m.p == T.P_DROP for m in drops)
        for m in drops:
            m.register_forward_hook(lambda mod, args, res: seen["masks"].append((res != 0).numpy().astype(np.uint8)))
        net.register_forward_hook(lambda mod, args, res: seen.__setitem__("heads", {k: v.detach().numpy().copy() for k, v in res.items()}))
        return net, trainer, seen

    def tensors(b):
        return {k: torch.from_numpy(b[k]) for k in ("image", "reference", "features")}

    def record(tag, net, trainer, seen, b, loss, parts, before):
        """one step's records; ``before``: the parameters the step started from"""
        masks = np.stack(seen["masks"])
        seen["masks"].clear()
        assert masks.shape == (T.sites(DIMS[2]), 4, DIMS[1])
        out[f"{tag}/masks"] = masks
        n = 16 * 20
        for k in R.HEADS:
            out[f"{tag}/{k}"] = seen["heads"][k]
        for k in ("L_low", "L_high"):
            pos = seen["heads"][k].astype(np.float64) / 100.0 * n
            if np.abs(pos - np.round(pos)).min() < 1e-3:
                raise Unfit(f"{tag}: a sorted position within 1e-3 of an integer")
        out[f"{tag}/loss"], out[f"{tag}/l1"], out[f"{tag}/l2"] = np.array(loss), np.array(parts["l1"]), np.array(parts["l2"])
        _, _, _, _, g64 = T.step_grads64(before, b["image"], b["reference"], b["features"], masks)
        for k, p in net.named_parameters():
            if k in T.FREE:
                assert p.grad is None, k
                continue
            g = p.grad.numpy().copy()
            if not np.array_equal(g == 0, g64[k] == 0):
                raise Unfit(f"{tag}: the zeros of {k} differ from the float64 restatement's")
            out[f"{tag}/grad/{k}"] = g
        return masks

    def snapshot(tag, net, trainer):
        sd = trainer.optimizer.state_dict()["state"]
        names = [k for k, _ in net.named_parameters()]
        assert sorted(sd) == [i for i, k in enumerate(names) if k not in T.FREE], sorted(sd)
        for i, k in enumerate(names):
            out[f"{tag}/param/{k}"] = net.state_dict()[k].numpy().copy()
            if i in sd:
                assert sd[i]["step"].dtype == torch.float32 and sd[i]["step"].dim() == 0
                out[f"{tag}/exp_avg/{k}"], out[f"{tag}/exp_avg_sq/{k}"] = sd[i]["exp_avg"].numpy().copy(), sd[i]["exp_avg_sq"].numpy().copy()
        out[f"{tag}/step"] = np.array(float(next(iter(sd.values()))["step"]))

    def norm_of(net):
        return float(np.sqrt(sum(float((p.grad.double() ** 2).sum()) for p in net.parameters() if p.grad is not None)))

    # case A: the real loop
    torch.manual_seed(seed)
    net, trainer, seen = fresh()
    for s in range(4):
        before = {k: v.numpy().copy() for k, v in net.state_dict().items()}
        loss, parts = trainer.train_epoch([tensors(data[s])])
        record(f"a/{s}", net, trainer, seen, data[s], loss, parts, before)
        out[f"a/{s}/norm"] = np.array(norm_of(net))
        if not out[f"a/{s}/norm"] < 1.0:
            raise Unfit(f"a/{s}: the norm {out[f'a/{s}/norm']} is not below 1")
        if s in (0, 3):
            snapshot(f"a/after{s + 1}", net, trainer)

    # case B: the loop body (:273-293) with a smaller max_norm
    torch.manual_seed(seed + 1)
    net, trainer, seen = fresh()
    net.train()
    for s in range(2):
        before = {k: v.numpy().copy() for k, v in net.state_dict().items()}
        b = tensors(data[s])
        enhanced = trainer.enhancement(b["image"], net(b["features"]))
        loss, parts = trainer.criterion(enhanced, b["reference"])
        trainer.optimizer.zero_grad()
        loss.backward()
        record(f"b/{s}", net, trainer, seen, data[s], loss.item(), parts, before)  # the gradients before the clip
        out[f"b/{s}/norm"] = np.array(norm_of(net))
        if not out[f"b/{s}/norm"] > B_MAX_NORM:
            raise Unfit(f"b/{s}: the norm {out[f'b/{s}/norm']} does not exceed {B_MAX_NORM}")
        torch.nn.utils.clip_grad_norm_(net.parameters(), max_norm=B_MAX_NORM)
        trainer.optimizer.step()
    snapshot("b/after2", net, trainer)
    return out


def main():
    gg.import_reference()
    if "tqdm" not in sys.modules:
        try:
            import tqdm  # noqa: F401
        except ImportError:
            class Bar(list):  # train_epoch iterates its progress bar and calls set_postfix on it
                def __init__(self, it, **kw):
                    super().__init__(it)

                def set_postfix(self, *a, **kw):
                    pass

            bar = types.ModuleType("tqdm")
            bar.tqdm = Bar
            sys.modules["tqdm"] = bar
    sys.path.insert(0, gg.REF)
    import torch
    import deep_learning_parameters as D

    state = R.small_state(R.load_golden())
    for seed in range(20261101, 20261101 + 50):
        try:
            out = attempt(D, torch, state, seed)
        except Unfit as e:
            print("seed", seed, "does not fit:", e)
            continue
        np.savez_compressed(OUT, **out)
        print("seed", seed, "wrote", OUT, os.path.getsize(OUT), "bytes;",
              "norms a", [float(out[f"a/{s}/norm"]) for s in range(4)], "b", [float(out[f"b/{s}/norm"]) for s in range(2)])
        return
    raise SystemExit("no seed met the preconditions")


if __name__ == "__main__":
    main()
