#!/usr/bin/env python3
"""One training step of EndToEndTrainer's stack with the features given, B = 4 and B = 32 images of
256 x 256, ParameterPredictor (79, 256, 3):
  ours      uw.EndToEndTrainer.train_step: train-mode MLP, fused gated enhancement + ReferenceLoss and its backward, the MLP's
            backward, clip + Adam, one host read (the loss)
  baseline  what the library offered before: the same network as torch modules in train mode on the device feeding
            uw.ReferenceLoss().through(uw.GatedDifferentiableEnhancement(), ...), loss.backward(), clip_grad_norm_(1.0),
            torch.optim.Adam(lr=1e-4), loss.item()
alternated rep by rep in one process after a warm-up, medians of --reps repetitions (HIP events around each step, host read
included).  Then the parts of our step on their own, and the launches of each from the library's per-kernel timing.

usage: python profiles/mlp_train_bench.py [--reps N]      (profiles/mlp_train_bench.txt holds the default output)"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import underwater_image_enhancement_amd as uw  # noqa: E402
import gated_predictor_ref as R  # noqa: E402
from gated_u8_bench import timed  # noqa: E402


class TorchPredictor(torch.nn.Module):
    """deep_learning_parameters.ParameterPredictor's layers under the reference's names (train mode: Dropout(0.3) live)"""

    def __init__(self, state):
        super().__init__()
        h, f = state["input_proj.0.weight"].shape
        nn = torch.nn

        class Block(nn.Module):
            def __init__(self):
                super().__init__()
                self.block = nn.Sequential(nn.Linear(h, h), nn.ReLU(), nn.Dropout(0.3), nn.Linear(h, h))
                self.relu, self.dropout = nn.ReLU(), nn.Dropout(0.3)

            def forward(self, x):
                return self.relu(self.dropout(self.block(x) + x))

        self.input_proj = nn.Sequential(nn.Linear(f, h), nn.ReLU(), nn.Dropout(0.3))
        self.res_blocks = nn.ModuleList([Block() for _ in range(3)])
        self.output_proj = nn.Sequential(nn.Linear(h, h // 2), nn.ReLU())
        self.param_heads = nn.ModuleDict({k: nn.Linear(h // 2, 1) for k in R.HEADS})
        self.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()})

    def forward(self, x):
        x = self.input_proj(x)
        for b in self.res_blocks:
            x = b(x)
        f = self.output_proj(x)
        return {k: torch.sigmoid(self.param_heads[k](f)) * R.RANGES[k][0] + R.RANGES[k][1] for k in R.HEADS}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    args = ap.parse_args()
    dev = uw.get_device(0)
    rng = np.random.default_rng(0)
    state = R.seeded_state(20261018)
    print(f"{'B':>4} {'ours ms':>9} {'baseline ms':>12} {'baseline / ours':>16}   parts of ours: "
          f"{'MLP fwd':>8} {'MLP bwd':>8} {'clip+Adam':>10}")
    counts = {}
    for B in (4, 32):
        img = dev.tensor(rng.integers(0, 256, (B, 3, 256, 256)).astype(np.float32) / np.float32(255.0))
        ref = dev.tensor(rng.random((B, 3, 256, 256), dtype=np.float32))
        feat = dev.tensor(rng.standard_normal((B, 79)).astype(np.float32))
        ours = uw.EndToEndTrainer(state)
        net = TorchPredictor(state).to(dev.torch_device).train()
        opt = torch.optim.Adam(net.parameters(), lr=1e-4)
        crit, enh = uw.ReferenceLoss(0.5, 0.5), uw.GatedDifferentiableEnhancement()

        def step_ours():
            return ours.train_step(img, ref, feat)[0]

        def step_base():
            loss, _ = crit.through(enh, img, net(feat), ref)
            opt.zero_grad()
            loss.backward()
            torch.nn.utils.clip_grad_norm_(net.parameters(), max_norm=1.0)
            opt.step()
            return loss.item()

        a, b = timed([step_ours, step_base], args.reps)
        ws = dev.mlp_train_workspace(B, 256, 3)
        gcols = dev.tensor(rng.standard_normal((B, 4)).astype(np.float32))
        h = ours._handle
        fwd, bwd, adam = timed([lambda: dev.mlp_train_forward(h, feat, ws, 0.3), lambda: dev.mlp_backward(h, feat, ws, gcols),
                                lambda: dev.mlp_adam_step(h, 1e-4, (0.9, 0.999), 1e-8, 1.0)], args.reps)
        print(f"{B:>4} {a:9.3f} {b:12.3f} {b / a:16.2f} {'':>17} {fwd:8.3f} {bwd:8.3f} {adam:10.3f}")
        for tag, fn in (("MLP forward", lambda: dev.mlp_train_forward(h, feat, ws, 0.3)), ("MLP backward", lambda: dev.mlp_backward(h, feat, ws, gcols)),
                        ("clip + Adam", lambda: dev.mlp_adam_step(h, 1e-4, (0.9, 0.999), 1e-8, 1.0)), ("whole step", step_ours)):
            dev.profile(True)
            fn()
            rows = dev.profile_rows()
            dev.profile(False)
            counts[(B, tag)] = (sum(c for _, c in rows.values()), sum(ms for ms, _ in rows.values()))
        ours.close()
    print("\nlaunches of the library per call (its per-kernel HIP-event timing; the sum of the kernels' own times in ms)")
    for (B, tag), (n, ms) in counts.items():
        print(f"{B:>4} {tag:<13} {n:>3} launches {ms:8.3f}")


if __name__ == "__main__":
    main()
