#!/usr/bin/env python3
"""The gated stack's way from u8 frames to u8 frames, three routes alternated in one process:
  (a) the float32 route to bytes: u8_to_f32, uwie_diff_gated_f32, * 255, .to(uint8)
  (b) uwie_diff_gated_u8, bytes out
  (c) uwie_diff_gated_u8, float32 out
at 32 x 224 x 224, 8 x 1080 x 1920 and 8 x 2160 x 3840; the outputs are compared at every shape before anything is timed.
Then the per-launch times of (b) and (c) from the library's HIP-event timing, the apply kernel against its 6 (15) B/px and
against the 5.1 TB/s the MI355X's streaming kernels reach (k_trans_init).  Last, ParameterPredictor
(79, 256, 3) at B = 4 and 32 against the same network as torch modules on the device.
Parameters inside the network's ranges; frames of random bytes (a lookup's time does not depend on the values, its LDS bank
conflicts do: random bytes are the unfavourable case).

usage: python profiles/gated_u8_bench.py [--reps N]      (profiles/gated_u8_bench.txt holds the default output)"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import underwater_image_enhancement_amd as uw  # noqa: E402
import gated_predictor_ref as R  # noqa: E402

SHAPES = ((32, 224, 224), (8, 1080, 1920), (8, 2160, 3840))
STREAM_TBS = 5.1  # k_trans_init, DESIGN.md section 7


def timed(fns, reps):
    """Median ms of each function, the functions alternated rep by rep after a warm-up of each."""
    for fn in fns:
        fn()
        fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ms = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            ev[0].record()
            fn()
            ev[1].record()
            torch.cuda.synchronize()
            ms[i].append(ev[0].elapsed_time(ev[1]))
    return [float(np.median(m)) for m in ms]


def launches(dev, fn, reps):
    per = {}
    for _ in range(reps):
        dev.profile(True)
        fn()
        for name, (ms, _) in dev.profile_rows().items():
            per.setdefault(name, []).append(ms)
        dev.profile(False)
    return {k: float(np.median(v)) for k, v in per.items()}


def torch_predictor(state, device):
    """the same network as torch modules (eval mode: Dropout left out), returning the device's [B,4] columns"""
    lin = lambda k: torch.nn.Linear(state[k + ".weight"].shape[1], state[k + ".weight"].shape[0])  # noqa: E731

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.inp = lin("input_proj.0")
            self.blocks = torch.nn.ModuleList([torch.nn.ModuleList([lin(f"res_blocks.{i}.block.0"), lin(f"res_blocks.{i}.block.3")])
                                               for i in range(3)])
            self.outp = lin("output_proj.0")
            self.heads = torch.nn.ModuleList([lin(f"param_heads.{k}") for k in R.GATED_ORDER])

        def forward(self, x):
            x = torch.relu(self.inp(x.float()))
            for a, b in self.blocks:
                x = torch.relu(b(torch.relu(a(x))) + x)
            f = torch.relu(self.outp(x))
            return torch.cat([torch.sigmoid(h(f)) * R.RANGES[k][0] + R.RANGES[k][1] for h, k in zip(self.heads, R.GATED_ORDER)], dim=1)

    net = Net()
    mods = [("input_proj.0", net.inp)] + [(f"res_blocks.{i}.block.{j}", m) for i, ab in enumerate(net.blocks) for j, m in zip((0, 3), ab)]
    mods += [("output_proj.0", net.outp)] + [(f"param_heads.{k}", h) for k, h in zip(R.GATED_ORDER, net.heads)]
    with torch.no_grad():
        for key, m in mods:
            m.weight.copy_(torch.from_numpy(state[key + ".weight"]))
            m.bias.copy_(torch.from_numpy(state[key + ".bias"]))
    return net.eval().to(device)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    args = ap.parse_args()
    dev = uw.get_device(0)
    rng = np.random.default_rng(0)
    print(f"{'B x H x W':>16} {'(a) f32 route ms':>17} {'(b) u8 out ms':>14} {'(c) f32 out ms':>15} {'a/b':>6} {'a/c':>6}")
    rows = {}
    for B, H, W in SHAPES:
        u8 = dev.tensor(rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8))
        cols = dev.tensor(np.stack([rng.uniform(5, 20, B), rng.uniform(85, 98, B), rng.uniform(0, 1, B),
                                    rng.uniform(1.0, 1.5, B)], axis=1).astype(np.float32))

        def route_a():
            return (dev.diff_gated_f32(dev.u8_to_f32(u8), cols, planar=False) * 255).to(torch.uint8)

        def route_b():
            return dev.diff_gated_u8(u8, cols, want_u8=True, want_f32=False)[0]

        def route_c():
            return dev.diff_gated_u8(u8, cols, want_u8=False, want_f32=True)[1]

        assert torch.equal(route_a(), route_b()), "bytes differ"
        assert torch.equal(dev.diff_gated_f32(dev.u8_to_f32(u8), cols, planar=False).view(torch.int32), route_c().view(torch.int32)), \
            "float words differ"
        assert dev.check_status() == 0
        a, b, c = timed([route_a, route_b, route_c], args.reps)
        print(f"{B:>4} x {H:>4} x {W:>4} {a:17.3f} {b:14.3f} {c:15.3f} {a / b:6.2f} {a / c:6.2f}")
        n = max(5, args.reps // 3)
        rows[(B, H, W)] = (launches(dev, route_b, n), launches(dev, route_c, n))
        del u8
        torch.cuda.empty_cache()
    print("\nper-launch times (library HIP-event timing, median); apply: 3 B/px read + 3 (bytes) or 12 (floats) B/px written")
    print(f"{'B x H x W':>16} {'route':<6} {'launch':<16} {'ms':>8} {'GB/s':>8} {'of 5.1 TB/s':>12}")
    for (B, H, W), pers in rows.items():
        for route, per in zip("bc", pers):
            for name, ms in per.items():
                line = f"{B:>4} x {H:>4} x {W:>4} {route:<6} {name:<16} {ms:8.3f}"
                bpp = {"k_dg8_apply<1>": 6, "k_dg8_apply<2>": 15, "k_frame_hist": 3}.get(name)
                if bpp:
                    gbs = bpp * B * H * W / ms / 1e6
                    line += f" {gbs:8.0f} {gbs / (STREAM_TBS * 1e3):12.3f}"
                print(line)

    state = R.seeded_state(20261018)
    model = uw.ParameterPredictor(state)
    net = torch_predictor(state, dev.torch_device)
    print("\nParameterPredictor (79, 256, 3), float64 rows in, [B,4] out: device kernels against torch modules on the device")
    print(f"{'B':>4} {'uwie_mlp_forward ms':>20} {'torch ms':>10} {'torch / ours':>13} {'max |diff| / range':>19}")
    span = torch.tensor([R.SPAN[k] for k in R.GATED_ORDER], device=dev.torch_device)
    for B in (4, 32):
        x = dev.tensor(rng.standard_normal((B, 79)))
        with torch.no_grad():
            diff = float(((model.columns(x) - net(x)).abs() / span).max())
            ours, theirs = timed([lambda: model.columns(x), lambda: net(x)], args.reps)
        print(f"{B:>4} {ours:20.3f} {theirs:10.3f} {theirs / ours:13.2f} {diff:19.2e}")


if __name__ == "__main__":
    main()
