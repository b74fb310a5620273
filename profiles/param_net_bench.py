#!/usr/bin/env python3
"""ImprovedVGGParameterNet timings: the eval-mode forward through (a) torch's route
(param_net_torch on the device, MIOpen) and (b) the device kernels (VGGParameterNet), alternated, at 1, 4 and 32 x 3 x 224
x 224; per-layer times of conv4_1 ... conv4_3 and the head from the library's per-launch HIP-event timing; and
EnhancementPredictor.enhance_batch on 1080p frames at batch 1 and 16.  Seeded weights (tests/param_net_ref.py); the times
do not depend on the values.

--kernels: device forwards only, for  rocprofv3 --kernel-trace --stats -- python profiles/param_net_bench.py --kernels

usage: python profiles/param_net_bench.py [--reps N] [--kernels]
(profiles/param_net_bench.txt holds the default output, profiles/param_net_kernel_stats.csv the trace stats)"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import param_net_ref as PN  # noqa: E402
import underwater_image_enhancement_amd as uw  # noqa: E402

# forward FLOP of one 224 x 224 image per conv (2 * H * W * Cin * Cout * 9)
CONV_SHAPES = [(224, 3, 64), (224, 64, 64), (112, 64, 128), (112, 128, 128), (56, 128, 256), (56, 256, 256), (56, 256, 256),
               (28, 256, 512), (28, 512, 512), (28, 512, 512)]
PEAK_TF = 157.3  # f32 MFMA (MI355X)
HEAD = ("pn avgpool", "pn fusion.0", "pn fusion.4", "pn attention.0", "pn attention.2", "pn heads.0", "pn heads.3")


def timed_pair(fns, reps):
    """Median ms of each function, the functions alternated rep by rep after a warm-up of each."""
    for fn in fns:
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--kernels", action="store_true")
    args = ap.parse_args()
    dev = uw.get_device(0)
    state = PN.seeded_state(1)
    net = uw.VGGParameterNet(state, device=0)
    tm = net.torch_module(dev.torch_device)
    rng = np.random.default_rng(0)
    if args.kernels:
        img = dev.tensor(rng.standard_normal((32, 3, 224, 224)).astype(np.float32))
        feats = dev.tensor(rng.random((32, 79), dtype=np.float32))
        for _ in range(args.reps):
            net(img, feats)
        torch.cuda.synchronize()
        return
    fl = sum(2.0 * h * h * ci * co * 9 for h, ci, co in CONV_SHAPES)
    print(f"trunk forward: {fl / 1e9:.1f} GFLOP per 224^2 image")
    print(f"{'batch':>5} {'torch (MIOpen) ms':>18} {'device ms':>10} {'device TFLOP/s':>15}")
    per_batch = {}
    for B in (1, 4, 32):
        img = dev.tensor(rng.standard_normal((B, 3, 224, 224)).astype(np.float32))
        feats = dev.tensor(rng.random((B, 79), dtype=np.float32))

        def torch_route():
            with torch.no_grad():
                tm(img, feats)

        def device_route():
            net(img, feats)

        t_ms, d_ms = timed_pair([torch_route, device_route], args.reps)
        print(f"{B:>5} {t_ms:18.3f} {d_ms:10.3f} {fl * B / d_ms / 1e9:15.1f}")
        per = {}
        device_route()
        for _ in range(args.reps):
            dev.profile(True)
            device_route()
            for name, (ms, _) in dev.profile_rows().items():
                per.setdefault(name, []).append(ms)
            dev.profile(False)
        per_batch[B] = {k: float(np.median(v)) for k, v in per.items()}
    print("\nper-launch times (library HIP-event timing, median): conv4_x as TFLOP/s and share of the f32 MFMA peak")
    print(f"{'batch':>5} {'launch':<18} {'ms':>8} {'TFLOP/s':>8} {'of peak':>8}")
    for B, per in per_batch.items():
        for k, (h, ci, co) in enumerate(CONV_SHAPES[7:]):
            name = f"vgg conv4_{k + 1}"
            tf = 2.0 * h * h * ci * co * 9 * B / per[name] / 1e9
            print(f"{B:>5} {name[4:]:<18} {per[name]:8.3f} {tf:8.1f} {tf / PEAK_TF:8.2f}")
        head = sum(per[n] for n in HEAD if n in per)
        print(f"{B:>5} {'avgpool + head':<18} {head:8.3f}")
    print("\nEnhancementPredictor.enhance_batch, 1080 x 1920 frames (input_size 224)")
    pred = uw.EnhancementPredictor(state, device=0)
    for B in (1, 16):
        frames = dev.tensor(rng.integers(0, 256, (B, 1080, 1920, 3), dtype=np.uint8))
        (ms,) = timed_pair([lambda: pred.enhance_batch(frames)], max(3, args.reps // 4))
        print(f"batch {B:>2}: {ms:8.2f} ms per call, {ms / B:7.2f} ms per frame")


if __name__ == "__main__":
    main()
