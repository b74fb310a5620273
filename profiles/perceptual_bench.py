#!/usr/bin/env python3
"""PerceptualLoss timings: forward + backward of mse_loss(F(pred), F(target)) through
(a) torch's own route (vgg16_features16 on the device, MIOpen; under autocast for float16) and (b) the device kernels
(k_vgg.hip), and (c) one CombinedLoss.through step with each enhancement module, at 4 and 32 x 3 x 224 x 224.
Random He-scaled weights (tests/perceptual_ref.py); the times do not depend on the values.

--layers: per-conv times of the device route at 32 x 3 x 224 x 224 (the library's HIP-event timing of each launch, named
by layer; forward = the launches on pred and target, bwd = the data-gradient) with TFLOP/s against the MFMA peaks.
--kernels: device steps only, for  rocprofv3 --kernel-trace --stats -- python profiles/perceptual_bench.py --kernels

usage: python profiles/perceptual_bench.py [--reps N] [--layers | --kernels]
(profiles/perceptual_bench.txt holds the default and --layers output, profiles/perceptual_kernel_stats.csv the trace stats)"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import perceptual_ref as PR  # noqa: E402
import underwater_image_enhancement_amd as uw  # noqa: E402

# forward FLOP of one 224 x 224 image per conv (2 * H * W * Cin * Cout * 9)
CONV_SHAPES = [(224, 3, 64), (224, 64, 64), (112, 64, 128), (112, 128, 128), (56, 128, 256), (56, 256, 256), (56, 256, 256)]


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ms = []
    for _ in range(reps):
        ev[0].record()
        fn()
        ev[1].record()
        torch.cuda.synchronize()
        ms.append(ev[0].elapsed_time(ev[1]))
    return float(np.median(ms))


PEAK_TF = {"f32": 157.3, "f16": 2500.0}  # f32 MFMA, dense f16 MFMA (MI355X)


def device_step(crit, pred, target, ac):
    p = pred.detach().requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.float16, enabled=ac):
        loss = crit(p, target)
    loss.backward()


def layers(dev, crit, reps):
    B = 32
    rng = np.random.default_rng(B)
    pred = dev.tensor(rng.random((B, 3, 224, 224), dtype=np.float32))
    target = dev.tensor(rng.random((B, 3, 224, 224), dtype=np.float32))
    # the data-gradients run on autograd's backward thread, which this timing does not record: the kernel trace has them
    print(f"forward convs, {B} x 3 x 224 x 224, median of {reps} steps: ms per step (the launches on pred and target)")
    print(f"{'prec':>4} {'layer':<16} {'ms':>8} {'TFLOP/s':>8} {'of peak':>8}")
    for prec, ac in (("f32", False), ("f16", True)):
        device_step(crit, pred, target, ac)
        per = {}
        for _ in range(reps):
            dev.profile(True)
            device_step(crit, pred, target, ac)
            for name, (ms, _) in dev.profile_rows().items():
                per.setdefault(name, []).append(ms)
            dev.profile(False)
        for k, (h, ci, co) in enumerate(CONV_SHAPES):
            name = f"vgg conv{[1, 1, 2, 2, 3, 3, 3][k]}_{[1, 2, 1, 2, 1, 2, 3][k]}"
            ms = float(np.median(per[name]))
            tf = 2.0 * h * h * ci * co * 9 * B * 2 / ms / 1e9
            print(f"{prec:>4} {name[4:]:<16} {ms:8.3f} {tf:8.1f} {tf / PEAK_TF[prec]:8.2f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--layers", action="store_true")
    ap.add_argument("--kernels", action="store_true")
    args = ap.parse_args()
    dev = uw.get_device(0)
    state = PR.seeded_weights(1)
    crit = uw.PerceptualLoss(state)
    if args.layers:
        layers(dev, crit, args.reps)
        return
    if args.kernels:
        rng = np.random.default_rng(32)
        pred = dev.tensor(rng.random((32, 3, 224, 224), dtype=np.float32))
        target = dev.tensor(rng.random((32, 3, 224, 224), dtype=np.float32))
        for ac in (False, True):
            for _ in range(args.reps):
                device_step(crit, pred, target, ac)
        torch.cuda.synchronize()
        return
    cl = uw.CombinedLoss(weights=state)
    vgg = crit.features(dev.torch_device)
    fl = sum(2.0 * h * h * ci * co * 9 for h, ci, co in CONV_SHAPES)
    print(f"{'batch':>5} {'prec':>4} {'route':<28} {'ms':>8} {'TFLOP/s':>8}")
    for B in (4, 32):
        rng = np.random.default_rng(B)
        pred = dev.tensor(rng.random((B, 3, 224, 224), dtype=np.float32))
        target = dev.tensor(rng.random((B, 3, 224, 224), dtype=np.float32))
        flop = 3.0 * fl * B  # forward on pred and target + the data-gradient of pred
        for prec, ac in (("f32", False), ("f16", True)):
            def torch_route():
                p = pred.detach().requires_grad_(True)
                with torch.autocast("cuda", dtype=torch.float16, enabled=ac):
                    loss = torch.nn.functional.mse_loss(vgg(p), vgg(target))
                loss.backward()

            def device_route():
                p = pred.detach().requires_grad_(True)
                with torch.autocast("cuda", dtype=torch.float16, enabled=ac):
                    loss = crit(p, target)
                loss.backward()

            for name, fn in (("(a) torch vgg16_features16", torch_route), ("(b) device PerceptualLoss", device_route)):
                ms = timed(fn, args.reps)
                print(f"{B:>5} {prec:>4} {name:<28} {ms:8.3f} {flop / ms / 1e9:8.1f}")
            for gated in (False, True):
                mod = uw.GatedDifferentiableEnhancement() if gated else uw.DifferentiableEnhancement()
                t = lambda v: torch.full((B, 1), v, device=dev.torch_device)  # noqa: E731
                par = {"L_low": t(10.0), "L_high": t(90.0)}
                par.update({"use_gamma": t(0.5), "gamma": t(1.2)} if gated else {"omega": t(0.6), "gamma": t(1.2)})

                def step():
                    leaves = {k: v.clone().requires_grad_(k not in ("L_low", "L_high")) for k, v in par.items()}
                    with torch.autocast("cuda", dtype=torch.float16, enabled=ac):
                        total, _ = cl.through(mod, pred, leaves, target)
                    total.backward()

                ms = timed(step, args.reps)
                name = f"(c) CombinedLoss.through {'gated' if gated else 'vgg'}"
                print(f"{B:>5} {prec:>4} {name:<28} {ms:8.3f}")


if __name__ == "__main__":
    main()
