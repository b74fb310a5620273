#!/usr/bin/env python3
"""What the patched dark channel (uwie_params.dark_patch, k_trans_patch; DESIGN.md "Dark channel over a patch") costs.

1. The kernel: k_trans_patch for dark_patch 3 / 15 / 31 against k_trans_init, alternated launch by launch in one process
   through uwie_transmission_init, each timed by the library's HIP-event pair with the profile filter on that one kernel.
   Both read 3 B/px and write 4 B/px; what the patched kernel takes beyond that is halo re-reads and LDS minima.  Its
   float32 plane is compared with the definition's on a crop before anything is timed.
2. The step: a whole strategy-2 call with dark_patch 15 against dark_patch 1 on the same unfused route (gf_fuse = 0), and
   against today's default (gf_fuse = 2), alternated call by call.

at 16 x 2160 x 3840 and 8 x 1080 x 1920, random bytes.

usage: python profiles/dark_patch_bench.py [--reps N]      (profiles/dark_patch_bench.txt holds the default output)"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import underwater_image_enhancement_amd as uw  # noqa: E402
from underwater_image_enhancement_amd import _lib  # noqa: E402
import dark_patch_ref as ref  # noqa: E402

SHAPES = ((16, 2160, 3840), (8, 1080, 1920))
PATCHES = (3, 15, 31)


def kernel_ms(dev, calls, reps):
    """calls: [(kernel name, function)]; median ms of each kernel's launch, the functions alternated rep by rep."""
    for _, fn in calls:
        fn()
        fn()
    ms = [[] for _ in calls]
    for _ in range(reps):
        for i, (name, fn) in enumerate(calls):
            dev.profile(True, only=name)
            fn()
            rows = dev.profile_rows()
            dev.profile(False)
            assert rows[name][1] == 1, (name, rows)
            ms[i].append(rows[name][0])
    return [float(np.median(m)) for m in ms]


def step_ms(fns, reps):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    dev = uw.get_device(0)
    rng = np.random.default_rng(0)
    tw, th = _lib.dark_patch_plan(2160, 3840, 15)
    print(f"k_trans_patch: {tw} x {th} output tile per 256-thread workgroup; medians of {args.reps} alternated runs")
    for B, H, W in SHAPES:
        host = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
        frames = dev.tensor(host)
        A = dev.tensor(np.tile(np.array([[0.8, 0.78, 0.82]], np.float32), (B, 1)))
        kinds = torch.zeros(B, dtype=torch.int32, device=dev.torch_device)
        px = B * H * W

        def stage(k):
            p = dev.params(_lib.SURFACE_SIX, 2, dark_patch=k)
            return lambda: dev.transmission_init(frames, A, kinds, p)[0]

        for k in PATCHES:  # the plane is the definition's (last frame, a crop that spans tile seams and the frame's corner)
            got = stage(k)()[B - 1, H - 200:, W - 300:].cpu().numpy()
            # (no window of the crop reaches further than 30 pixels up or left: a margin of 31 stands for the rest of the frame)
            want = ref.six_t0(host[B - 1, H - 231:, W - 331:], 0, (0.8, 0.78, 0.82), 0.5, k)[31:, 31:]
            assert np.array_equal(got, want), k
        names = ["k_trans_init"] + ["k_trans_patch"] * len(PATCHES)
        ms = kernel_ms(dev, list(zip(names, [stage(1)] + [stage(k) for k in PATCHES])), args.reps)
        print(f"\n{B} x {H} x {W}: one launch, 3 B/px read + 4 B/px written")
        print(f"{'kernel':<28} {'ms':>8} {'GB/s':>8} {'x k_trans_init':>15}")
        for label, t in zip(["k_trans_init"] + [f"k_trans_patch dark_patch={k}" for k in PATCHES], ms):
            print(f"{label:<28} {t:8.3f} {7 * px / t / 1e6:8.0f} {t / ms[0]:15.2f}")

        def step(k, fuse):
            p = dev.params(_lib.SURFACE_SIX, 2, dark_patch=k)

            def run():
                with dev.tuning(gf_fuse=fuse):
                    return dev.enhance_u8(frames, p)[0]
            return run

        s = step_ms([step(15, 0), step(1, 0), step(1, 2)], args.reps)
        print(f"strategy-2 step: dark_patch=15 {s[0]:.3f} ms | dark_patch=1, gf_fuse=0 (the same unfused route) {s[1]:.3f} ms | "
              f"dark_patch=1, gf_fuse=2 (the default) {s[2]:.3f} ms | the patch costs {s[0] - s[1]:+.3f} ms over the unfused route, "
              f"{s[0] - s[2]:+.3f} ms over the default")
        assert dev.check_status() == 0
        del frames
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
