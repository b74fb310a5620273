#!/usr/bin/env python3
"""EnhancementPredictor's way from u8 frames to u8 frames, three routes alternated in one process:
  (a) the float32 route to bytes: u8_to_f32, uwie_diff_enhance_f32, clamp_ / nan_to_num_ / clamp_, * 255, .to(uint8)
  (b) uwie_diff_enhance_u8, bytes out
  (c) uwie_diff_enhance_u8, float32 out
at 32 x 224 x 224, 8 x 1080 x 1920 and 8 x 2160 x 3840; the outputs are compared at every shape before anything is timed.
Then the per-launch times of (b) from the library's HIP-event timing, the apply kernel against its 6 B/px.
Parameters inside the network's ranges; frames of random bytes (the times do not depend on the values).

usage: python profiles/predictor_u8_bench.py [--reps N]      (profiles/predictor_u8_bench.txt holds the default output)"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

import underwater_image_enhancement_amd as uw  # noqa: E402

SHAPES = ((32, 224, 224), (8, 1080, 1920), (8, 2160, 3840))
HBM_TBS = 8.0  # MI355X peak


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
        cols = dev.tensor(np.stack([rng.uniform(2, 15, B), rng.uniform(60, 95, B), rng.uniform(0.3, 0.9, B),
                                    rng.uniform(1.0, 1.5, B)], axis=1).astype(np.float32))

        def route_a():
            out = dev.diff_enhance_f32(dev.u8_to_f32(u8), cols, planar=False).clamp_(0.0, 1.0)
            out = torch.nan_to_num_(out, nan=0.0, posinf=1.0, neginf=0.0).clamp_(0.0, 1.0)
            return (out * 255).to(torch.uint8)

        def route_b():
            return dev.diff_enhance_u8(u8, cols, 3, want_u8=True, want_f32=False)[0]

        def route_c():
            return dev.diff_enhance_u8(u8, cols, 3, want_u8=False, want_f32=True)[1]

        assert torch.equal(route_a(), route_b()), "bytes differ"
        assert torch.equal(dev.diff_enhance_f32(dev.u8_to_f32(u8), cols, planar=False).view(torch.int32), route_c().view(torch.int32)), \
            "float words differ"
        a, b, c = timed([route_a, route_b, route_c], args.reps)
        print(f"{B:>4} x {H:>4} x {W:>4} {a:17.3f} {b:14.3f} {c:15.3f} {a / b:6.2f} {a / c:6.2f}")
        per = {}
        for _ in range(max(5, args.reps // 3)):
            dev.profile(True)
            route_b()
            for name, (ms, _) in dev.profile_rows().items():
                per.setdefault(name, []).append(ms)
            dev.profile(False)
        rows[(B, H, W)] = {k: float(np.median(v)) for k, v in per.items()}
        del u8
        torch.cuda.empty_cache()
    print("\nper-launch times of (b) (library HIP-event timing, median); apply: 3 B/px read + 3 B/px written")
    print(f"{'B x H x W':>16} {'launch':<16} {'ms':>8} {'GB/s':>8} {'of HBM peak':>12}")
    for (B, H, W), per in rows.items():
        for name, ms in per.items():
            line = f"{B:>4} x {H:>4} x {W:>4} {name:<16} {ms:8.3f}"
            bpp = {"k_du8_apply": 6, "k_frame_hist": 3}.get(name)
            if bpp:
                gbs = bpp * B * H * W / ms / 1e6
                line += f" {gbs:8.0f} {gbs / (HBM_TBS * 1e3):12.3f}"
            print(line)


if __name__ == "__main__":
    main()
