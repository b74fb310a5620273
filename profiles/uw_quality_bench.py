#!/usr/bin/env python3
"""What the underwater scores (uwie_underwater_scores_u8: UCIQE, UIQM; DESIGN.md "Underwater quality metrics") cost.

1. The two passes: k_uwq_stream (LAB, three histograms, three float64 sums) and k_uwq_tiles (Sobel, block extrema, two
   logarithms per block), each timed by the library's HIP-event pair with the profile filter on that one kernel, alternated
   launch by launch in one process with k_qa_maps, the streaming pass of uwie_quality_scores: the same table-driven LAB and
   LDS histograms without any float64 arithmetic per pixel.  All three read 3 B/px.
2. The whole call against uwie_quality_scores (the yardstick the library already had) on the same frames, alternated
   call by call.

at 16 x 2160 x 3840 and 8 x 1080 x 1920, random bytes.  The scores of the last frame are compared with the definition's
(tests/uw_quality_ref.py) before anything is timed.

usage: python profiles/uw_quality_bench.py [--reps N]      (profiles/uw_quality_bench.txt holds the default output)"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import underwater_image_enhancement_amd as uw  # noqa: E402
from underwater_image_enhancement_amd import _lib  # noqa: E402
import uw_quality_ref as ref  # noqa: E402

SHAPES = ((16, 2160, 3840), (8, 1080, 1920))


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


def call_ms(fns, reps):
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
    tw, th = _lib.underwater_plan(2160, 3840)
    print(f"k_uwq_tiles: {tw} x {th} tile per 256-thread workgroup; medians of {args.reps} alternated runs")
    for B, H, W in SHAPES:
        host = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
        frames = dev.tensor(host)
        px = B * H * W
        under = lambda: dev.underwater_scores(frames)  # noqa: E731
        generic = lambda: dev.quality_scores(frames)  # noqa: E731
        err = np.abs(under()[B - 1].cpu().numpy() - ref.scores(host[B - 1]))
        assert err.max() <= 1e-9, err
        ms = kernel_ms(dev, [("k_uwq_stream", under), ("k_uwq_tiles", under), ("k_uwq_finish", under), ("k_qa_maps", generic)], args.reps)
        print(f"\n{B} x {H} x {W}: 3 B/px read; last frame within {err.max():.1e} of the definition")
        print(f"{'kernel':<16} {'ms':>8} {'GB/s':>8} {'Gpx/s':>8}")
        for label, t in zip(("k_uwq_stream", "k_uwq_tiles", "k_uwq_finish", "k_qa_maps"), ms):
            print(f"{label:<16} {t:8.3f} {3 * px / t / 1e6:8.0f} {px / t / 1e6:8.1f}")
        c = call_ms([under, generic], args.reps)
        print(f"whole call: uwie_underwater_scores_u8 {c[0]:.3f} ms | uwie_quality_scores (u8 frames) {c[1]:.3f} ms | ratio {c[0] / c[1]:.2f}")
        assert dev.check_status() == 0
        del frames
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
