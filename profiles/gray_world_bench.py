#!/usr/bin/env python3
"""What the gray-world pre-pass (uwie_gray_world_u8) costs.

1. Its launches, each timed by the library's HIP-event pair with the profile filter on that one kernel, alternated launch by
   launch in one process with the kernels of uwie_diff_gated_u8 that move the same bytes: k_gw_sums (3 B/px read into
   per-frame integers) beside k_frame_hist (the same traffic into per-frame histograms), k_gw_apply (3 B/px read, 3 B/px
   written, float64 arithmetic per pixel) beside k_dg8_apply<1> (the same traffic through a byte table).
2. The whole call against the same numbers from torch float64 tensor operations on the device (asserted equal first).
3. A strategy-2 enhance step with and without ``gray_world=True``.

at 16 x 2160 x 3840 and 8 x 1080 x 1920, seeded bytes under a green cast.  The bytes and stats of the last frame are compared
with the contract's NumPy statement (tests/gray_world_ref.py) before anything is timed.

usage: python profiles/gray_world_bench.py [--reps N]      (profiles/gray_world_bench.txt holds the default output)"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import underwater_image_enhancement_amd as uw  # noqa: E402
from underwater_image_enhancement_amd import _lib  # noqa: E402
import gray_world_ref as ref  # noqa: E402

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


def torch_gray_world(x, red=1.0, blue=0.0):
    """The contract (max_gain = 0) in torch float64 tensor operations: sums of integers below 2^53 are exact in float64, every
    other step is one elementwise operation.  x: uint8 [B,H,W,3] on the device -> (uint8 [B,H,W,3], gains [B,3])."""
    f = x.to(torch.float64)
    r, g, b = f.unbind(-1)
    S_r, S_g, S_b = r.sum((1, 2)), g.sum((1, 2)), b.sum((1, 2))
    S_rg, S_bg = (r * g).sum((1, 2)), (b * g).sum((1, 2))
    # divisors as tensors: torch divides by a Python scalar through its reciprocal, which is not the contract's division
    N, c65025, three = (torch.full_like(S_r, v) for v in (float(x.shape[1] * x.shape[2]), 65025.0, 3.0))
    mean_r, mean_g, mean_b = S_r / N, S_g / N, S_b / N
    k_r = (red * (mean_g - mean_r).clamp_min(0.0)) / c65025
    k_b = (blue * (mean_g - mean_b).clamp_min(0.0)) / c65025
    m_r = (S_r + k_r * (255.0 * S_g - S_rg)) / N
    m_b = (S_b + k_b * (255.0 * S_g - S_bg)) / N
    gray = ((m_r + mean_g) + m_b) / three
    one = torch.ones_like(gray)
    s = [torch.where(m > 0, gray / m, one) for m in (m_r, mean_g, m_b)]
    v = lambda t: t.view(-1, 1, 1)  # noqa: E731
    w_r = v(s[0]) * r + v(s[0] * k_r) * ((255.0 - r) * g)
    w_g = v(s[1]) * g
    w_b = v(s[2]) * b + v(s[2] * k_b) * ((255.0 - b) * g)
    out = torch.stack([w_r, w_g, w_b], -1).clamp_max(255.0).round().to(torch.uint8)
    return out, torch.stack(s, 1)


def cast_frames(rng, B, H, W):
    """Seeded bytes under a green cast, each frame with a cast of its own."""
    host = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    for i in range(B):
        tint = np.array([0.25 + 0.01 * i, 0.9 - 0.01 * i, 0.7])
        host[i] = (host[i] * tint + np.array([0, 20, 10])).clip(0, 255).astype(np.uint8)
    return host


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    dev = uw.get_device(0)
    rng = np.random.default_rng(0)
    block_px, thread_px = _lib.gray_world_plan(2160, 3840)
    print(f"k_gw_sums: {block_px} pixels per 256-thread workgroup; k_gw_apply: {thread_px} pixels per thread and step; "
          f"medians of {args.reps} alternated runs")
    for B, H, W in SHAPES:
        host = cast_frames(rng, B, H, W)
        frames = dev.tensor(host)
        px = B * H * W
        cols = dev.tensor(np.stack([rng.uniform(5, 20, B), rng.uniform(85, 98, B), rng.uniform(0, 1, B),
                                    rng.uniform(1.0, 1.5, B)], axis=1).astype(np.float32))
        out_buf = torch.empty_like(frames)
        ours = lambda: dev.gray_world(frames, want_stats=True, out=out_buf)  # noqa: E731
        gated = lambda: dev.diff_gated_u8(frames, cols, want_u8=True, want_f32=False)[0]  # noqa: E731
        out, st = ours()
        want_st = ref.coeffs(host[B - 1])
        assert np.array_equal(out[B - 1].cpu().numpy(), ref.apply(host[B - 1], want_st)), "bytes differ from the contract"
        assert np.array_equal(st[B - 1].cpu().numpy().view(np.uint64), want_st.view(np.uint64)), "stats differ from the contract"
        names = ("k_gw_sums", "k_frame_hist", "k_gw_coeffs", "k_gw_apply", "k_dg8_apply<1>")
        fns = (ours, gated, ours, ours, gated)
        bpp = (3, 3, 0, 6, 6)
        ms = kernel_ms(dev, list(zip(names, fns)), args.reps)
        print(f"\n{B} x {H} x {W}: last frame equal to the contract, bytes and stats; mean gains "
              f"{st[:, 9].mean().item():.3f} / {st[:, 10].mean().item():.3f} / {st[:, 11].mean().item():.3f}")
        print(f"{'kernel':<16} {'B/px':>5} {'ms':>8} {'GB/s':>8} {'Gpx/s':>8}")
        for label, t, n in zip(names, ms, bpp):
            print(f"{label:<16} {n:>5} {t:8.3f} {n * px / t / 1e6:8.0f} {px / t / 1e6:8.1f}")
        print(f"k_gw_sums / k_frame_hist {ms[0] / ms[1]:.2f} | k_gw_apply / k_dg8_apply<1> {ms[3] / ms[4]:.2f}")

        t_out, t_gain = torch_gray_world(frames)
        assert torch.equal(t_out, out) and torch.equal(t_gain, st[:, 9:12]), "torch float64 gives other numbers"
        del t_out, t_gain
        c = call_ms([ours, lambda: torch_gray_world(frames)], max(3, args.reps // 4))
        print(f"whole call: uwie_gray_world_u8 {c[0]:.3f} ms | torch float64 tensor operations {c[1]:.3f} ms | ratio {c[1] / c[0]:.1f}")
        torch.cuda.empty_cache()

        p = dev.params(_lib.SURFACE_SIX, 2)
        plain = lambda: dev.enhance_u8(frames, p)[0]  # noqa: E731
        composed = lambda: dev.enhance_u8(dev.gray_world(frames)[0], p)[0]  # noqa: E731  (what enhance(x, gray_world=True) runs)
        s = call_ms([plain, composed], args.reps)
        print(f"strategy-2 step: plain {s[0]:.3f} ms | with the gray-world pre-pass {s[1]:.3f} ms | the pre-pass costs {s[1] - s[0]:+.3f} ms "
              f"({s[1] / s[0]:.2f} x)")
        assert dev.check_status() == 0
        del frames, out_buf, out
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
