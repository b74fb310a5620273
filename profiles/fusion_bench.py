#!/usr/bin/env python3
"""What the multi-scale fusion (uwie_fusion_u8) costs.

1. Its launches, each timed by the library's HIP-event pair with the profile filter on that one kernel (a row per pyramid
   level), alternated launch by launch in one process.
2. The whole call beside uwie_gray_world_u8 and uwie_reference_scores_u8 on the same frames, and against the same bytes from
   torch float64 tensor operations on the device (asserted equal first), alternated call by call.

at 16 x 2160 x 3840 and 8 x 1080 x 1920, L = 6, gamma 2.2, seeded bytes under a green cast, each frame its own.  All four
results of the last frame are compared with the contract's NumPy statement (tests/fusion_ref.py) before anything is timed.

usage: python profiles/fusion_bench.py [--reps N]      (profiles/fusion_bench.txt holds the default output)"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import underwater_image_enhancement_amd as uw  # noqa: E402
from underwater_image_enhancement_amd import _lib  # noqa: E402
import fusion_ref as ref  # noqa: E402
from gray_world_bench import call_ms, cast_frames, kernel_ms  # noqa: E402

SHAPES = ((16, 2160, 3840), (8, 1080, 1920))
GAMMA, LEVELS = 2.2, 6


# ---------------------------------------------------------------- the contract in torch float64 tensor operations
def t_shift(p, d, axis):
    n = p.shape[axis]
    return p.index_select(axis, (torch.arange(n, device=p.device) + d).clamp_(0, n - 1))


def t_taps(p, axis):
    return ((t_shift(p, -2, axis) + t_shift(p, 2, axis)) + 4 * (t_shift(p, -1, axis) + t_shift(p, 1, axis))) + 6 * p


def t_blur(p):  # [B, H, W, ...]
    return t_taps(t_taps(p, 2), 1)


def t_weight(img, n):
    """img: int64 [B, H, W, 3] -> W_k float64 [B, H, W]"""
    r, g, b = img.unbind(-1)
    Y = (r * 9798 + g * 19235 + b * 3735 + 16384) >> 15
    lap = (4 * Y - t_shift(Y, -1, 1) - t_shift(Y, 1, 1) - t_shift(Y, -1, 2) - t_shift(Y, 1, 2)).abs()
    c255, c65025, three = (torch.full((), v, dtype=torch.float64, device=img.device) for v in (255.0, 65025.0, 3.0))
    wl = lap.to(torch.float64) / c255  # (divisors as tensors: torch divides by a Python scalar through its reciprocal)
    mu = img.sum((1, 2)).to(torch.float64) / torch.full((), float(n), dtype=torch.float64, device=img.device)
    d = mu[:, None, None, :] - t_blur(img).to(torch.float64) * 2.0 ** -8
    d2 = d * d
    sal = ((0.0 + d2[..., 0]) + d2[..., 1]) + d2[..., 2]
    q = ((img - Y[..., None]) ** 2).sum(-1)
    return (wl + sal / c65025) + torch.sqrt(q.to(torch.float64) / three) / c255


def t_reduce(p):
    return (t_taps(t_taps(p, 2), 1) * 2.0 ** -8)[:, ::2, ::2]


def t_expand_axis(p, size, axis):
    i = torch.arange(size, device=p.device)
    k = i // 2
    n = p.shape[axis]
    at = lambda j: p.index_select(axis, j.clamp(0, n - 1))  # noqa: E731
    even = ((at(k - 1) + at(k + 1)) + 6 * at(k)) * 0.125
    odd = (at(k) + at(k + 1)) * 0.5
    shape = [1] * p.dim()
    shape[axis] = size
    return torch.where((i % 2 == 0).view(shape), even, odd)


def t_expand(p, h, w):
    return t_expand_axis(t_expand_axis(p, w, 2), h, 1)


def torch_fusion(x, table, levels):
    """x: uint8 [B,H,W,3] on the device, table: uint8 [256] on the device -> uint8 [B,H,W,3]"""
    xi = x.to(torch.int64)
    n = x.shape[1] * x.shape[2]
    in1 = table[xi].to(torch.int64)
    in2 = ((512 * xi - t_blur(xi) + 128) >> 8).clamp_(0, 255)
    a = t_weight(in1, n) + 0.1
    wn = a / (a + (t_weight(in2, n) + 0.1))
    gw, gd = [wn[..., None]], [(in1 - in2).to(torch.float64)]
    for _ in range(1, levels):
        gw.append(t_reduce(gw[-1]))
        gd.append(t_reduce(gd[-1]))
    acc = gw[-1] * gd[-1]
    for l in range(levels - 2, -1, -1):
        h, w = gd[l].shape[1:3]
        acc = gw[l] * (gd[l] - t_expand(gd[l + 1], h, w)) + t_expand(acc, h, w)
    return (in2.to(torch.float64) + acc).clamp_(0.0, 255.0).round_().to(torch.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    dev = uw.get_device(0)
    rng = np.random.default_rng(0)
    tw, th = _lib.fusion_plan(2160, 3840, LEVELS)
    print(f"level-0 tile {tw} x {th} per 256-thread workgroup, 2-pixel halo; L = {LEVELS}, gamma {GAMMA}; medians of {args.reps} alternated runs")
    table = dev.tensor(_lib.fusion_table(GAMMA))
    for B, H, W in SHAPES:
        host = cast_frames(rng, B, H, W)
        frames = dev.tensor(host)
        px = B * H * W
        ours = lambda: dev.fusion(frames, GAMMA, LEVELS)[0]  # noqa: E731
        out, parts = dev.fusion(frames, GAMMA, LEVELS, want_parts=True)
        want = ref.fusion(host[B - 1], GAMMA, LEVELS)
        got = [t[B - 1].cpu().numpy() for t in (out, *parts)]
        for name, g, w in zip(("out", "in1", "in2"), got, want):
            assert np.array_equal(g, w), f"{name} differs from the contract"
        assert np.array_equal(got[3].view(np.uint64), want[3].view(np.uint64)), "weights differ from the contract"
        del parts
        print(f"\n{B} x {H} x {W}: last frame equal to the contract (out, in1, in2, weight); workspace "
              f"{dev.lib.uwie_workspace_bytes_fusion(B, H, W, LEVELS) / px:.1f} B/px")

        names = ["k_fu_inputs", "k_fu_means", "k_fu_level0"] + [f"k_fu_reduce<{l}>" for l in range(1, LEVELS)]
        names += [f"k_fu_collapse<{l}>" for l in range(LEVELS - 1, -1, -1)]
        # bytes per level-0 pixel that a launch must move (halo re-reads not counted): see DESIGN.md section 27
        lv = [1.0 / 4 ** l for l in range(LEVELS)]
        bpp = [3 + 3, 0, 3 + 3 + 8 + 6] + [(8 + (6 if l == 1 else 24)) * lv[l - 1] + 32 * lv[l] for l in range(1, LEVELS)]
        for l in range(LEVELS - 1, -1, -1):
            top, own = l == LEVELS - 1, (8 + 6 + 3 + 3) if l == 0 else (8 + 24 + 24)
            bpp.append(own * lv[l] + (0 if top else 48 * lv[l + 1]))
        ms = kernel_ms(dev, [(n, ours) for n in names], args.reps)
        print(f"{'kernel':<18} {'B/px':>6} {'ms':>8} {'GB/s':>8}")
        for label, t, n in zip(names, ms, bpp):
            print(f"{label:<18} {n:6.2f} {t:8.3f} {n * px / t / 1e6:8.0f}")
        print(f"sum of the launches {sum(ms):.3f} ms = {px / sum(ms) / 1e6:.2f} Gpx/s")

        refs = torch.empty_like(frames).copy_(frames.flip(0))
        gw_out = torch.empty_like(frames)
        gray_world = lambda: dev.gray_world(frames, out=gw_out)  # noqa: E731
        scores = lambda: dev.reference_scores(frames, refs)  # noqa: E731
        c = call_ms([ours, gray_world, scores], args.reps)
        print(f"whole call: uwie_fusion_u8 {c[0]:.3f} ms | uwie_gray_world_u8 {c[1]:.3f} ms | uwie_reference_scores_u8 {c[2]:.3f} ms")
        del refs, gw_out
        torch.cuda.empty_cache()

        t_out = torch_fusion(frames, table, LEVELS)
        assert torch.equal(t_out, out), "torch float64 gives other bytes"
        del t_out
        c = call_ms([ours, lambda: torch_fusion(frames, table, LEVELS)], max(3, args.reps // 4))
        print(f"uwie_fusion_u8 {c[0]:.3f} ms | torch float64 tensor operations (equal bytes) {c[1]:.3f} ms | ratio {c[1] / c[0]:.1f}")
        assert dev.check_status() == 0
        del frames, out
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
