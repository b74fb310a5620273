#!/usr/bin/env python3
"""What the full-reference scores (uwie_reference_scores_u8: MAE, MSE, PSNR, SSIM; DESIGN.md "Full-reference quality") cost.

1. The three kernels: k_rq_stream (integer sums of the differences), k_rq_tiles (the SSIM pass: four planes, five window sums
   per map point in float64) and k_rq_finish, each timed by the library's HIP-event pair with the profile filter on that one
   kernel, alternated launch by launch in one process.
2. The whole call against
   - the same eight numbers from torch ops on the device, which is what a user would otherwise write: the planes as float64,
     two depthwise conv2d calls (1 x 11, then 11 x 1) with the same taps for each of the five window sums, the rest
     elementwise; if conv2d refuses float64 on this build, the same sums as eleven shifted slices per direction;
   - uwie_underwater_scores_u8 on the same frames,
   alternated call by call.

at 16 x 2160 x 3840 and 8 x 1080 x 1920, random bytes against the same bytes with a bounded perturbation.  Before anything is
timed, the last frame's scores are compared with the definition's (tests/ref_quality_ref.py) and the torch formulation's with
the call's.

usage: python profiles/ref_quality_bench.py [--reps N] [--out FILE]      (profiles/ref_quality_bench.txt holds the default output)"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import underwater_image_enhancement_amd as uw  # noqa: E402
from underwater_image_enhancement_amd import _lib  # noqa: E402
import ref_quality_ref as ref  # noqa: E402

SHAPES = ((16, 2160, 3840), (8, 1080, 1920))
KERNELS = ("k_rq_stream", "k_rq_tiles", "k_rq_finish")


class TorchScores:
    """The eight numbers from torch ops: u8 cuda [B,H,W,3] pairs -> float64 [B,8]."""

    def __init__(self, device):
        self.w = torch.from_numpy(ref.taps()).to(device)
        self.route = "conv2d"
        try:
            self.window(torch.zeros((1, 4, 11, 11), dtype=torch.float64, device=device))
        except RuntimeError:
            self.route = "slices"

    def window(self, v):
        if self.route == "conv2d":
            c = v.shape[1]
            rows = torch.nn.functional.conv2d(v, self.w.view(1, 1, 1, 11).repeat(c, 1, 1, 1), groups=c)
            return torch.nn.functional.conv2d(rows, self.w.view(1, 1, 11, 1).repeat(c, 1, 1, 1), groups=c)
        H, W = v.shape[2:]
        rows = sum(self.w[k] * v[..., k:W - 10 + k] for k in range(11))
        return sum(self.w[k] * rows[..., k:H - 10 + k, :] for k in range(11))

    @staticmethod
    def planes(f):
        i = f.to(torch.int32)
        gray = (i[..., 0] * 9798 + i[..., 1] * 19235 + i[..., 2] * 3735 + 16384) >> 15
        return torch.cat([gray.unsqueeze(1), i.permute(0, 3, 1, 2)], dim=1).to(torch.float64)

    def __call__(self, xs, ys):
        d = xs.to(torch.int64) - ys.to(torch.int64)
        n3 = float(d[0].numel())
        mae, mse = d.abs().sum(dim=(1, 2, 3)).double() / n3, (d * d).sum(dim=(1, 2, 3)).double() / n3
        psnr = torch.where(mse == 0, torch.full_like(mse, float("inf")), 10 * torch.log10(65025.0 / mse))
        x, y = self.planes(xs), self.planes(ys)
        mx, my = self.window(x), self.window(y)
        vx, vy, cv = self.window(x * x) - mx * mx, self.window(y * y) - my * my, self.window(x * y) - mx * my
        s = ((2 * mx * my + ref.C1) * (2 * cv + ref.C2)) / ((mx * mx + my * my + ref.C1) * (vx + vy + ref.C2))
        m = s.mean(dim=(2, 3))
        return torch.cat([mae[:, None], mse[:, None], psnr[:, None], m, m[:, 1:].sum(dim=1, keepdim=True) / 3], dim=1)


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
    for r in range(reps):
        order = range(len(fns)) if r % 2 == 0 else reversed(range(len(fns)))  # alternating order
        for i in order:
            ev[0].record()
            fns[i]()
            ev[1].record()
            torch.cuda.synchronize()
            ms[i].append(ev[0].elapsed_time(ev[1]))
    return [float(np.median(m)) for m in ms]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ref_quality_bench.txt"))
    args = ap.parse_args()
    lines = []

    def say(text=""):
        print(text, flush=True)
        lines.append(text)

    dev = uw.get_device(0)
    rng = np.random.default_rng(0)
    tw, th = _lib.reference_plan(2160, 3840)
    by_torch = TorchScores(dev.torch_device)
    say(f"k_rq_tiles: {tw} x {th} map points per 256-thread workgroup; medians of {args.reps} alternated runs; torch formulation: "
        f"float64 {by_torch.route}")
    for B, H, W in SHAPES:
        host_y = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
        host_x = np.clip(host_y.astype(np.int16) + rng.integers(-24, 25, host_y.shape, dtype=np.int16), 0, 255).astype(np.uint8)
        xs, ys = dev.tensor(host_x), dev.tensor(host_y)
        px = B * H * W
        ours = lambda: dev.reference_scores(xs, ys)  # noqa: E731
        torched = lambda: by_torch(xs, ys)  # noqa: E731
        under = lambda: dev.underwater_scores(xs)  # noqa: E731
        got = ours().cpu().numpy()
        want = ref.scores(host_x[B - 1], host_y[B - 1])
        err = np.abs(got[B - 1] - want)
        assert got[B - 1, :2].tobytes() == want[:2].tobytes() and err.max() <= 1e-9, (got[B - 1], want)
        terr = np.abs(torched().cpu().numpy() - got).max()
        assert terr <= 1e-9, terr
        ms = kernel_ms(dev, [(k, ours) for k in KERNELS], args.reps)
        say(f"\n{B} x {H} x {W}: last frame within {err.max():.1e} of the definition, torch formulation within {terr:.1e} of the call")
        say(f"{'kernel':<16} {'ms':>8} {'Gpx/s':>8}")
        for label, t in zip(KERNELS, ms):
            say(f"{label:<16} {t:8.3f} {px / t / 1e6:8.1f}")
        c = call_ms([ours, torched, under], max(3, args.reps // 4))
        say(f"whole call: uwie_reference_scores_u8 {c[0]:.3f} ms | torch float64 {by_torch.route} {c[1]:.3f} ms ({c[1] / c[0]:.1f} x) | "
            f"uwie_underwater_scores_u8 {c[2]:.3f} ms")
        assert c[0] < c[1], "the kernel has no reason to exist"
        assert dev.check_status() == 0
        del xs, ys
        torch.cuda.empty_cache()
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
