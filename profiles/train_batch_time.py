"""Trainer input batches on the device (uwie_resize_rgb_u8, k_resize.hip): what the resize kernel costs, what a whole
training_batch call costs, and the per-image CPU time of the NumPy restatement.

Rows:
  kernel    device events around `iters` Device.resize_rgb calls (u8 + float32 outputs, frames already in HBM, the
            descriptor table rebuilt each call as the API does), median of `reps` windows; plus the kernel alone from the
            library's per-kernel event timing (uw.Device.profile) and the bytes it moves
  batch     uw.training_batch from host NumPy frames (pinned packing, H2D, resize, features), wall clock per call after a
            warm-up, for features="extractor" and "basic"
  numpy     tests/resize_ref.py's resize of one frame on the CPU (the restatement, NOT OpenCV, which is absent here)

Run:  python profiles/train_batch_time.py [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import resize_ref as R  # noqa: E402
import underwater_image_enhancement_amd as uw  # noqa: E402

SHAPES = ((32, 1080, 1920, 256), (16, 2160, 3840, 224), (64, 720, 1280, 224))


def frames_for(B, H, W):
    base = R.synth_frame(H, W, seed=H)
    return [np.roll(base, 13 * i, axis=1) for i in range(B)]


def time_kernel(dev, t, size, iters, warmup, reps):
    for _ in range(warmup):
        dev.resize_rgb(t, size, size, want_f32=True)
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            dev.resize_rgb(t, size, size, want_f32=True)
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / iters)
    dev.profile(True, only="k_resize_rgb")
    dev.resize_rgb(t, size, size, want_f32=True)
    rows = dev.profile_rows()
    dev.profile(False)
    dev.check_status()
    return statistics.median(ms), rows.get("k_resize_rgb", (float("nan"), 0))[0]


def time_batch(frames, size, features, iters):
    uw.training_batch(frames, size=size, features=features)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        uw.training_batch(frames, size=size, features=features)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batch-iters", type=int, default=3)
    args = ap.parse_args()
    dev = uw.get_device(0)
    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    for B, H, W, size in SHAPES:
        frames = frames_for(B, H, W)
        t = torch.from_numpy(np.stack(frames)).to(dev.torch_device)
        call_ms, kern_ms = time_kernel(dev, t, size, args.iters, args.warmup, args.reps)
        # source bytes the kernel can touch (two rows per output row, or all of them when rows are fewer), outputs written
        rows_read = min(H, 2 * size)
        moved = B * (rows_read * W * 3 + size * size * 3 * (1 + 4))
        emit({"row": "kernel", "shape": f"{B}x{H}x{W}->{size}", "call_ms": round(call_ms, 4), "kernel_ms": round(kern_ms, 4),
              "bytes_mb": round(moved / 1e6, 2), "gbps": round(moved / (kern_ms * 1e-3) / 1e9, 1)})
        del t
        for feats in ("extractor", "basic"):
            ms = time_batch(frames, size, feats, args.batch_iters)
            emit({"row": "batch", "shape": f"{B}x{H}x{W}->{size}", "features": feats, "ms_per_call": round(ms, 2),
                  "ms_per_image": round(ms / B, 3), "h2d_mb": round(B * H * W * 3 / 1e6, 1)})
        t0 = time.perf_counter()
        for f in frames[:4]:
            R.resize(f, (size, size))
        emit({"row": "numpy", "shape": f"{H}x{W}->{size}", "what": "tests/resize_ref.py restatement, not OpenCV",
              "ms_per_image": round((time.perf_counter() - t0) * 1e3 / 4, 2)})
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
