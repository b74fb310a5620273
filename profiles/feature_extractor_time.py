"""uw.FeatureExtractor on the device: ms per call of uwie_feature_extractor_u8 at 1080p x 16 and 4K x 4, and where the time goes.

Rows per shape:
  call     device events around `iters` calls after `warmup` calls (frames resident in HBM), median of `reps` windows
  kernels  the library's per-kernel HIP-event timing of one further call (uw.Device.profile)
  dct      the two DCT products' MACs (even / odd split: H W (W / 2) + W H (H / 2) per frame), their achieved TFLOP/s
           over the 157.3 TF f32 MFMA peak (MI355X spec)

Run:  python profiles/feature_extractor_time.py [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import features79_ref as R  # noqa: E402
import underwater_image_enhancement_amd as uw  # noqa: E402

F32_MFMA_PEAK_TF = 157.3


def time_calls(dev, t, iters, warmup, reps):
    for _ in range(warmup):
        dev.feature_extractor(t)
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            dev.feature_extractor(t)
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / iters)
    dev.check_status()
    return statistics.median(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    dev = uw.get_device(0)
    lines = []
    for B, H, W in ((16, 1080, 1920), (4, 2160, 3840)):
        frames = np.stack([R.frame("underwater", H, W, seed=i) for i in range(B)])
        t = torch.from_numpy(frames).to(dev.torch_device)
        ms = time_calls(dev, t, args.iters, args.warmup, args.reps)
        dev.profile(True)
        dev.feature_extractor(t)
        rows = dev.profile_rows()
        dev.profile(False)
        macs = B * (H * W * (W // 2) + W * H * (H // 2))
        dct_ms = sum(v[0] for k, v in rows.items() if k.startswith("k_fx_dct"))
        tf = 2 * macs / (dct_ms * 1e-3) / 1e12 if dct_ms else float("nan")
        rec = {"shape": f"{B}x{H}x{W}", "ms_per_call": round(ms, 3), "ms_per_frame": round(ms / B, 3),
               "kernels_ms": {k: round(v[0], 3) for k, v in sorted(rows.items(), key=lambda kv: -kv[1][0])},
               "dct_gmac": round(macs / 1e9, 2), "dct_ms": round(dct_ms, 3), "dct_tflops": round(tf, 1),
               "dct_of_f32_mfma_peak": round(tf / F32_MFMA_PEAK_TF, 3)}
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
