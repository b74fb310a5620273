"""uw.StrategyClassifier on the device: ms per call of uwie_classify_f64 (predict_rows) at B = 64 and 4096 rows for the
fixture's config-sized five-class models (tests/golden/classifier.npz: RF 200 trees, GB 100 stages x 5, SVC), and of
uwie_predict_strategy_u8 (predict) at 4K x 16.  Run it under ``rocprofv3 --kernel-trace --stats`` for the kernel table.

Rows: device events around `iters` calls after `warmup` calls (inputs resident in HBM), median of `reps` windows.

Run:  python profiles/classifier_time.py [--out FILE]
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import gen_golden_classifier as gen  # noqa: E402
import underwater_image_enhancement_amd as uw  # noqa: E402


def time_ms(fn, iters, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / iters)
    return statistics.median(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    with np.load(os.path.join(ROOT, "tests", "golden", "classifier.npz"), allow_pickle=False) as z:
        golden = {k: z[k] for k in z.files}
    dev = uw.get_device()
    X = golden["c5_X"]
    X = X[~np.isnan(X).any(axis=1)]
    lines = []
    for kind in ("rf", "gb", "svc"):
        clf = uw.StrategyClassifier(gen.arrays_of(golden, f"c5_{kind}"))
        h = clf._model(dev)
        for B in (64, 4096):
            rows = torch.from_numpy(np.resize(X, (B, 79)).copy()).to(dev.torch_device)
            label = dev.empty((B,), torch.int32)
            proba = dev.empty((B, 5), torch.float64)

            def call():
                uw._lib.check(dev.lib.uwie_classify_f64(dev._ctx, h, ctypes.c_void_p(rows.data_ptr()), B, 79,
                                                        ctypes.c_void_p(label.data_ptr()), ctypes.c_void_p(proba.data_ptr()),
                                                        dev.stream()))

            ms = time_ms(call, args.iters, 3, 5)
            dev.check_status()
            lines.append({"what": "classify_f64", "model": kind, "rows": B, "ms_per_call": round(ms, 4),
                          "us_per_row": round(1000 * ms / B, 4)})
    clf = uw.StrategyClassifier(gen.arrays_of(golden, "c5_rf"))
    g = torch.Generator(device=dev.torch_device).manual_seed(0)
    frames = torch.randint(0, 256, (16, 2160, 3840, 3), dtype=torch.uint8, device=dev.torch_device, generator=g)
    ms = time_ms(lambda: clf._predict_device(dev, frames, None), 5, 2, 3)
    dev.check_status()
    lines.append({"what": "predict_strategy_u8", "model": "rf", "shape": "16x2160x3840", "ms_per_call": round(ms, 3)})
    text = "\n".join(json.dumps(r) for r in lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
