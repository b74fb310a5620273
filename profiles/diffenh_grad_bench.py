"""DifferentiableEnhancement forward + backward on the device, per training step, against the same step in torch ops.

Shapes: the trainer's 224x224 (vgg_16_UIE.py target_size) at batch 32, and 4K (2160x3840) at batch 8, NCHW float32, with
omega and gamma.  Rows:
  step      forward + backward through uw.DifferentiableEnhancement (loss = sum(out * g)), with / without grad_img
  bwd       the backward entry alone (uwie_diff_enhance_bwd_f32), with / without grad_img, and its algorithmic traffic
            (12 B/px x, 12 B/px grad_out, 12 B/px grad_img) over that time
  torch     the same step through the torch-op restatement (tests/diffenh_grad_ref.py: one torch.sort per plane, autograd)
Times are device events around `iters` steps after `warmup` steps, median of `reps` windows.

Run:  python profiles/diffenh_grad_bench.py [--out FILE]
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

import diffenh_grad_ref as R  # noqa: E402
import underwater_image_enhancement_amd as uw  # noqa: E402


def timed(fn, iters, warmup, reps=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / iters)
    return statistics.median(out), min(out), max(out)


def case(dev, B, H, W, log, torch_ref=True):
    gen = torch.Generator(device=dev.torch_device).manual_seed(B * H + W)
    x = torch.rand((B, 3, H, W), generator=gen, device=dev.torch_device)
    g = torch.randn((B, 3, H, W), generator=gen, device=dev.torch_device)
    L_low = torch.full((B, 1), 5.0, device=dev.torch_device)
    L_high = torch.full((B, 1), 95.0, device=dev.torch_device)
    om = torch.linspace(0.3, 0.8, B, device=dev.torch_device).reshape(B, 1).requires_grad_(True)
    ga = torch.linspace(0.7, 1.8, B, device=dev.torch_device).reshape(B, 1).requires_grad_(True)
    enh = uw.DifferentiableEnhancement()
    npx = B * H * W
    tag = f"{B}x3x{H}x{W}"

    def step(img):
        def run():
            om.grad = ga.grad = None
            if img.requires_grad:
                img.grad = None
            (enh(img, {"L_low": L_low, "L_high": L_high, "omega": om, "gamma": ga}) * g).sum().backward()
        return run

    iters, warmup = (20, 5) if npx > 10**7 else (100, 20)
    xg = x.clone().requires_grad_(True)
    rows = []
    for name, img in (("step grad_img+params", xg), ("step params only", x)):
        med, lo, hi = timed(step(img), iters, warmup)
        rows.append({"case": tag, "row": name, "ms": med, "min": lo, "max": hi})
    p = torch.cat([L_low, L_high, om.detach(), ga.detach()], dim=1).contiguous()
    out, saved = dev.diff_enhance_save_f32(x, p, True, 3)
    for want_img in (True, False):
        med, lo, hi = timed(lambda: dev.diff_enhance_bwd_f32(x, p, saved, g, True, 3, want_img=want_img), iters, warmup)
        nbytes = npx * 3 * 4 * (3 if want_img else 2)
        rows.append({"case": tag, "row": "bwd " + ("grad_img+params" if want_img else "params only"), "ms": med, "min": lo,
                     "max": hi, "GB": nbytes / 1e9, "TB/s": nbytes / (med * 1e-3) / 1e12, "of 8 TB/s": nbytes / (med * 1e-3) / 8e12})
    med, lo, hi = timed(lambda: dev.diff_enhance_f32(x, p, True), iters, warmup)
    rows.append({"case": tag, "row": "forward alone (inference entry)", "ms": med, "min": lo, "max": hi})
    if torch_ref:
        def ref():
            xg.grad = om.grad = ga.grad = None
            (R.diff_enhance(xg, L_low, L_high, om, ga) * g).sum().backward()
        med, lo, hi = timed(ref, max(2, iters // 10), 2, reps=3)
        rows.append({"case": tag, "row": "torch ops (sort per plane, autograd), grad_img+params", "ms": med, "min": lo, "max": hi})
    base = next(r["ms"] for r in rows if r["row"] == "step grad_img+params")
    for r in rows:
        if r["row"].startswith("torch"):
            r["speedup of the device step"] = r["ms"] / base
    for r in rows:
        log(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in r.items()}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)

    dev = uw.get_device(0)
    log(f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}, libuwie {uw.load().uwie_version().decode()}")
    case(dev, 32, 224, 224, log)
    case(dev, 8, 2160, 3840, log)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
