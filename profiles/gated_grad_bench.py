"""The gated-gamma DifferentiableEnhancement (deep_learning_parameters.py:24-90) forward + backward on the device, per
training step, against the same step in torch ops on the same GPU.

Shapes: EndToEndTrainer's default batch 4 at 256x256, 32x224x224 and 8x4K (2160x3840), NCHW float32, with L_low, L_high,
use_gamma and gamma in ParameterPredictor's ranges.  Rows:
  step      forward + backward through uw.GatedDifferentiableEnhancement (loss = sum(out * g)), with / without grad_img;
            each call waits for the device once (the sorted-position check)
  bwd       the backward entry alone (uwie_diff_gated_bwd_f32), with / without grad_img, and its algorithmic traffic
            (12 B/px x, 12 B/px grad_out, 12 B/px grad_img) over that time
  forward   the inference entry alone (uwie_diff_gated_f32, no wait)
  torch     the same step in torch ops: the reference's structure (a loop over the B*3 planes, each a full torch.sort and
            two .item() reads, then the gate; autograd), and the batched restatement (tests/dlp_grad_ref.py: one sort)
Times are device events around `iters` steps after `warmup` steps, median of `reps` windows.

Run:  python profiles/gated_grad_bench.py [--out FILE]
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

import dlp_grad_ref as R  # noqa: E402
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


def per_plane(img, p):
    """The reference module's operation sequence in torch ops: per plane a full sort and two host reads of L."""
    B, C, H, W = img.shape
    n = H * W
    enhanced = torch.zeros_like(img)
    for b in range(B):
        for c in range(C):
            ch = img[b, c]
            sv, _ = torch.sort(ch.flatten())
            k_lo, k_hi = int(p["L_low"][b].item() / 100.0 * n), int(p["L_high"][b].item() / 100.0 * n)
            enhanced[b, c] = torch.clamp((ch - sv[k_lo]) / (sv[k_hi] - sv[k_lo] + 1e-8), 0, 1)
    u, ga = p["use_gamma"].view(-1, 1, 1, 1), p["gamma"].view(-1, 1, 1, 1)
    return torch.clamp(u * torch.pow(enhanced + 1e-8, 1.0 / ga) + (1 - u) * enhanced, 0, 1)


def case(dev, B, H, W, log):
    gen = torch.Generator(device=dev.torch_device).manual_seed(B * H + W)
    x = torch.rand((B, 3, H, W), generator=gen, device=dev.torch_device)
    g = torch.randn((B, 3, H, W), generator=gen, device=dev.torch_device)
    L_low = torch.linspace(5.0, 20.0, B, device=dev.torch_device).reshape(B, 1)
    L_high = torch.linspace(98.0, 85.0, B, device=dev.torch_device).reshape(B, 1)
    u = torch.linspace(0.2, 0.9, B, device=dev.torch_device).reshape(B, 1).requires_grad_(True)
    ga = torch.linspace(1.0, 1.5, B, device=dev.torch_device).reshape(B, 1).requires_grad_(True)
    par = {"L_low": L_low, "L_high": L_high, "use_gamma": u, "gamma": ga}
    enh = uw.GatedDifferentiableEnhancement()
    npx = B * H * W
    tag = f"{B}x3x{H}x{W}"

    def step(img):
        def run():
            u.grad = ga.grad = None
            if img.requires_grad:
                img.grad = None
            (enh(img, par) * g).sum().backward()
        return run

    iters, warmup = (20, 5) if npx > 10**7 else (100, 20)
    xg = x.clone().requires_grad_(True)
    rows = []
    for name, img in (("step grad_img+params", xg), ("step params only", x)):
        med, lo, hi = timed(step(img), iters, warmup)
        rows.append({"case": tag, "row": name, "ms": med, "min": lo, "max": hi})
    p = torch.cat([L_low, L_high, u.detach(), ga.detach()], dim=1).contiguous()
    out, saved = dev.diff_gated_save_f32(x, p, True)
    for want_img in (True, False):
        med, lo, hi = timed(lambda: dev.diff_gated_bwd_f32(x, p, saved, g, True, want_img=want_img), iters, warmup)
        nbytes = npx * 3 * 4 * (3 if want_img else 2)
        rows.append({"case": tag, "row": "bwd " + ("grad_img+params" if want_img else "params only"), "ms": med, "min": lo,
                     "max": hi, "GB": nbytes / 1e9, "TB/s": nbytes / (med * 1e-3) / 1e12, "of 8 TB/s": nbytes / (med * 1e-3) / 8e12})
    med, lo, hi = timed(lambda: dev.diff_gated_f32(x, p, True), iters, warmup)
    rows.append({"case": tag, "row": "forward alone (inference entry)", "ms": med, "min": lo, "max": hi})
    dev.check_status()

    def ref_loop():
        xg.grad = u.grad = ga.grad = None
        (per_plane(xg, par) * g).sum().backward()

    def ref_batched():
        xg.grad = u.grad = ga.grad = None
        (R.gated(xg, L_low, L_high, u, ga) * g).sum().backward()

    for name, fn in (("torch ops, reference structure (sort + 2 .item() per plane), grad_img+params", ref_loop),
                     ("torch ops, batched restatement (one stable sort), grad_img+params", ref_batched)):
        med, lo, hi = timed(fn, max(2, iters // 10), 2, reps=3)
        rows.append({"case": tag, "row": name, "ms": med, "min": lo, "max": hi})
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
    case(dev, 4, 256, 256, log)
    case(dev, 32, 224, 224, log)
    case(dev, 8, 2160, 3840, log)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
