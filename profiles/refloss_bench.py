"""ReferenceLoss fused into the gated DifferentiableEnhancement's sweeps, per training step, against the unfused step.

Shapes: EndToEndTrainer's default batch 4 at 256x256, 32x224x224 and 8x4K (2160x3840), NCHW float32, parameters in
ParameterPredictor's ranges, parameter gradients only (the trainer's images do not require grad).  Rows:
  (a) module + torch ReferenceLoss   uw.GatedDifferentiableEnhancement, then deep_learning_parameters.ReferenceLoss's
                                     body in torch (l1_loss, mse_loss, 0.5 l1 + 0.5 l2, two .item()), backward: today's
                                     trainer step
  (b) fused                          uw.ReferenceLoss(0.5, 0.5).through(module, ...), backward (one host read per call)
  (c) module + sum(out * g)          the step of profiles/gated_grad_bench.py, whose loss costs nothing
Times are device events around `iters` steps after `warmup` steps, median of `reps` windows.  Row (d), the kernels on their
own, comes from a separate `rocprofv3 --kernel-trace --stats` run of `--kernels` (fused steps only).

Run:  python profiles/refloss_bench.py [--out FILE] [--kernels]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

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


def case(dev, B, H, W, log, kernels_only=False):
    gen = torch.Generator(device=dev.torch_device).manual_seed(B * H + W)
    x = torch.rand((B, 3, H, W), generator=gen, device=dev.torch_device)
    ref = torch.rand((B, 3, H, W), generator=gen, device=dev.torch_device)
    g = torch.randn((B, 3, H, W), generator=gen, device=dev.torch_device)
    L_low = torch.linspace(5.0, 20.0, B, device=dev.torch_device).reshape(B, 1)
    L_high = torch.linspace(98.0, 85.0, B, device=dev.torch_device).reshape(B, 1)
    u = torch.linspace(0.2, 0.9, B, device=dev.torch_device).reshape(B, 1).requires_grad_(True)
    ga = torch.linspace(1.0, 1.5, B, device=dev.torch_device).reshape(B, 1).requires_grad_(True)
    par = {"L_low": L_low, "L_high": L_high, "use_gamma": u, "gamma": ga}
    enh = uw.GatedDifferentiableEnhancement()
    crit = uw.ReferenceLoss(0.5, 0.5)
    tag = f"{B}x3x{H}x{W}"

    def unfused():
        u.grad = ga.grad = None
        out = enh(x, par)
        l1 = torch.nn.functional.l1_loss(out, ref)
        l2 = torch.nn.functional.mse_loss(out, ref)
        loss = 0.5 * l1 + 0.5 * l2
        _ = {"l1": l1.item(), "l2": l2.item()}
        loss.backward()

    def fused():
        u.grad = ga.grad = None
        loss, _ = crit.through(enh, x, par, ref)
        loss.backward()

    def sum_g():
        u.grad = ga.grad = None
        (enh(x, par) * g).sum().backward()

    iters, warmup = (20, 5) if B * H * W > 10**7 else (100, 20)
    if kernels_only:
        for _ in range(warmup + iters):
            fused()
        torch.cuda.synchronize()
        return
    rows = []
    for name, fn in (("(a) module + torch ReferenceLoss", unfused), ("(b) fused", fused), ("(c) module + sum(out * g)", sum_g)):
        med, lo, hi = timed(fn, iters, warmup)
        rows.append({"case": tag, "row": name, "ms": med, "min": lo, "max": hi})
    a, b, c = (r["ms"] for r in rows)
    rows[1]["vs (a)"] = b / a
    rows[1]["vs (c)"] = b / c
    dev.check_status()
    for r in rows:
        log(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in r.items()}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernels", action="store_true", help="fused steps only, for a rocprofv3 --kernel-trace --stats run")
    a = ap.parse_args()
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)

    dev = uw.get_device(0)
    log(f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}, libuwie {uw.load().uwie_version().decode()}")
    for B, H, W in ((4, 256, 256), (32, 224, 224), (8, 2160, 3840)):
        case(dev, B, H, W, log, a.kernels)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
